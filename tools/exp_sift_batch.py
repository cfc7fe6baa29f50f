"""dev helper: pcc_sift_keypoints_batch against the loop it replaces, per COMPARISON (SIFT keypoints plus the keypoint snap of
every cluster above 700 points of both scenes, reference src/comparator.cpp:1228-1231, :1264-1265, :686-822).  In ONE process, on
one context handle and one loop handle, alternating:
  batch   one pcc_sift_keypoints_batch (with the snap) for all clusters
  loop    set_input + sift_keypoints + first_within per cluster on one re-pointed handle (what pcc::siftSnappedCloud does per
          cluster; its device code is the parent commit's), timed twice: the difference between its two columns is the
          run-to-run spread the other differences have to beat
  host    the one-core host mirror (build/sift_host), the sum of its own per-cluster timings (detector only, no snap)
Workloads: 2 x 30 clusters of 1000 points, 2 x 30 of 3000, and 60 clusters drawn from 701 ... 8000 points; clouds from
synth.rift_cloud at the density of the test scenes, all in one corner of space.
Then ONE cloud alone through either route of the batch call (PCC_OPT_SIFT_BATCH_BRUTE_MAX above / below its size) and through
the single calls, 2048 ... 32768 points: the crossover of a cloud on its own; and the mixed workload under several values of
the option: what the same choice costs a cloud that has others beside it.  Both stand behind the option's default.
Every slice of the batch is checked bit for bit against the host mirror (keypoints) and the loop (keypoints and snapped
indices) before anything is timed.  Host clock around calls that end in a synchronise; every shape warmed up; each figure from a
window of at least --window seconds.
usage: exp_sift_batch.py [--window SECONDS] [--no-host] [--no-sweep] [--trace]
  --trace   for a rocprofv3 --kernel-trace --stats run of its own: 10 batch calls over 60 clusters and 10 over 10 clusters,
            nothing else -- every kernel's dispatch count is the same whatever the cluster count"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import sift_util
from pointcloudcomparator_amd import capi, synth

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, default=0.2)
ap.add_argument("--no-host", action="store_true", help="leave the one-core host mirror out (the batch is then checked against the loop alone)")
ap.add_argument("--no-sweep", action="store_true")
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()
SNAP = 0.05


def cloud(n, seed):
    p, rgb = synth.rift_cloud(n, seed, extent=0.12 * (n / 600.0) ** (1.0 / 3.0))
    return p, synth.pack_rgb(rgb), rgb


def window(fn, seconds):
    """milliseconds per call of fn over a window of at least `seconds` (fn ends in a synchronise)"""
    fn()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n * 1e3


def same_bits(a, b):
    return a.shape == b.shape and (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all()


rng = np.random.default_rng(20261018)
mixed = np.round(np.exp(rng.uniform(np.log(701), np.log(8000), 60))).astype(int)
WORKLOADS = {
    "2x30x1000": [1000] * 60,
    "2x30x3000": [3000] * 60,
    "mixed60": [int(v) for v in mixed],
}

ctx = capi.Index(np.zeros((1, 3), np.float32), engine=capi.ENGINE_BRUTE, device=0)
if args.trace:
    for sizes in ([1000] * 60, [1000] * 10):
        clouds = [cloud(n, 500 + k) for k, n in enumerate(sizes)]
        for _ in range(10):
            ctx.sift_keypoints_batch([c[0] for c in clouds], [c[1] for c in clouds], snap_radius=SNAP)
        print(f"{len(sizes)} clusters: {int(ctx.stats()[2])} octave rounds per call")
    print("batch calls: 10 over 60 clusters, 10 over 10 clusters")
    ctx.close()
    sys.exit(0)

if not args.no_host:
    subprocess.check_call(["make", "build/sift_host"], cwd=ROOT, stdout=subprocess.DEVNULL)
tmp = tempfile.mkdtemp()
loop_ix = capi.Index(cloud(300, 1)[0], engine=capi.ENGINE_GRID, device=0)


def single(p, w):
    loop_ix.set_input(p)
    kp = loop_ix.sift_keypoints(p, w)
    snap = loop_ix.first_within(np.ascontiguousarray(kp[:, :3]), SNAP) if len(kp) else np.zeros(0, np.int32)
    return kp, snap


print(f"{'workload':9s} {'clusters':>8s} {'points':>7s} {'keypoints':>9s} {'rounds':>6s} | {'batch ms':>9s} {'loop ms':>9s} {'loop again':>10s} "
      f"{'host 1 core ms':>14s} | loop / batch")
for name, sizes in WORKLOADS.items():
    clouds = [cloud(n, 500 + k) for k, n in enumerate(sizes)]
    pts, words = [c[0] for c in clouds], [c[1] for c in clouds]

    def batch():
        return ctx.sift_keypoints_batch(pts, words, snap_radius=SNAP)

    def loop():
        return [single(p, w) for p, w in zip(pts, words)]

    (kp, off, snap), ref = batch(), loop()
    rounds = int(ctx.stats()[2])
    host_ms = float("nan")
    if not args.no_host:
        host_ms = 0.0
        for k, c in enumerate(clouds):
            h = sift_util.run_host(c[0], c[2], tmp, tag="c")
            host_ms += float(h["info"]["ms"])
            assert same_bits(kp[off[k]:off[k + 1]], h["keypoints"]), f"{name}: cluster {k} differs from the host mirror"
    bad = [k for k in range(len(clouds)) if not (same_bits(kp[off[k]:off[k + 1]], ref[k][0]) and np.array_equal(snap[off[k]:off[k + 1]], ref[k][1]))]
    assert not bad, f"{name}: clusters {bad[:5]} differ from the loop"
    t = [0.0, 0.0, 0.0]
    for rep in range(2):  # alternating, two rounds; the batch figure is the mean of its two windows
        t[0] += window(batch, args.window) / 2
        t[1 + rep] = window(loop, args.window)
    print(f"{name:9s} {len(sizes):8d} {sum(sizes):7d} {len(kp):9d} {rounds:6d} | {t[0]:9.3f} {t[1]:9.3f} {t[2]:10.3f} {host_ms:14.1f} | "
          f"{min(t[1], t[2]) / t[0]:.2f}", flush=True)

if not args.no_sweep:
    default = ctx.get_option(capi.OPT_SIFT_BATCH_BRUTE_MAX)
    print(f"\none cloud alone (PCC_OPT_SIFT_BATCH_BRUTE_MAX default {default:.0f})")
    print(f"{'points':>7s} {'keypoints':>9s} | {'batch kernels ms':>16s} {'batch, work handle ms':>21s} {'single calls ms':>15s} {'single again':>12s}")
    for n in (2048, 4096, 8192, 16384, 32768):
        p, w, _ = cloud(n, 17)

        def one():
            return ctx.sift_keypoints_batch([p], [w], snap_radius=SNAP)

        ref = single(p, w)
        for label, limit in (("brute", 1 << 30), ("work", 0)):
            ctx.set_option(capi.OPT_SIFT_BATCH_BRUTE_MAX, limit)
            kp, off, snap = one()
            assert same_bits(kp, ref[0]) and np.array_equal(snap, ref[1]), f"{n} points, {label} route differs from the single calls"
        t = {"brute": 0.0, "work": 0.0}
        s = [0.0, 0.0]
        for rep in range(2):
            for label, limit in (("brute", 1 << 30), ("work", 0)):
                ctx.set_option(capi.OPT_SIFT_BATCH_BRUTE_MAX, limit)
                t[label] += window(one, args.window) / 2
            s[rep] = window(lambda: single(p, w), args.window)
        ctx.set_option(capi.OPT_SIFT_BATCH_BRUTE_MAX, default)
        print(f"{n:7d} {len(ref[0]):9d} | {t['brute']:16.3f} {t['work']:21.3f} {s[0]:15.3f} {s[1]:12.3f}", flush=True)
    # the same choice for clouds that have others beside them: the mixed workload under several limits
    clouds = [cloud(n, 500 + k) for k, n in enumerate(WORKLOADS["mixed60"])]
    pts, words = [c[0] for c in clouds], [c[1] for c in clouds]
    limits = (2048, 3072, 4096, 6144, 8192, 1 << 30)
    print(f"\nmixed60 under PCC_OPT_SIFT_BATCH_BRUTE_MAX (clusters on the work handle / batch ms)")
    t = {limit: 0.0 for limit in limits}
    for rep in range(2):
        for limit in limits:
            ctx.set_option(capi.OPT_SIFT_BATCH_BRUTE_MAX, limit)
            t[limit] += window(lambda: ctx.sift_keypoints_batch(pts, words, snap_radius=SNAP), args.window) / 2
    ctx.set_option(capi.OPT_SIFT_BATCH_BRUTE_MAX, default)
    for limit in limits:
        print(f"{limit:10d} {sum(len(p) > limit for p in pts):3d} {t[limit]:9.3f}", flush=True)
loop_ix.close()
ctx.close()
