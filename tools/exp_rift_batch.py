"""dev helper: pcc_rift_descriptors_batch against the loop it replaces, per COMPARISON (the descriptors of every cluster of both
scenes, reference src/comparator.cpp:1224-1272).  In ONE process, on one context handle and one loop handle, alternating:
  batch   one pcc_rift_descriptors_batch for all clusters
  loop    set_input + rift_descriptors per cluster on one re-pointed handle (what pcc::processRIFT does per cluster; its device
          code is the parent commit's), timed twice: the difference between its two columns is the run-to-run spread the other
          differences have to beat
  host    the one-core host mirror (build/rift_host), the sum of its own per-cluster timings
Workloads: 2 x 30 clusters of 300 points (the projection of EXPERIMENTS.md, "RIFT descriptors"), 2 x 30 of 700, and a mixed set
of 60 clusters of 20 ... 5000 points; clouds from synth.rift_cloud at the density of the test scenes, all in one corner of space.
Then ONE cloud alone through either route of the batch call (PCC_OPT_RIFT_BATCH_BRUTE_MAX above / below its size) and through
the single call, 300 ... 50 000 points: the crossover behind the option's default.
Every slice of the batch is checked bit for bit against the host mirror (workloads) or the single call (one cloud alone) before
anything is timed.  Host clock around calls that end in a synchronise; every shape warmed up; each figure from a window of at
least --window seconds.
usage: exp_rift_batch.py [--window SECONDS] [--no-host] [--no-sweep] [--trace]
  --trace   for a rocprofv3 --kernel-trace --stats run of its own: 10 batch calls over 60 clusters and 10 over 10 clusters,
            nothing else -- every kernel's dispatch count is the same multiple of 20 whatever the cluster count"""
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
import rift_util
from pointcloudcomparator_amd import capi, synth

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, default=0.2)
ap.add_argument("--no-host", action="store_true", help="leave the one-core host mirror out (the batch is then checked against the loop)")
ap.add_argument("--no-sweep", action="store_true")
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()


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


def same(a, b):
    return np.array_equal(a[1], b[1]) and a[0].shape == b[0].shape and (a[0].view(np.uint32) == b[0].view(np.uint32)).all()


rng = np.random.default_rng(20251017)
mixed = np.round(np.exp(rng.uniform(np.log(20), np.log(5000), 60))).astype(int)
WORKLOADS = {
    "2x30x300": [300] * 60,
    "2x30x700": [700] * 60,
    "mixed60": [int(v) for v in mixed],
}

ctx = capi.Index(np.zeros((1, 3), np.float32), engine=capi.ENGINE_BRUTE, device=0)
if args.trace:
    for sizes in ([300] * 60, [300] * 10):
        clouds = [cloud(n, 500 + k) for k, n in enumerate(sizes)]
        for _ in range(10):
            ctx.rift_descriptors_batch([c[0] for c in clouds], [c[1] for c in clouds])
    print("batch calls: 10 over 60 clusters, 10 over 10 clusters")
    ctx.close()
    sys.exit(0)

if not args.no_host:
    subprocess.check_call(["make", "build/rift_host"], cwd=ROOT, stdout=subprocess.DEVNULL)
tmp = tempfile.mkdtemp()
loop_ix = capi.Index(cloud(300, 1)[0], engine=capi.ENGINE_GRID, device=0)
print(f"{'workload':9s} {'clusters':>8s} {'points':>7s} {'kept':>7s} | {'batch ms':>9s} {'loop ms':>9s} {'loop again':>10s} {'host 1 core ms':>14s} | loop / batch")
for name, sizes in WORKLOADS.items():
    clouds = [cloud(n, 500 + k) for k, n in enumerate(sizes)]
    pts, words = [c[0] for c in clouds], [c[1] for c in clouds]

    def batch():
        return ctx.rift_descriptors_batch(pts, words)

    def loop():
        out = []
        for p, w in zip(pts, words):
            loop_ix.set_input(p)
            out.append(loop_ix.rift_descriptors(w))
        return out

    got, ref = batch(), loop()
    host_ms = float("nan")
    if not args.no_host:
        host_ms = 0.0
        for k, c in enumerate(clouds):
            h, i, out = rift_util.run_tool(rift_util.HOST, c[0], c[2], tmp, tag="c")
            host_ms += float(out.split("ms=")[1])
            assert same(got[k], (h, i)), f"{name}: cluster {k} differs from the host mirror"
    bad = [k for k in range(len(clouds)) if not same(got[k], ref[k])]
    assert not bad, f"{name}: clusters {bad[:5]} differ from the loop"
    t = [0.0, 0.0, 0.0]
    for rep in range(2):  # alternating, two rounds; the batch figure is the mean of its two windows
        t[0] += window(batch, args.window) / 2
        t[1 + rep] = window(loop, args.window)
    print(f"{name:9s} {len(sizes):8d} {sum(sizes):7d} {sum(len(g[1]) for g in got):7d} | {t[0]:9.3f} {t[1]:9.3f} {t[2]:10.3f} {host_ms:14.1f} | "
          f"{min(t[1], t[2]) / t[0]:.2f}", flush=True)

if not args.no_sweep:
    default = ctx.get_option(capi.OPT_RIFT_BATCH_BRUTE_MAX)
    print(f"\none cloud alone (PCC_OPT_RIFT_BATCH_BRUTE_MAX default {default:.0f})")
    print(f"{'points':>7s} {'kept':>7s} | {'batch, exhaustive rows ms':>25s} {'batch, work handle ms':>21s} {'single call ms':>14s} {'single again':>12s}")
    for n in (300, 700, 2000, 5000, 10000, 16384, 20000, 30000, 50000):
        p, w, _ = cloud(n, 17)

        def brute():
            return ctx.rift_descriptors_batch([p], [w])[0]

        def single():
            loop_ix.set_input(p)
            return loop_ix.rift_descriptors(w)

        ref = single()
        t = {}
        for label, limit in (("brute", 1 << 30), ("work", 0)):
            ctx.set_option(capi.OPT_RIFT_BATCH_BRUTE_MAX, limit)
            assert same(brute(), ref), f"{n} points, {label} route differs from the single call"
        t = {"brute": 0.0, "work": 0.0}
        s = [0.0, 0.0]
        for rep in range(2):
            for label, limit in (("brute", 1 << 30), ("work", 0)):
                ctx.set_option(capi.OPT_RIFT_BATCH_BRUTE_MAX, limit)
                t[label] += window(brute, args.window) / 2
            s[rep] = window(single, args.window)
        ctx.set_option(capi.OPT_RIFT_BATCH_BRUTE_MAX, default)
        print(f"{n:7d} {len(ref[1]):7d} | {t['brute']:25.3f} {t['work']:21.3f} {s[0]:14.3f} {s[1]:12.3f}", flush=True)
loop_ix.close()
ctx.close()
