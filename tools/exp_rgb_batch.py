"""dev helper: pcc_region_growing_rgb_batch against the loop it replaces, per COMPARISON (color_growing_segmentation of both
clusters of every accepted match, reference src/comparator.cpp:1456-1495, src/segmentation.cpp:161-216).  In ONE process, on one
context handle and one loop handle, alternating:
  batch   one pcc_region_growing_rgb_batch for all clusters
  loop    set_input + region_growing_rgb per cluster on one re-pointed handle (the parent commit's path, unchanged), timed
          twice: the difference between its two columns is the run-to-run spread the other differences have to beat
  host    the one-core host mirror (build/rgb_time, path (a): rows down, PCL's logic on one core), measured on --host-clusters
          clusters spread over the set and scaled to the whole set (one process per cluster: the full set would take minutes)
Clusters are cut from tools/exp_rgb.py's painted room: the n points nearest to a random point of a 300 000-point room.
Workloads: 2 x 30 clusters of 300 points, 2 x 30 of 3000, and 60 clusters drawn from 11 ... 8000 points.
Then the mixed workload, and ONE cloud alone, under PCC_OPT_RGB_BATCH_BRUTE_MAX = 2048 / 4096 / 8192 / 16384: what stands behind
the option's default.  Every slice of the batch is checked against the loop before anything is timed.  Host clock around calls
that end in a synchronise; every shape warmed up; each figure from a window of at least --window seconds.
usage: exp_rgb_batch.py [--window SECONDS] [--host-clusters N] [--no-sweep] [--trace]
  --trace   for a rocprofv3 --kernel-trace --stats run of its own: 10 batch calls over 60 clusters of 3000 points and 10 over 10
            of them, nothing else -- every kernel's dispatch count per call is the same whatever the cluster count (the label
            sweeps aside, which depend on the scene: stats[7] is printed) -- and the waits are stats[7] + 4"""
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
from ply_util import write_ply
from pointcloudcomparator_amd import capi, synth

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, default=0.2)
ap.add_argument("--host-clusters", type=int, default=4)
ap.add_argument("--no-sweep", action="store_true")
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()

BASE = np.array([[180, 170, 150], [90, 60, 40], [40, 90, 160], [200, 40, 40], [60, 160, 80]], np.int32)
rng = np.random.default_rng(20261018)
ROOM = synth.room_cloud(300000, synth.SEED_A)
_which = (np.floor(ROOM[:, 0] * 1.3).astype(int) + np.floor(ROOM[:, 1] * 0.9).astype(int) * 2) % len(BASE)
ROOM_RGB = np.clip(BASE[_which] + np.random.default_rng(8).integers(-2, 3, (len(ROOM), 3)), 0, 255).astype(np.uint8)


def cluster(n):
    """(points, colour words, colours) of the n points of the room nearest to one of its points"""
    centre = ROOM[rng.integers(len(ROOM))]
    d = ((ROOM - centre) ** 2).sum(1)
    take = np.sort(np.argpartition(d, n - 1)[:n])
    p, c = np.ascontiguousarray(ROOM[take]), ROOM_RGB[take]
    return p, synth.pack_rgb(c), c


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
    return all(x[1] == y[1] and np.array_equal(x[0], y[0]) for x, y in zip(a, b)) and len(a) == len(b)


mixed = np.round(np.exp(rng.uniform(np.log(11), np.log(8000), 60))).astype(int)
WORKLOADS = {"2x30x300": [300] * 60, "2x30x3000": [3000] * 60, "mixed60": [int(v) for v in mixed]}

ctx = capi.Index(np.zeros((1, 3), np.float32), engine=capi.ENGINE_BRUTE, device=0)
if args.trace:
    for count in (60, 10):
        clouds = [cluster(3000) for _ in range(count)]
        for _ in range(10):
            ctx.region_growing_rgb_batch([c[0] for c in clouds], [c[1] for c in clouds])
        st = ctx.stats()
        print(f"{count} clusters of 3000 points: {int(st[7])} label sweeps per call, {int(st[7]) + 4} waits, {int(st[0])} segments, {int(st[1])} pairs")
    print("batch calls: 10 over 60 clusters, 10 over 10 clusters")
    ctx.close()
    sys.exit(0)

tool = os.path.join(ROOT, "build", "rgb_time")
if args.host_clusters and not os.path.exists(tool):
    subprocess.check_call(["make", "build/rgb_time"], cwd=ROOT, stdout=subprocess.DEVNULL)
tmp = tempfile.mkdtemp()
loop_ix = capi.Index(cluster(300)[0], engine=capi.ENGINE_GRID, device=0)


def single(p, w):
    loop_ix.set_input(p)
    return loop_ix.region_growing_rgb(w)


def host_ms(clouds):
    """the host mirror's milliseconds for the whole set, from a sample of its clusters scaled by their share of the points"""
    if not args.host_clusters:
        return float("nan")
    pick = sorted(set(np.linspace(0, len(clouds) - 1, args.host_clusters).astype(int).tolist()))
    ms, points = 0.0, 0
    for k in pick:
        ply = os.path.join(tmp, "c.ply")
        write_ply(ply, clouds[k][0], clouds[k][2])
        out = subprocess.run([tool, ply, "3"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and out.stdout.startswith("time "), (out.stdout[-500:], out.stderr[-500:])
        ms += float(out.stdout.split()[2])
        points += len(clouds[k][0])
    return ms * sum(len(c[0]) for c in clouds) / points


print(f"{'workload':9s} {'clusters':>8s} {'points':>7s} {'segments':>8s} {'pairs':>8s} {'sweeps':>6s} | {'batch ms':>9s} {'loop ms':>9s} {'loop again':>10s} "
      f"{'host 1 core ms (scaled)':>23s} | loop / batch")
sets = {}
for name, sizes in WORKLOADS.items():
    clouds = [cluster(n) for n in sizes]
    sets[name] = clouds
    pts, words = [c[0] for c in clouds], [c[1] for c in clouds]

    def batch():
        return ctx.region_growing_rgb_batch(pts, words)

    def loop():
        return [single(p, w) for p, w in zip(pts, words)]

    got, ref = batch(), loop()
    st = ctx.stats()
    assert same(got, ref), f"{name}: the batch differs from the loop"
    assert st[2] == sum(sizes) and st[3] == 0
    t = [0.0, 0.0, 0.0]
    for rep in range(2):  # alternating, two rounds; the batch figure is the mean of its two windows
        t[0] += window(batch, args.window) / 2
        t[1 + rep] = window(loop, args.window)
    print(f"{name:9s} {len(sizes):8d} {sum(sizes):7d} {int(st[0]):8d} {int(st[1]):8d} {int(st[7]):6d} | {t[0]:9.3f} {t[1]:9.3f} {t[2]:10.3f} "
          f"{host_ms(clouds):23.1f} | {min(t[1], t[2]) / t[0]:.2f}", flush=True)

if not args.no_sweep:
    default = ctx.get_option(capi.OPT_RGB_BATCH_BRUTE_MAX)
    limits = (2048, 4096, 8192, 16384)
    clouds = sets["mixed60"]
    pts, words = [c[0] for c in clouds], [c[1] for c in clouds]
    print(f"\nmixed60 under PCC_OPT_RGB_BATCH_BRUTE_MAX (default {default:.0f}): limit, clusters on the work handle, batch ms")
    t = {limit: 0.0 for limit in limits}
    for rep in range(2):
        for limit in limits:
            ctx.set_option(capi.OPT_RGB_BATCH_BRUTE_MAX, limit)
            t[limit] += window(lambda: ctx.region_growing_rgb_batch(pts, words), args.window) / 2
    for limit in limits:
        print(f"{limit:10d} {sum(len(p) > limit for p in pts):3d} {t[limit]:9.3f}", flush=True)
    print(f"\none cloud alone: points | batch kernels ms, batch call through the work handle ms, single calls ms, single again")
    for n in (2048, 4096, 8192, 16384):
        p, w, _ = cluster(n)
        ref = [single(p, w)]
        res = {}
        for label, limit in (("brute", 1 << 30), ("work", 0)):
            ctx.set_option(capi.OPT_RGB_BATCH_BRUTE_MAX, limit)
            assert same(ctx.region_growing_rgb_batch([p], [w]), ref), f"{n} points, {label} route differs from the single call"
        tt = {"brute": 0.0, "work": 0.0}
        s = [0.0, 0.0]
        for rep in range(2):
            for label, limit in (("brute", 1 << 30), ("work", 0)):
                ctx.set_option(capi.OPT_RGB_BATCH_BRUTE_MAX, limit)
                tt[label] += window(lambda: ctx.region_growing_rgb_batch([p], [w]), args.window) / 2
            s[rep] = window(lambda: single(p, w), args.window)
        print(f"{n:7d} | {tt['brute']:9.3f} {tt['work']:9.3f} {s[0]:9.3f} {s[1]:9.3f}", flush=True)
    ctx.set_option(capi.OPT_RGB_BATCH_BRUTE_MAX, default)
loop_ix.close()
ctx.close()
