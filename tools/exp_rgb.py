"""dev helper: what color_growing_segmentation costs per cluster (reference src/segmentation.cpp:161-216, called twice per
accepted match) on its two paths, by cluster size.  Clouds: synth.room_cloud painted as the first scene of
tests/test_rgb_gpu.py.  Per size, 3 warm-ups and --reps warm repetitions (default 20), medians of the host clock:
  in this process, on one handle
    rows    Index.knn(pts, 100) to host arrays: the one GPU call of the host path and its n x 100 x 8 bytes coming down
    call    Index.region_growing_rgb(rgb): the new call, host colours in, host labels out
  in build/rgb_time (tools/rgb_time.cpp; the host logic is C++, so the whole host path is timed there), one process per
  size, both paths alternating on one tree, the index build part of both
    (a) host    pcc::RegionGrowingRGB::extract as it stands: the rows call above, then PCL's growing / segment
                neighbours / merging on one core (include/pcc/region_growing_rgb.hpp)
    (b) device  setDeviceSegmentation(true): one pcc_region_growing_rgb call
The two paths' clusters are compared before anything is printed.  Also printed: the bytes either path brings to the host,
grown segments, distinct ordered segment pairs, label sweeps, clusters kept.
usage: exp_rgb.py [--only N] [--reps R]"""
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
ap.add_argument("--only", type=int, action="append")
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()
subprocess.check_call(["make", "build/rgb_time"], cwd=ROOT, stdout=subprocess.DEVNULL)
tool = os.path.join(ROOT, "build", "rgb_time")
tmp = tempfile.mkdtemp()
base = np.array([[180, 170, 150], [90, 60, 40], [40, 90, 160], [200, 40, 40], [60, 160, 80]], np.int32)


def median_ms(fn, reps):
    for _ in range(3):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


print(f"{'points':>7s} | {'rows ms':>8s} {'call ms':>8s} | {'(a) host ms':>11s} {'(b) device ms':>13s} {'a / b':>6s} | {'rows MB':>8s} {'records+pairs KB':>16s} | "
      f"{'segments':>8s} {'pairs':>8s} {'sweeps':>6s} {'clusters':>8s}")
for n in args.only or [300, 3000, 30000, 300000]:
    rng = np.random.default_rng(8)
    room = synth.room_cloud(n, synth.SEED_A)
    which = (np.floor(room[:, 0] * 1.3).astype(int) + np.floor(room[:, 1] * 0.9).astype(int) * 2) % len(base)
    rgb = np.clip(base[which] + rng.integers(-2, 3, (len(room), 3)), 0, 255).astype(np.uint8)
    words = synth.pack_rgb(rgb)
    with capi.Index(room, device=0) as ix:
        rows_ms = median_ms(lambda: ix.knn(room, min(100, len(room))), args.reps)
        call_ms = median_ms(lambda: ix.region_growing_rgb(words), args.reps)
    ply = os.path.join(tmp, f"room{n}.ply")
    write_ply(ply, room, rgb)
    out = subprocess.run([tool, ply, str(args.reps)], capture_output=True, text=True, timeout=1100)
    assert out.returncode == 0 and out.stdout.startswith("time "), (out.stdout[-500:], out.stderr[-500:])
    _, m, host, dev, ns, pairs, sweeps, ncl = out.stdout.split()
    m, host, dev, ns, pairs = int(m), float(host), float(dev), int(ns), int(pairs)
    print(f"{m:7d} | {rows_ms:8.3f} {call_ms:8.3f} | {host:11.3f} {dev:13.3f} {host / dev:6.2f} | {m * 800 / 1e6:8.2f} {(ns * 16 + pairs * 12) / 1e3:16.1f} | "
          f"{ns:8d} {pairs:8d} {sweeps:>6s} {ncl:>8s}", flush=True)
