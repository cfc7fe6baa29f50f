"""dev helper: what one pcc_sift_keypoints call costs (reference src/comparator.cpp:435-469, processSift for one cluster), for
both layouts of the scale-space kernel (PCC_OPT_SIFT_LAYOUT: 1 = a wave per point, 0 = one lane per (point, scale)), beside the
host mirror of the same detector on one core (build/sift_host, exhaustive rows).  Clouds: synth.rift_cloud at the density of
the test scenes' largest (8 000 points per 0.285 m cube).  In ONE process, layouts alternating.
Per size and layout, over --reps warm calls (default 15) with host arrays in and out:
  call   median host clock around the call (it ends in a synchronise; points and colours up, keypoints down included)
Kernel times come from a trace in a run of its own: rocprofv3 --kernel-trace --stats -- python tools/exp_sift.py --only 8000
--no-host.  Results are compared bit for bit with the host mirror before anything is timed.
usage: exp_sift.py [--only N] [--reps R] [--no-host]"""
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
ap.add_argument("--only", type=int, action="append")
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--no-host", action="store_true", help="leave the one-core host mirror out (profiling runs: nothing is checked)")
args = ap.parse_args()
if not args.no_host:
    subprocess.check_call(["make", "build/sift_host"], cwd=ROOT, stdout=subprocess.DEVNULL)

tmp = tempfile.mkdtemp()
ctx_cloud, _ = synth.rift_cloud(200, 3)
print(f"{'points':>7s} {'keypoints':>9s} {'octave sizes':>28s} {'longest row':>11s} | {'host 1 core ms':>14s} | {'layout 1 call ms':>16s} | {'layout 0 call ms':>16s}")
for n in args.only or [300, 700, 2000, 8000]:
    p, rgb = synth.rift_cloud(n, 17, extent=0.285 * (n / 8000.0) ** (1.0 / 3.0))
    words = synth.pack_rgb(rgb)
    host_ms, want, sizes, longest = float("nan"), None, "", ""
    if not args.no_host:
        h = sift_util.run_host(p, rgb, tmp, tag=f"n{n}")
        want, host_ms, sizes, longest = h["keypoints"], float(h["info"]["ms"]), h["info"]["sizes"], h["info"]["rows_max"]
    with capi.Index(ctx_cloud, engine=capi.ENGINE_GRID, device=0) as ix:
        calls = {1: [], 0: []}
        for layout in (1, 0):  # check + warm-up
            ix.set_option(capi.OPT_SIFT_LAYOUT, layout)
            for _ in range(3):
                k = ix.sift_keypoints(p, words)
            if want is not None:
                assert k.shape == want.shape and (k.view(np.uint32) == want.view(np.uint32)).all(), (n, layout)
        for _ in range(args.reps):
            for layout in (1, 0):
                ix.set_option(capi.OPT_SIFT_LAYOUT, layout)
                t0 = time.perf_counter()
                k = ix.sift_keypoints(p, words)
                calls[layout].append((time.perf_counter() - t0) * 1e3)
    print(f"{n:7d} {len(k):9d} {sizes:>28s} {longest:>11s} | {host_ms:14.1f} | {np.median(calls[1]):16.3f} | {np.median(calls[0]):16.3f}", flush=True)
