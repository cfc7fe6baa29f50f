"""dev helper: what one pcc_fpfh_descriptors call costs (reference src/comparator.cpp:824-875, processFPFH for one cloud), for
both layouts of its two kernels (PCC_OPT_FPFH_LAYOUT: 1 = a wave per row, 0 = one lane per row), beside the host mirror of the
same pipeline on one core (build/fpfh_host, exhaustive rows).  Clouds: synth.rift_cloud at the density of the test scenes
(600 points per 0.12 m cube; ~30 entries per 3 cm row, ~140 per 5 cm row).  In ONE process, layouts alternating.
Per size and layout, over --reps warm calls (default 25) with host arrays out:
  call    median host clock around the call (it ends in a synchronise; descriptors down included)
  spfh    the SPFH kernel, weight: the weighting kernel -- the handle's event timing (pcc_index_timing [0] and [1]), averaged
          over the calls of a second pass with timing on (the events cost a few microseconds each: not part of `call`)
Results are compared bit for bit with the host mirror before anything is timed.
usage: exp_fpfh.py [--only N] [--reps R] [--no-host]"""
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
import fpfh_util
from pointcloudcomparator_amd import capi, synth

ap = argparse.ArgumentParser()
ap.add_argument("--only", type=int, action="append")
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--no-host", action="store_true", help="leave the one-core host mirror out (nothing is checked)")
args = ap.parse_args()
if not args.no_host:
    subprocess.check_call(["make", "build/fpfh_host"], cwd=ROOT, stdout=subprocess.DEVNULL)

tmp = tempfile.mkdtemp()
print(f"{'points':>7s} {'kept':>6s} {'row 3cm':>7s} {'row 5cm':>7s} | {'host 1 core ms':>14s} | {'layout 1: call ms':>17s} {'spfh us':>8s} {'weight us':>9s} | "
      f"{'layout 0: call ms':>17s} {'spfh us':>8s} {'weight us':>9s}")
for n in args.only or [300, 3000, 20000]:
    p, _ = synth.rift_cloud(n, 17, extent=0.12 * (n / 600.0) ** (1.0 / 3.0))
    host_ms, want = float("nan"), None
    if not args.no_host:
        h, i, out = fpfh_util.run_host(p, tmp, tag=f"n{n}")
        want, host_ms = (h, i), float(out.split("ms=")[1])
    sample = p[:: max(1, n // 500)]
    d2 = ((sample[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    rows3, rows5 = np.median((d2 < 0.03 ** 2).sum(1)), np.median((d2 < 0.05 ** 2).sum(1))
    with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
        calls, kernels = {1: [], 0: []}, {}
        for layout in (1, 0):  # check + warm-up
            ix.set_option(capi.OPT_FPFH_LAYOUT, layout)
            for _ in range(3):
                h, i = ix.fpfh_descriptors()
            if want is not None:
                assert np.array_equal(i, want[1]) and (h.view(np.uint32) == want[0].view(np.uint32)).all(), (n, layout)
        for _ in range(args.reps):
            for layout in (1, 0):
                ix.set_option(capi.OPT_FPFH_LAYOUT, layout)
                t0 = time.perf_counter()
                h, i = ix.fpfh_descriptors()
                calls[layout].append((time.perf_counter() - t0) * 1e3)
        for layout in (1, 0):  # the per-kernel split, timing on
            ix.set_option(capi.OPT_FPFH_LAYOUT, layout)
            ix.enable_timing(2)
            for _ in range(min(args.reps, 20)):
                ix.fpfh_descriptors()
            ms = ix.timing()
            kernels[layout] = (ms[0] * 1e3, ms[1] * 1e3)
            ix.enable_timing(0)
    print(f"{n:7d} {len(i):6d} {rows3:7.0f} {rows5:7.0f} | {host_ms:14.1f} | {np.median(calls[1]):17.3f} {kernels[1][0]:8.1f} {kernels[1][1]:9.1f} | "
          f"{np.median(calls[0]):17.3f} {kernels[0][0]:8.1f} {kernels[0][1]:9.1f}", flush=True)
