"""dev helper: what one pcc_shot_descriptors call costs (reference src/comparator.cpp:941-986, the deterministic part of
processSHOT for one cloud), from host and from device memory, beside the host mirror of the same pipeline on one core
(build/shot_host, exhaustive rows) and beside pcc_fpfh_descriptors on the same handle for scale.  Clouds: synth.rift_cloud at
the density of the test scenes (600 points per 0.12 m cube; ~57 ... 87 entries per 4 cm row).  In ONE process.
Per size, over --reps warm calls (default 25):
  host / device   median [min .. max] host clock around the call, ms (it ends in a synchronise; with host arrays the
                  descriptors, 1408 bytes a point, come down inside it; the device-memory call is followed by a device
                  synchronise inside the clock)
  lrf, desc       the frame kernel and the descriptor kernel -- the handle's event timing (pcc_index_timing [0] and [1]),
                  averaged over the calls of a second pass with timing on (the events cost a few microseconds each: not part of
                  the call figures)
  fpfh            pcc_fpfh_descriptors on the same handle, host arrays, median ms
Results are compared bit for bit with the host mirror before anything is timed.
usage: exp_shot.py [--only N] [--reps R] [--no-host]"""
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
import torch
import shot_util
from pointcloudcomparator_amd import capi, synth

ap = argparse.ArgumentParser()
ap.add_argument("--only", type=int, action="append")
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--no-host", action="store_true", help="leave the one-core host mirror out (nothing is checked)")
args = ap.parse_args()
if not args.no_host:
    subprocess.check_call(["make", "build/shot_host"], cwd=ROOT, stdout=subprocess.DEVNULL)


def same(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and ((got.view(np.uint32) == want.view(np.uint32)) | nan).all()


def spread(ms):
    return f"{np.median(ms):8.3f} [{min(ms):7.3f} .. {max(ms):7.3f}]"


tmp = tempfile.mkdtemp()
print(f"{'points':>7s} {'kept':>6s} {'NaN':>5s} {'row 4cm':>7s} | {'host 1 core ms':>14s} | {'host memory: call ms':>30s} | {'device memory: call ms':>30s} | "
      f"{'lrf us':>8s} {'desc us':>8s} | {'fpfh ms':>8s}")
for n in args.only or [300, 3000, 20000]:
    p, _ = synth.rift_cloud(n, 17, extent=0.12 * (n / 600.0) ** (1.0 / 3.0))
    host_ms, want = float("nan"), None
    if not args.no_host:
        d, r, i, out = shot_util.run_host(p, tmp, tag=f"n{n}")
        want, host_ms = (d, r, i), float(out.split("ms=")[1])
    sample = p[:: max(1, n // 500)]
    d2 = ((sample[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    rows4 = np.median((d2 < 0.04 ** 2).sum(1))
    calls = {"host": [], "device": [], "fpfh": []}
    with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
        for _ in range(3):  # check + warm-up
            d, r, i = ix.shot_descriptors()
            ix.fpfh_descriptors()
        if want is not None:
            assert np.array_equal(i, want[2]) and same(d, want[0]) and same(r, want[1]), n
        for _ in range(args.reps):
            t0 = time.perf_counter()
            d, r, i = ix.shot_descriptors()
            calls["host"].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            ix.fpfh_descriptors()
            calls["fpfh"].append((time.perf_counter() - t0) * 1e3)
        ix.enable_timing(2)  # the per-kernel split, timing on
        for _ in range(min(args.reps, 20)):
            ix.shot_descriptors()
        ms = ix.timing()
        kernels = (ms[0] * 1e3, ms[1] * 1e3)
        ix.enable_timing(0)
    with capi.Index(torch.from_numpy(p).cuda(), engine=capi.ENGINE_GRID, device=0) as ix:
        for _ in range(3):
            dd, dr, di = ix.shot_descriptors()
        torch.cuda.synchronize()
        if want is not None:
            assert np.array_equal(di.cpu().numpy(), want[2]) and same(dd.cpu().numpy(), want[0]) and same(dr.cpu().numpy(), want[1]), n
        for _ in range(args.reps):
            t0 = time.perf_counter()
            ix.shot_descriptors()
            torch.cuda.synchronize()
            calls["device"].append((time.perf_counter() - t0) * 1e3)
    print(f"{n:7d} {len(i):6d} {int(np.isnan(d).all(1).sum()):5d} {rows4:7.0f} | {host_ms:14.1f} | {spread(calls['host']):>30s} | {spread(calls['device']):>30s} | "
          f"{kernels[0]:8.1f} {kernels[1]:8.1f} | {np.median(calls['fpfh']):8.3f}", flush=True)
