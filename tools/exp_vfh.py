"""dev helper: what one pcc_vfh_descriptor call costs (reference src/comparator.cpp:482-516, processVHF for one cloud), beside the
host mirror of the same pipeline on one core (build/vfh_host, exhaustive rows) and beside pcc_fpfh_descriptors on the same
cloud and handle.  Clouds: synth.rift_cloud at the density of the test scenes (600 points per 0.12 m cube; ~30 entries per 3 cm
row).  In ONE process.  Per size, over --reps warm calls (default 25) with host arrays out:
  call     median host clock around the call (it ends in a synchronise; the 308 floats down included)
  cent     k_vfh_centroids (one wave, six serial chains of n links), votes: k_vfh_votes, finish: k_vfh_finish (308 lanes, each up
           to n serial additions) -- the handle's event timing (pcc_index_timing [4], [0] and [1]), averaged over the calls of a
           second pass with timing on (the events cost a few microseconds each: not part of `call`); the rest of a call is the
           radius CSR and the plane fit
  fpfh     median host clock around pcc_fpfh_descriptors (layout 1) on the same handle
The descriptor is compared bit for bit with the host mirror before anything is timed.  Above --host-rows-max points (default
20000) the mirror is given the library's normals instead of fitting its own over exhaustive rows (quadratic: minutes at
250 000); its time is then that of the stages behind the normals alone and is marked with '*'.
usage: exp_vfh.py [--only N] [--reps R] [--no-host] [--host-rows-max M]"""
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
import vfh_util
from pointcloudcomparator_amd import capi, synth

ap = argparse.ArgumentParser()
ap.add_argument("--only", type=int, action="append")
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--no-host", action="store_true", help="leave the one-core host mirror out (nothing is checked)")
ap.add_argument("--host-rows-max", type=int, default=20000)
args = ap.parse_args()
if not args.no_host:
    subprocess.check_call(["make", "build/vfh_host"], cwd=ROOT, stdout=subprocess.DEVNULL)

tmp = tempfile.mkdtemp()
print(f"{'points':>7s} {'row 3cm':>7s} | {'host 1 core ms':>15s} | {'vfh call ms':>11s} {'cent us':>8s} {'votes us':>8s} {'finish us':>9s} | {'fpfh call ms':>12s}")
for n in args.only or [300, 3000, 20000, 250000]:
    p, _ = synth.rift_cloud(n, 17, extent=0.12 * (n / 600.0) ** (1.0 / 3.0))
    sample = p[:: max(1, n // 64)]
    rows3 = np.median((((sample[:, None, :] - p[None, :, :]) ** 2).sum(-1) < 0.03 ** 2).sum(1))
    with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
        host, want = "nan", None
        if not args.no_host:
            given = ix.normals_radius(0.03)[:, :3] if n > args.host_rows_max else None
            r = vfh_util.run_host(p, tmp, tag=f"n{n}", normals=given, timeout=3000)
            want, host = r["hist"][0], f"{float(r['stdout'].split('ms=')[1]):.1f}" + ("*" if given is not None else "")
        for _ in range(3):  # check + warm-up
            h = ix.vfh_descriptor()
            ix.fpfh_descriptors()
        if want is not None:
            assert (h.view(np.uint32) == want.view(np.uint32)).all(), n
        calls, fpfh = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            ix.vfh_descriptor()
            t1 = time.perf_counter()
            ix.fpfh_descriptors()
            calls.append((t1 - t0) * 1e3)
            fpfh.append((time.perf_counter() - t1) * 1e3)
        ix.enable_timing(2)  # the per-kernel split, timing on
        for _ in range(min(args.reps, 20)):
            ix.vfh_descriptor()
        ms = ix.timing()
        ix.enable_timing(0)
    print(f"{n:7d} {rows3:7.0f} | {host:>15s} | {np.median(calls):11.3f} {ms[4] * 1e3:8.1f} {ms[0] * 1e3:8.1f} {ms[1] * 1e3:9.1f} | {np.median(fpfh):12.3f}", flush=True)
