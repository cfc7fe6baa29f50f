#!/usr/bin/env python3
"""What the reference's spatial_change_detection (src/comparator.cpp:54-110) costs on the device (EXPERIMENTS.md, "Change
detection"): pcc_change_detection at 10^5, 10^6 and 10^7 points per cloud, from host memory and from device memory, with and
without the records; beside it build/changes_host, the same lattice with std::unordered_set on ONE host core
(tools/changes_host.cpp).  Scene: a room scan (synth.room_cloud) and a second scan of the same room in which two pieces of
furniture have been moved.
Warm; per run a host clock around a call that begins and ends with the handle's stream idle; median [min max] of --runs runs.
The device's index list must equal the host core's.  The last column is the least traffic the call needs -- both clouds read
once (12 bytes a point), two random 8-byte table accesses a point, the table cleared once (12 bytes a slot) -- at the 6.3 TB/s a
streaming copy reaches on this chip: a floor the passes are compared with, not a prediction."""
import argparse
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
STREAM_BYTES_PER_S = 6.3e12


def scene(n):
    from pointcloudcomparator_amd import synth
    a = synth.room_cloud(n, synth.SEED_A)
    b = synth.room_cloud(n, synth.SEED_B)
    for (x0, y0, x1, y1, h), shift in zip(synth._ROOM_BOXES[:2], ((0.5, 0.4, 0.0), (-0.3, 0.6, 0.0))):
        on = ((b[:, 0] > x0 - 0.02) & (b[:, 0] < x1 + 0.02) & (b[:, 1] > y0 - 0.02) & (b[:, 1] < y1 + 0.02) & (b[:, 2] > 0.02) &
              (b[:, 2] < h + 0.02))
        b[on] += np.asarray(shift, np.float32)
    return a, np.ascontiguousarray(b)


def table_slots(points):
    s = 64
    while s < 2 * points:
        s *= 2
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="100000,1000000,10000000")
    ap.add_argument("--resolutions", default="0.1,0.02")
    ap.add_argument("--out", default="profiles/changes_exp.txt")
    args = ap.parse_args()
    import torch
    from pointcloudcomparator_amd import capi
    assert capi.device_count() > 0, "no HIP device: nothing is measured without one"
    host_exe = ROOT / "build" / "changes_host"
    if not host_exe.exists():
        subprocess.check_call(["make", "build/changes_host"], cwd=ROOT)
    ctx = capi.Index(np.zeros((1, 3), np.float32))
    cell = lambda v: "%9.3f [%9.3f %9.3f]" % (np.median(v), min(v), max(v))

    def timed(fn):
        out = []
        for run in range(args.warmup + args.runs):
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            if run >= args.warmup:
                out.append((time.perf_counter() - t0) * 1e3)
        return out

    lines = ["change_detection, ms per pair of clouds: median [min max] of %d runs after %d warm-up runs; room scan against the same "
             "room with two pieces of furniture moved, min_points_per_leaf 0" % (args.runs, args.warmup),
             "%-9s %-5s %-6s %9s %9s  %-32s %-32s %12s %8s %9s" % ("points", "res", "memory", "voxels", "reported", "indices", "indices + records",
                                                               "1 host core", "host/dev", "floor ms")]
    for n in [int(s) for s in args.sizes.split(",")]:
        a, b = scene(n)
        for res in [float(s) for s in args.resolutions.split(",")]:
            with tempfile.TemporaryDirectory() as tmp:
                fa, fb, fout = Path(tmp) / "a.f32", Path(tmp) / "b.f32", Path(tmp) / "out.i32"
                a.tofile(fa)
                b.tofile(fb)
                r = subprocess.run([str(host_exe), str(fa), str(fb), str(fout), repr(res), "0"], capture_output=True, text=True, check=True)
                host_idx = np.fromfile(fout, np.int32)
            host_ms = float([l for l in r.stdout.splitlines() if l.startswith("total")][0].split()[1])
            k = np.floor((np.concatenate([a, b]).astype(np.float64) - a[0].astype(np.float64)) / res).astype(np.int64)
            k -= k.min(axis=0)
            voxels = len(np.unique((k[:, 2] << 42) | (k[:, 1] << 21) | k[:, 0]))  # (of a lattice through A's first point: a count, not the cells)
            floor_ms = (12.0 * 2 * n + 16.0 * 2 * n + 12.0 * table_slots(2 * n)) / STREAM_BYTES_PER_S * 1e3
            for memory in ("host", "device"):
                xa, xb = (a, b) if memory == "host" else (torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
                idx = ctx.change_detection(xa, xb, res)
                idx = idx.cpu().numpy() if memory == "device" else idx
                assert np.array_equal(idx, host_idx), (n, res, memory, len(idx), len(host_idx))
                t_idx = timed(lambda: ctx.change_detection(xa, xb, res))
                t_rec = timed(lambda: ctx.change_detection(xa, xb, res, with_records=True))
                lines.append("%-9d %-5g %-6s %9d %9d  %-32s %-32s %12.3f %8.1f %9.4f" % (n, res, memory, voxels, len(idx), cell(t_idx), cell(t_rec),
                                                                                     host_ms, host_ms / np.median(t_idx), floor_ms))
    text = "\n".join(lines) + "\n"
    print(text)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text)


if __name__ == "__main__":
    main()
