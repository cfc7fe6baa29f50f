#!/usr/bin/env python3
"""What the reference's ground_segmentation (src/segmentation.cpp:330-387) costs on the device (EXPERIMENTS.md, "Ground filter"):
pcc_ground_segmentation, pcc_progressive_morphological_filter alone, and the OPEN pass of every window over the points that
window sees, in host memory and in device memory; beside them build/ground_host, the same filter on ONE host core with the same
lattice (tools/ground_host.cpp).  Scenes: the synthetic airborne tile of tests/ground_util.py (about one point per square
metre) at 38 000, 10^5 and 10^6 points, the reference's filter parameters.  The voxel grid's leaf is 1.0 here: the reference's
0.01 asks for more voxels over such a tile than pcc_voxel_grid (or PCL's VoxelGrid) takes.
Warm; per run a host clock around a call that begins and ends with the handle's stream idle; median [min max] of --runs runs.
The device's ground list must equal the host mirror's."""
import argparse
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="38000,100000,1000000")
    ap.add_argument("--leaf", type=float, default=1.0)
    ap.add_argument("--out", default="profiles/ground_exp.txt")
    args = ap.parse_args()
    import torch
    import ground_util as gu
    from pointcloudcomparator_amd import capi
    assert capi.device_count() > 0, "no HIP device: nothing is measured without one"
    host_exe = ROOT / "build" / "ground_host"
    if not host_exe.exists():
        subprocess.check_call(["make", "build/ground_host"], cwd=ROOT)
    P = gu.REFERENCE
    windows, thresholds = capi.pmf_windows(**P)
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

    lines = ["ground_segmentation, ms per cloud: median [min max] of %d runs after %d warm-up runs; filter parameters of the reference "
             "(windows %s, thresholds %s), voxel leaf %g" % (args.runs, args.warmup, windows.tolist(), thresholds.tolist(), args.leaf),
             "%-9s %-6s %8s %8s  %-32s %-32s %12s %8s" % ("points", "memory", "filtered", "ground", "pcc_ground_segmentation", "filter alone",
                                                       "1 host core", "host/dev")]
    split = ["OPEN pass of each window over the points it sees (pcc_morphological_operator), ms, and the host core's whole window:"]
    for n in [int(s) for s in args.sizes.split(",")]:
        pts = gu.airborne_tile(n)
        with tempfile.TemporaryDirectory() as tmp:
            fin, fout = Path(tmp) / "in.f32", Path(tmp) / "out.i32"
            pts.tofile(fin)
            r = subprocess.run([str(host_exe), str(fin), str(fout), str(P["max_window_size"]), str(P["slope"]), str(P["initial_distance"]),
                                str(P["max_distance"]), str(P["cell_size"]), str(P["base"]), "1"], capture_output=True, text=True, check=True)
            host_ground = np.fromfile(fout, np.int32)
        host_lines = [l for l in r.stdout.splitlines() if l.startswith("window")]
        host_ms = float([l for l in r.stdout.splitlines() if l.startswith("total")][0].split()[1])
        host_window_ms = [float(l.split()[-2]) for l in host_lines]
        for memory in ("host", "device"):
            arg = pts if memory == "host" else torch.from_numpy(pts).cuda()
            ground, sizes = ctx.progressive_morphological_filter(arg, **P)
            ground = ground.cpu().numpy() if memory == "device" else ground
            assert np.array_equal(ground, host_ground), (n, memory, len(ground), len(host_ground))
            seg = ctx.ground_segmentation(arg, leaf=args.leaf, **P)
            t_seg = timed(lambda: ctx.ground_segmentation(arg, leaf=args.leaf, **P))
            t_filter = timed(lambda: ctx.progressive_morphological_filter(arg, **P))
            lines.append("%-9d %-6s %8d %8d  %-32s %-32s %12.3f %8.1f" % (n, memory, len(seg["filtered"]), len(seg["ground_index"]), cell(t_seg),
                                                                      cell(t_filter), host_ms, host_ms / np.median(t_filter)))
            # the windows one by one: the survivors of the windows before, then OPEN with this window
            current = np.arange(n)
            row = []
            for k, w in enumerate(windows):
                sub = np.ascontiguousarray(pts[current])
                sub_arg = sub if memory == "host" else torch.from_numpy(sub).cuda()
                t = timed(lambda: ctx.morphological_operator(sub_arg, float(w), capi.MORPH_OPEN))
                row.append("w %g (%d points) %.3f / host %.3f" % (w, len(sub), np.median(t), host_window_ms[k] if k < len(host_window_ms) else 0.0))
                current, _ = ctx.progressive_morphological_filter(pts, **dict(P, max_window_size=int(w)))
            split.append("%-9d %-6s %s" % (n, memory, ";  ".join(row)))
        split += ["%-9d host   %s" % (n, l) for l in host_lines]
    text = "\n".join(lines + split) + "\n"
    print(text)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text)


if __name__ == "__main__":
    main()
