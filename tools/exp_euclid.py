#!/usr/bin/env python3
"""What the reference's -e segmentation path (euclidean_cluster_segmentation, src/segmentation.cpp:64-156) costs per cloud in two
forms (EXPERIMENTS.md), in host memory and in device memory:
  (a) the sequence of calls the one call is specified by, on the same context handle: pcc_voxel_grid, pcc_plane_removal with the
      remaining records, an index over what remains (a second handle re-pointed with set_input, as KdTree::setInputCloud does),
      pcc_euclidean_clusters, pcc_extract_clusters
  (b) pcc_euclidean_cluster_segmentation: one call
Scenes: `rooms` of tests/euclid_segment_util.py (3351 points), and the five-plane room of tools/exp_planes.py at 10^5 and 10^6
points.  Warm; per run a host clock around a form that begins and ends with the handles' streams idle; (a) and (b) interleaved run
by run; median [min max] of --runs runs.  (a) is also split into its stages by host clocks.  Both forms must give the same
counts, and the tool says whether every bit agrees (the voxel centroids of a raw scan are double sums taken in the order the cell
sort left the points in, so two runs of the voxel grid need not agree in the last bit, and what follows inherits that)."""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="profiles/euclid_segment_exp.txt")
    args = ap.parse_args()
    import torch
    from euclid_segment_util import EC, rooms
    from exp_planes import room
    from pointcloudcomparator_amd import capi
    assert capi.device_count() > 0, "no HIP device: nothing is measured without one"

    scenes = [("rooms_3351", rooms()), ("room_100000", room(100000)), ("room_1000000", room(1000000))]
    one = np.zeros((1, 3), np.float32)
    ctx, tree = capi.Index(one), capi.Index(one)
    stages = ("voxel", "planes", "index+clusters", "extract")
    lines = ["-e segmentation path, ms per cloud: median [min max] of %d runs, (a) (b) interleaved, %d warm-up runs each" % (args.runs, args.warmup),
             "(a) pcc_voxel_grid, pcc_plane_removal, set_input + pcc_euclidean_clusters, pcc_extract_clusters   (b) pcc_euclidean_cluster_segmentation",
             "%-13s %-6s %8s %6s %9s %8s  %-26s %-26s %6s  %s" % ("scene", "memory", "filtered", "planes", "remaining", "clusters", "(a) ms", "(b) ms",
                                                              "a / b", "bits")]
    split = []

    def voxel_grid(pts):
        """pcc_voxel_grid in either memory space (Index.voxel_grid takes host arrays only)"""
        if not torch.is_tensor(pts):
            return np.ascontiguousarray(ctx.voxel_grid(pts, 0.025, False))
        out = torch.zeros_like(pts)
        cnt = C.c_size_t(0)
        capi._check(capi.LIB.pcc_voxel_grid(ctx._h, pts.data_ptr(), len(pts), 12, capi.MEM_DEVICE, np.float32(0.025), 0, out.data_ptr(), 12,
                                            C.byref(cnt)))
        return out[:cnt.value]

    for name, host_pts in scenes:
        for memory in ("host", "device"):
            pts = host_pts if memory == "host" else torch.from_numpy(host_pts).cuda()
            clock = {}

            def form_a():
                t = [time.perf_counter()]
                filtered = voxel_grid(pts)
                t.append(time.perf_counter())
                _, _, coeff, sizes, _, _, rem = ctx.plane_removal(filtered, with_points=True)
                t.append(time.perf_counter())
                rem = rem.contiguous() if memory == "device" else np.ascontiguousarray(rem)
                tree.set_input(rem)
                labels, ncl, _ = tree.euclidean_clusters(EC["tolerance"], EC["min_size"], EC["max_size"],
                                                         device_out=rem if memory == "device" else None)
                t.append(time.perf_counter())
                index, offsets, records = ctx.extract_clusters(rem, labels, ncl)
                ctx.sync()
                t.append(time.perf_counter())
                for s, d in zip(stages, np.diff(t)):
                    clock.setdefault(s, []).append(d * 1e3)
                return len(filtered), sizes, rem, labels, ncl, records

            def form_b():
                r = ctx.euclidean_cluster_segmentation(pts)
                return r["n_filtered"], r["plane_sizes"], r["points"], r["labels"], r["n_clusters"], r["cluster_points"]

            a, b = form_a(), form_b()
            ctx.sync(); tree.sync()
            assert a[0] == b[0] and list(a[1]) == list(b[1]) and len(a[2]) == len(b[2]) and a[4] == b[4], (name, a[0], b[0], a[1], b[1], a[4], b[4])
            host = lambda x: np.ascontiguousarray(x.cpu().numpy() if torch.is_tensor(x) else x)
            bits = all(host(x).shape == host(y).shape and (host(x).view(np.uint32) == host(y).view(np.uint32)).all()
                       for x, y in zip((a[2], a[3], a[5]), (b[2], b[3], b[5])))
            times = dict(a=[], b=[])
            for run in range(args.warmup + args.runs):
                if run == args.warmup:
                    clock.clear()
                for k, f in (("a", form_a), ("b", form_b)):
                    ctx.sync(); tree.sync()
                    t0 = time.perf_counter()
                    f()
                    ctx.sync(); tree.sync()
                    if run >= args.warmup:
                        times[k].append((time.perf_counter() - t0) * 1e3)
            cell = lambda v: "%8.3f [%8.3f %8.3f]" % (np.median(v), min(v), max(v))
            lines.append("%-13s %-6s %8d %6d %9d %8d  %-26s %-26s %6.2f  %s" % (
                name, memory, b[0], len(b[1]), len(b[2]), b[4], cell(times["a"]), cell(times["b"]), np.median(times["a"]) / np.median(times["b"]),
                "equal" if bits else "differ"))
            split.append("%-13s %-6s (a) %s;  host copies of the current cloud in (b): %d" % (
                name, memory, ", ".join("%s %.3f" % (s, np.median(clock[s])) for s in stages), ctx.stats()[4]))
    lines.append("stages of (a), ms: medians of host clocks around each stage (the last one ends with the stream idle):")
    text = "\n".join(lines + split) + "\n"
    print(text)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text)


if __name__ == "__main__":
    main()
