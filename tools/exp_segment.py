#!/usr/bin/env python3
"""What the reference's default segmentation path (region_growing_segmentation, src/segmentation.cpp:218-327) costs per cloud
in two forms (EXPERIMENTS.md):
  (a) the sequence of calls the pcc:: classes issue: an index over the RAW cloud (VoxelGrid::filter's context handle) +
      pcc_voxel_grid, an index over the filtered cloud with PCC_OPT_KNN_CACHE_K = 100, pcc_normals (50) down to the host,
      pcc_region_growing with those normals uploaded again, the labels walked on the host into one cloud per cluster
  (b) pcc_region_growing_segmentation: one call, host memory in and out
Both on host clouds, one handle per path kept over the runs ((a) re-points its two handles with set_input, as
KdTree::setInputCloud does).  Scenes: the room scan of synth.py at 10^5 and 10^6 raw points, and walls27 (2187 points) of the
tests.  Warm; per run a host clock around a form that begins and ends with the handles' streams idle; (a) and (b) interleaved run by
run; median [min max] of --runs runs, no handle instrumented meanwhile.  (a) is also split into its stages by host clocks.
For (b) a separate pass of --timed-runs calls per scene, bracketed by enable_timing(2) / enable_timing(0) so that the event ring
holds those calls alone, gives pcc_index_timing[2]: the mean stream time from the call's start -- in front of the upload of the raw
cloud -- to the arrival of the cluster offsets, host waits included; what is left of the wall clock is the delivery of the results.
Both forms must give the same counts, and the tool says whether every bit
agrees (the voxel centroids of a raw scan are double sums taken in the order the cell sort left the points in)."""
import argparse
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
    ap.add_argument("--timed-runs", type=int, default=5)
    ap.add_argument("--out", default="profiles/segment_exp.txt")
    args = ap.parse_args()
    from pointcloudcomparator_amd import capi, synth
    from segment_util import RG, walls27
    assert capi.device_count() > 0, "no HIP device: nothing is measured without one"

    scenes = [("walls27_2187", walls27()), ("room_100000", synth.room_cloud(100000, synth.SEED_A)),
              ("room_1000000", synth.room_cloud(1000000, synth.SEED_A))]
    one = np.zeros((1, 3), np.float32)
    raw_ctx, tree, ctx = capi.Index(one), capi.Index(one), capi.Index(one)
    tree.set_option(capi.OPT_KNN_CACHE_K, 100)
    stages = ("voxel", "index+normals", "growing", "clusters")
    lines = ["default segmentation path, ms per cloud: median [min max] of %d runs, (a) (b) interleaved, %d warm-up runs each" % (args.runs, args.warmup),
             "(a) raw index + pcc_voxel_grid, filtered index, pcc_normals, pcc_region_growing, host walk   (b) pcc_region_growing_segmentation",
             "%-14s %8s %8s  %-26s %-26s %6s  %s" % ("scene", "filtered", "clusters", "(a) ms", "(b) ms", "a / b", "bits")]
    split = []

    for name, pts in scenes:
        clock = {}

        def form_a():
            t = [time.perf_counter()]
            raw_ctx.set_input(pts)
            filtered = np.ascontiguousarray(raw_ctx.voxel_grid(pts, 0.025, False))
            t.append(time.perf_counter())
            tree.set_input(filtered)
            normals = tree.normals(50)
            t.append(time.perf_counter())
            labels, ncl = tree.region_growing(normals, 100, **RG)
            t.append(time.perf_counter())
            order = np.argsort(labels, kind="stable")
            order = order[labels[order] >= 0]
            offsets = np.concatenate([[0], np.cumsum(np.bincount(labels[labels >= 0], minlength=ncl))])
            members = filtered[order]
            clusters = [members[offsets[c]:offsets[c + 1]] for c in range(ncl)]
            t.append(time.perf_counter())
            for s, d in zip(stages, np.diff(t)):
                clock.setdefault(s, []).append(d * 1e3)
            return filtered, normals, labels, ncl, members, clusters

        def form_b():
            r = ctx.region_growing_segmentation(pts)
            return r["filtered"], r["normals"], r["labels"], r["n_clusters"], r["cluster_points"], r["offsets"]

        a, b = form_a(), form_b()
        assert len(a[0]) == len(b[0]) and a[3] == b[3], (name, len(a[0]), len(b[0]), a[3], b[3])
        bits = all(x.shape == y.shape and (np.ascontiguousarray(x).view(np.uint32) == np.ascontiguousarray(y).view(np.uint32)).all()
                   for x, y in zip((a[0], a[1], a[2], a[4]), (b[0], b[1], b[2], b[4])))
        times = dict(a=[], b=[])
        clock.clear()
        for run in range(args.warmup + args.runs):
            if run == args.warmup:
                clock.clear()
            for k, f in (("a", form_a), ("b", form_b)):
                for h in (raw_ctx, tree, ctx):
                    h.sync()
                t0 = time.perf_counter()
                f()
                for h in (raw_ctx, tree, ctx):
                    h.sync()
                if run >= args.warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)
        cell = lambda v: "%8.3f [%8.3f %8.3f]" % (np.median(v), min(v), max(v))
        lines.append("%-14s %8d %8d  %-26s %-26s %6.2f  %s" % (name, len(a[0]), a[3], cell(times["a"]), cell(times["b"]),
                                                              np.median(times["a"]) / np.median(times["b"]), "equal" if bits else "differ"))
        # (b) by the handle's own events, in calls of their own: the ring is reset in front, so the mean is over these calls alone
        ctx.enable_timing(2)
        for _ in range(args.timed_runs):
            form_b()
        to_offsets = ctx.timing()[2]
        ctx.enable_timing(0)
        split.append("%-14s (a) %s;  (b) start of the call to the arrival of the offsets %.3f (mean of %d instrumented calls), sweeps %d" % (
            name, ", ".join("%s %.3f" % (s, np.median(clock[s])) for s in stages), to_offsets, args.timed_runs, ctx.stats()[7]))
    lines.append("stages, ms: medians of host clocks around each stage of (a); for (b) pcc_index_timing[2] of its context handle in a pass of its own,")
    lines.append("from in front of the raw cloud's upload to the offsets' arrival (host waits included; the deliveries of the results lie behind it):")
    text = "\n".join(lines + split) + "\n"
    print(text)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text)


if __name__ == "__main__":
    main()
