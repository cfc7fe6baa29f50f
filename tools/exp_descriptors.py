#!/usr/bin/env python3
"""What the reference's per-cluster descriptor loop (src/comparator.cpp:1224-1290) costs for all clusters of a comparison in two
forms (EXPERIMENTS.md, "Cluster descriptors in one call"), from host memory and from device memory:
  (a) the sequence of calls the one call replaces, on one kept context handle: pcc_sift_keypoints_batch with the snap for the
      clusters above 700 points, the host gather of the snapped clouds (duplicates kept, misses dropped),
      pcc_rift_descriptors_batch over every cluster's cloud, and the centroid loop on the host (float sums in index order).  From
      device memory it begins with the download of the cluster clouds: the two batch calls take host arrays only
  (b) pcc_cluster_descriptors: one call, on the same handle
Workloads: the three of profiles/sift_batch_exp.txt (60 clusters above the gate: 2x30x1000, 2x30x3000, mixed60 of 701 ... 8000
points), each mixed with 60 dense clusters of 50 ... 700 points.  Warm; (a) and (b) alternate run by run in one process, a host
clock around each form, which begins and ends with the stream idle; median [min max] of --runs runs.  Both forms must give the
same bits.  Last: the centroid kernel on one cluster of 250 000 points (the call with and without out_centroids, alternating)."""
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
    ap.add_argument("--out", default="profiles/cluster_descriptors_exp.txt")
    args = ap.parse_args()
    import torch
    import cluster_desc_util as cdu
    from pointcloudcomparator_amd import capi, synth
    assert capi.device_count() > 0, "no HIP device: nothing is measured without one"

    def cloud(n, seed):
        p, rgb = synth.rift_cloud(n, seed, extent=0.12 * (n / 600.0) ** (1.0 / 3.0))
        return cdu.records(p, rgb)

    rng = np.random.default_rng(20261018)
    mixed = np.round(np.exp(rng.uniform(np.log(701), np.log(8000), 60))).astype(int)  # (tools/exp_sift_batch.py's draw)
    dense = np.round(np.exp(np.random.default_rng(20261019).uniform(np.log(50), np.log(700), 60))).astype(int)
    workloads = {"2x30x1000": [1000] * 60, "2x30x3000": [3000] * 60, "mixed60": [int(v) for v in mixed]}
    ctx = capi.Index(np.zeros((1, 3), np.float32), engine=capi.ENGINE_BRUTE, device=0)
    gate = 700
    lines = ["descriptor loop, ms per comparison: median [min max] of %d runs, (a) (b) alternating, %d warm-up runs each" % (args.runs, args.warmup),
             "(a) pcc_sift_keypoints_batch + host gather + pcc_rift_descriptors_batch + host centroids (device: + download)   (b) pcc_cluster_descriptors",
             "%-10s %-6s %8s %7s %9s %8s %11s  %-26s %-26s %6s  %s" % ("workload", "memory", "clusters", "points", "keypoints", "snapped", "descriptors",
                                                                       "(a) ms", "(b) ms", "a / b", "bits")]
    for name, sizes in workloads.items():
        # SIFT-route and dense clusters interleaved, as a segmentation leaves them
        order = [v for pair in zip(sizes, dense) for v in pair]
        clusters = [cloud(int(n), 500 + k) for k, n in enumerate(order)]
        rec = np.ascontiguousarray(np.concatenate(clusters))
        off = np.concatenate([[0], np.cumsum([len(c) for c in clusters])]).astype(np.int64)
        large = [c for c in range(len(clusters)) if len(clusters[c]) > gate]
        for memory in ("host", "device"):
            src = rec if memory == "host" else torch.from_numpy(rec).cuda()

            def form_a():
                h = src if memory == "host" else src.cpu().numpy()  # the download of the cluster clouds
                cl = [h[off[c]:off[c + 1]] for c in range(len(clusters))]
                kp, koff, snap = ctx.sift_keypoints_batch([cl[c] for c in large], snap_radius=0.05)
                clouds, picked = list(cl), {}
                for i, c in enumerate(large):
                    s = snap[koff[i]:koff[i + 1]]
                    picked[c] = s[s >= 0]
                    clouds[c] = np.ascontiguousarray(cl[c][picked[c]])
                des = ctx.rift_descriptors_batch(clouds)
                cent = np.stack([cdu.centroid(c) for c in cl])
                return des, picked, cent, koff

            def form_b():
                return ctx.cluster_descriptors(src, None, off, sift_above=gate)

            a, b = form_a(), form_b()
            ctx.sync()
            bits = np.array_equal(cdu.bits(a[2]), cdu.bits(b["centroids"]))
            for c in range(len(clusters)):
                hist, j = a[0][c]
                lo, hi = int(b["offsets"][c]), int(b["offsets"][c + 1])
                idx = a[1][c][j] if c in a[1] else j
                bits = bits and hi - lo == len(j) and np.array_equal(b["point_index"][lo:hi], idx) and np.array_equal(cdu.bits(hist), cdu.bits(b["histograms"][lo:hi]))
            stats = ctx.stats()
            times = dict(a=[], b=[])
            for run in range(args.warmup + args.runs):
                for k, f in (("a", form_a), ("b", form_b)):
                    ctx.sync()
                    t0 = time.perf_counter()
                    f()
                    ctx.sync()
                    if run >= args.warmup:
                        times[k].append((time.perf_counter() - t0) * 1e3)
            cell = lambda v: "%8.3f [%8.3f %8.3f]" % (np.median(v), min(v), max(v))
            lines.append("%-10s %-6s %8d %7d %9d %8d %11d  %-26s %-26s %6.2f  %s" % (
                name, memory, len(clusters), len(rec), stats[3], stats[4], len(b["point_index"]), cell(times["a"]), cell(times["b"]),
                np.median(times["a"]) / np.median(times["b"]), "equal" if bits else "differ"))
            print(lines[-1], flush=True)

    # ---- the centroid kernel: one dense cluster of 250 000 points, the call with and without out_centroids ----------------------
    n = 250000
    big = cloud(n, 77)
    call = cdu.RawClusterDesc(capacity=n, records=big, offsets=[0, n])
    assert call(ctx._h, sift_above=cdu.SIZE_MAX) == 0
    assert np.array_equal(cdu.bits(call.out["cent"][0]), cdu.bits(cdu.centroid(big)))
    times = dict(with_=[], without=[])
    for run in range(args.warmup + args.runs):
        for k, kw in (("with_", {}), ("without", dict(cent=None))):
            ctx.sync()
            t0 = time.perf_counter()
            assert call(ctx._h, sift_above=cdu.SIZE_MAX, **kw) == 0
            if run >= args.warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    lines.append("one dense cluster of %d points, ms per call: with out_centroids %.3f [%.3f %.3f], without %.3f [%.3f %.3f]: the centroid kernel and "
                 "its copy cost %.3f ms (difference of the medians)" % (n, np.median(times["with_"]), min(times["with_"]), max(times["with_"]),
                                                                       np.median(times["without"]), min(times["without"]), max(times["without"]),
                                                                       np.median(times["with_"]) - np.median(times["without"])))
    text = "\n".join(lines) + "\n"
    print(text)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text)


if __name__ == "__main__":
    main()
