"""dev helper: pcc_cluster_matching against the path it replaces, per comparison (the cluster-matching loop, reference
src/comparator.cpp:1296-1366).  For each workload and descriptor family, in ONE process on one handle, the variants interleaved
round after round:
  host     Index.cluster_matching, descriptors in host memory
  device   the same with the descriptors in device memory (torch tensors)
  gates    the same call with every pair gated out by size: candidates, gates and acceptance alone, no device work -- the host
           first pass, in C++
  batch-l  the replaced path's library share: ONE Index.match_knn_batch over the gated pairs and the walk over its rows
           (len of each), PCC_TIES_LOWEST_INDEX
  batch-f  the same under PCC_TIES_FLANN (what pcc::matchRIFTFeaturesKnnBatch sets)
The replaced path per comparison is gates + batch-l or gates + batch-f: its first pass is the same arithmetic as the call's own
(report.hpp), so the `gates` column stands for it.
Workloads: the two recorded runs (tests/golden/cluster_tables.json: 7 and 88 searched pairs) and 300 drawn pairs (sizes from the
recorded descriptor counts, one scene-1 and one scene-2 cluster per pair, every other pair gated out by size).
Every count is checked against len(row) of the batch call before anything is timed.  Host clock around calls that end in a
synchronise; every shape warmed up; each figure the MEDIAN of --rounds windows of at least --window seconds, smallest and
largest beside it.
usage: exp_cluster_matching.py [--workload results|cuarto2|drawn300] [--family uniform|quantised] [--dim N] [--window S] [--rounds R]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import cluster_matching_util as cmu
import match_batch_util as mbu
from pointcloudcomparator_amd import capi, synth

ap = argparse.ArgumentParser()
ap.add_argument("--workload", action="append")
ap.add_argument("--family", action="append")
ap.add_argument("--dim", type=int, default=3)
ap.add_argument("--window", type=float, default=0.2)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()


def window(fn, seconds):
    """microseconds per call of fn over a window of at least `seconds` (fn ends in a synchronise)"""
    fn()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n * 1e6


def drawn_scene(family, n_pairs=300, seed=20250117):
    """(des1, offsets1, des2, offsets2, centroids1, centroids2, points1, points2): pair p is scene-1 cluster p against scene-2
    cluster p, 10 apart on a line; the point counts (100, 300, 900 in turn) gate every other candidate out"""
    counts = sorted({n for w in mbu.workloads().values() for n in w["descriptor_counts"]})
    rng = np.random.default_rng(seed)
    sizes = [(p, p, int(counts[a]), int(counts[b])) for p, (a, b) in enumerate(rng.integers(0, len(counts), (n_pairs, 2)))]
    pairs = synth.descriptor_pairs(sizes, family, seed=7)
    off = lambda parts: np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)
    cent = np.zeros((n_pairs, 3), np.float32)
    cent[:, 0] = np.arange(n_pairs, dtype=np.float32) * 10
    points = np.array([100 * 3 ** (p % 3) for p in range(n_pairs)], np.int64)
    a, b = [x for x, _ in pairs], [y for _, y in pairs]
    return np.ascontiguousarray(np.concatenate(a)), off(a), np.ascontiguousarray(np.concatenate(b)), off(b), cent, cent.copy(), points, points.copy()


ix = capi.Index(np.zeros((4, 32), np.float32), auto_sync=False)
med = lambda v: f"{np.median(v):9.1f} [{min(v):8.1f} {max(v):8.1f}]"
print("us per comparison: median [min max] of %d windows of >= %.2f s; dim %d" % (args.rounds, args.window, args.dim))
for name in args.workload or ["results", "cuarto2", "drawn300"]:
    for family in args.family or synth.DESCRIPTOR_FAMILIES:
        if name == "drawn300":
            des1, o1, des2, o2, c1, c2, p1, p2 = drawn_scene(family)
        else:
            o1, o2, c1, c2, p1, p2 = cmu.run_tables(name)
            des1, des2 = cmu.run_descriptors(name, family)
        t1, t2 = torch.from_numpy(des1).cuda(), torch.from_numpy(des2).cuda()
        torch.cuda.synchronize()
        got = ix.cluster_matching(des1, o1, des2, o2, c1, c2, p1, p2, dim=args.dim)
        searched = list(zip(*np.nonzero(got["state"] == cmu.SEARCHED)))
        cand = got["candidates"]
        pairs = [(des1[o1[i]:o1[i + 1]], des2[o2[cand[i, k]]:o2[cand[i, k] + 1]]) for i, k in searched]
        n_dist = sum(len(a) * len(b) for a, b in pairs)
        never = np.zeros_like(p2)  # (0 / points1 == 0: every pair gated out by size)
        variants = {
            "host": lambda: ix.cluster_matching(des1, o1, des2, o2, c1, c2, p1, p2, dim=args.dim),
            "device": lambda: ix.cluster_matching(t1, o1, t2, o2, c1, c2, p1, p2, dim=args.dim),
            "gates": lambda: ix.cluster_matching(des1, o1, des2, o2, c1, c2, p1, never, dim=args.dim),
            "batch-l": lambda: [len(r) for r in ix.match_knn_batch(pairs, ties=capi.TIES_LOWEST_INDEX, dim=args.dim)],
            "batch-f": lambda: [len(r) for r in ix.match_knn_batch(pairs, ties=capi.TIES_FLANN, dim=args.dim)],
        }
        want = [int(got["correspondences"][i, k]) for i, k in searched]
        assert variants["batch-l"]() == want and variants["batch-f"]() == want, f"{name} {family}: counts differ from the rows' lengths"
        dev = variants["device"]()
        assert all(np.array_equal(dev[key], got[key]) for key in got), f"{name} {family}: device memory differs from host memory"
        assert (variants["gates"]()["state"] != cmu.SEARCHED).all()
        t = {k: [] for k in variants}
        for _ in range(args.rounds):  # interleaved: one window of every variant per round
            for k, fn in variants.items():
                t[k].append(window(fn, args.window))
        for k in variants:
            print(f"{name:9s} {family:9s} {k:8s} pairs {len(pairs):4d} dist {n_dist:9.3g} matches {int((got['matches'] >= 0).sum()):3d} | {med(t[k])}", flush=True)
ix.close()
