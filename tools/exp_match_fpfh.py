"""dev helper: pcc_match_fpfh_batch (matchFPFH on 33 bins, reference src/comparator.cpp:877-910) per comparison, from host and
from device memory, beside the nearest call the library had before it.  For each workload (the recorded pair tables of
tests/golden/match_workloads.json and 300 drawn pairs) with 33-wide synthetic descriptors, in ONE process on one handle, the
variants interleaved round after round:
  fpfh-host    pcc_match_fpfh_batch on NumPy arrays (the records packed on the host, one upload)
  fpfh-dev     pcc_match_fpfh_batch on CUDA tensors (the records packed on the device)
  d2h+host     the CUDA tensors copied to the host, then fpfh-host (which uploads them again): the path without PCC_MEM_DEVICE
  dims32       pcc_match_knn_batch_dims with dim = 32 and out_d2 on the first 32 bins of the same arrays
Each figure is the MEDIAN of --rounds windows of at least --window seconds, with the smallest and the largest window beside it.
Host clock around calls that end in a synchronise; every shape warmed up.  Before anything is timed, the rows of the pairs
whose distance matrix fits a quick NumPy pass are checked against the float32 running sum in index order, and fpfh-dev
against fpfh-host on every pair.  ns/dist = time per distance pair (references x queries summed over the pairs).
cpu: NumPy brute force in matrix form on one BLAS thread, one pass (no bit parity claimed); workloads of more than 2e9 distance
pairs are left out.
usage: exp_match_fpfh.py [--workload results|cuarto2|drawn300] [--family fpfh-like|quantised] [--window S] [--rounds N] [--no-cpu]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import match_dims_util as mdu
import match_fpfh_util as mfu
from pointcloudcomparator_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--workload", action="append")
ap.add_argument("--family", action="append")
ap.add_argument("--window", type=float, default=0.2)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--no-cpu", action="store_true")
ap.add_argument("--only", action="append", help="run only these variants, e.g. under a profiler")
args = ap.parse_args()

recorded = json.load(open(os.path.join(ROOT, "tests", "golden", "match_workloads.json")))["workloads"]


def drawn(n_pairs=300, seed=20250117):
    counts = sorted({n for w in recorded.values() for n in w["descriptor_counts"]})
    rng = np.random.default_rng(seed)
    return [(p, p, int(counts[a]), int(counts[b])) for p, (a, b) in enumerate(rng.integers(0, len(counts), (n_pairs, 2)))]


def fpfh_pairs(sizes, family, seed):
    """[(des1, des2)] of (n, 33) float32 for sizes = [(cluster1, cluster2, n1, n2)]: one des1 array per distinct cluster1"""
    firsts, pairs = {}, []
    for p, (c1, _c2, n1, n2) in enumerate(sizes):
        if c1 not in firsts:
            firsts[c1] = mfu.fpfh_cloud(n1, family, seed * 100003 + 2 * c1)
        pairs.append((firsts[c1], mfu.fpfh_queries(firsts[c1], n2, family, seed * 100003 + 2 * p + 1)))
    return pairs


def window(fn, seconds):
    fn()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n * 1e6


ix = capi.Index(np.zeros((4, 3), np.float32))
ix.set_tie_order(capi.TIES_LOWEST_INDEX)
med = lambda v: f"{np.median(v):10.1f} [{min(v):9.1f} {max(v):9.1f}]"
print("us per call: median [min max] of %d windows of >= %.2f s" % (args.rounds, args.window))
for name in args.workload or ["results", "cuarto2", "drawn300"]:
    sizes = drawn() if name == "drawn300" else recorded[name]["pairs"]
    n_dist = sum(s[2] * s[3] for s in sizes)
    for family in args.family or mfu.FAMILIES:
        pairs = fpfh_pairs(sizes, family, seed=7)
        thr = np.float32(0.25 if family == "fpfh-like" else 0.004)
        dev = {}
        for a, b in pairs:
            for x in (a, b):
                if id(x) not in dev:
                    dev[id(x)] = torch.from_numpy(x).cuda()
        dpairs = [(dev[id(a)], dev[id(b)]) for a, b in pairs]
        pairs32 = [(a[:, :32], b[:, :32]) for a, b in pairs]       # (views: stride 132, 128 bytes read of each record)
        torch.cuda.synchronize()

        def d2h_host():
            back = {k: t.cpu().numpy() for k, t in dev.items()}
            return ix.match_fpfh_batch([(back[id(a)], back[id(b)]) for a, b in pairs], threshold=thr, return_d2=True)

        variants = {"fpfh-host": lambda: ix.match_fpfh_batch(pairs, threshold=thr, return_d2=True),
                    "fpfh-dev": lambda: ix.match_fpfh_batch(dpairs, threshold=thr, return_d2=True),
                    "d2h+host": d2h_host,
                    "dims32": lambda: ix.match_knn_batch(pairs32, threshold=thr, dim=32, return_d2=True)}
        if args.only:
            variants = {k: v for k, v in variants.items() if k in args.only}
        # the checks (the largest pairs are left to the tests: their distance matrices do not fit a quick NumPy pass)
        if "fpfh-host" in variants:
            rows, d2 = variants["fpfh-host"]()
            kept = sum(len(r) - 1 for r in rows)
            for p, (a, b) in enumerate(pairs):
                if len(a) * len(b) <= 4_000_000:
                    w_row, w_d2, _ = mdu.restate(a, b, 33, thr)
                    assert np.array_equal(rows[p], w_row) and np.array_equal(d2[p].view(np.uint32), w_d2.view(np.uint32)), (name, family, p)
            if "fpfh-dev" in variants:
                drows, dd2 = variants["fpfh-dev"]()
                assert all(np.array_equal(r, s) for r, s in zip(rows, drows)), f"{name} {family}: device rows differ from host rows"
                assert all(np.array_equal(r.view(np.uint32), s.view(np.uint32)) for r, s in zip(d2, dd2))
            print(f"{name:9s} {family:9s} checked: {kept} of {sum(s[3] for s in sizes)} queries kept at threshold {thr}", flush=True)
        t = {k: [] for k in variants}
        for _ in range(args.rounds):  # interleaved: one window of every variant per round
            for k, fn in variants.items():
                t[k].append(window(fn, args.window))
        for k in variants:
            print(f"{name:9s} {family:9s} {k:9s} pairs {len(pairs):4d} dist {n_dist:9.3g} | {med(t[k])} us | {np.median(t[k]) * 1e3 / n_dist:8.4f} ns/dist", flush=True)
        if not args.no_cpu and family == (args.family or mfu.FAMILIES)[0] and n_dist <= 2e9:
            from threadpoolctl import threadpool_limits
            with threadpool_limits(limits=1):
                t0 = time.perf_counter()
                for a, b in pairs:
                    aa = (a * a).sum(1)[None, :]
                    for q0 in range(0, len(b), 2048):   # (blocks of queries: the matrix of the largest pair is 2.5 GB)
                        bb = b[q0:q0 + 2048]
                        ((bb * bb).sum(1)[:, None] - 2 * (bb @ a.T) + aa).argmin(1)
                t_cpu = time.perf_counter() - t0
            print(f"{name:9s} {family:9s} cpu       NumPy brute force, one BLAS thread, one pass {t_cpu * 1e6:12.1f} us | {t_cpu * 1e9 / n_dist:8.4f} ns/dist", flush=True)
ix.close()
