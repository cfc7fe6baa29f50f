"""dev helper: pcc_match_knn_batch against the loop it replaces, per comparison (all gated pairs of one cluster-matching loop,
reference src/comparator.cpp:1296-1365).  For each workload, descriptor family and tie order, in ONE process, alternating:
  batch   one pcc_match_knn_batch for all pairs
  loop    set_input + match_knn per pair on one re-pointed handle (what pcc::matchRIFTFeaturesKnn does), timed twice: the
          difference between its two columns is the run-to-run spread the other differences have to beat
  cpu     oracle.match_rift_knn per pair (the CPU kd-tree)
Every row of the batch is checked against the oracle (FLANN order) or the loop (lowest index) before anything is timed.
Host clock around calls that end in a synchronise; every shape warmed up; each figure from a window of at least 0.2 s.
usage: exp_match_batch.py [--workload results|cuarto2|drawn300] [--family uniform|quantised] [--window SECONDS]

With --dim N (repeatable) the table is another one: pcc_match_knn_batch_dims at every N against pcc_match_knn_batch, lowest-index
ties, per workload and family, in ONE process on one handle, the variants interleaved round after round:
  batch3   pcc_match_knn_batch (three bins, the entry the parent commit has)
  dims3    pcc_match_knn_batch_dims with dim = 3 and out_d2 (the same search through the new entry)
  dimsN    pcc_match_knn_batch_dims with dim = N and out_d2
Each figure is the MEDIAN of --rounds windows, with the smallest and the largest window beside it (the spread).  Every row
is checked before anything is timed: dim 3 against the old entry, dim N against the float32 running sum in NumPy.  The
kernel's VALU operations are counted as (3 * dim + 3) per distance pair.  CPU figures (--cpu): scipy's cKDTree in N
dimensions, one thread, looped per pair, and NumPy brute force (float32 matrix form, no bit parity claimed)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import oracle
from pointcloudcomparator_amd import capi, synth

ap = argparse.ArgumentParser()
ap.add_argument("--workload", action="append")
ap.add_argument("--family", action="append")
ap.add_argument("--window", type=float, default=0.2)
ap.add_argument("--no-cpu", action="store_true", help="leave the CPU loop out (profiling runs)")
ap.add_argument("--dim", action="append", type=int, help="time pcc_match_knn_batch_dims at this dimension (repeatable)")
ap.add_argument("--rounds", type=int, default=5, help="with --dim: windows per variant")
ap.add_argument("--cpu", action="store_true", help="with --dim: also the CPU figures")
ap.add_argument("--only", action="append", help="with --dim: run only these variants (batch3, dims3, dimsN), e.g. under a profiler")
args = ap.parse_args()

recorded = json.load(open(os.path.join(ROOT, "tests", "golden", "match_workloads.json")))["workloads"]


def drawn(n_pairs=300, seed=20250117):
    counts = sorted({n for w in recorded.values() for n in w["descriptor_counts"]})
    rng = np.random.default_rng(seed)
    return [(p, p, int(counts[a]), int(counts[b])) for p, (a, b) in enumerate(rng.integers(0, len(counts), (n_pairs, 2)))]


CALLS = {}  # how often each timed function ran, warm-ups and checks included (read beside a kernel trace)


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


def chain_rows(a, b, dim, thr=np.float32(0.05)):
    """the float32 running sum over `dim` bins in index order; the lowest index among the nearest"""
    t = b[:, None, 0] - a[None, :, 0]
    d = t * t
    for k in range(1, dim):
        t = b[:, None, k] - a[None, :, k]
        d = d + t * t
    best, arg = d.min(1), d.argmin(1)
    keep = best < thr
    return np.concatenate([[0], arg[keep]]).astype(np.int32), np.concatenate([[0], best[keep]]).astype(np.float32)


def dims_table():
    ix = capi.Index(np.zeros((4, 32), np.float32), auto_sync=False)
    ix.set_tie_order(capi.TIES_LOWEST_INDEX)
    med = lambda v: f"{np.median(v):9.1f} [{min(v):8.1f} {max(v):8.1f}]"
    print("us per call: median [min max] of %d windows of >= %.2f s; VALU ops = (3 dim + 3) per distance pair" % (args.rounds, args.window))
    for name in args.workload or ["results", "cuarto2", "drawn300"]:
        sizes = drawn() if name == "drawn300" else recorded[name]["pairs"]
        n_dist = sum(s[2] * s[3] for s in sizes)
        for family in args.family or synth.DESCRIPTOR_FAMILIES:
            pairs = synth.descriptor_pairs(sizes, family, seed=7)
            variants = {"batch3": lambda: ix.match_knn_batch(pairs),
                        "dims3": lambda: ix.match_knn_batch(pairs, dim=3, return_d2=True)}
            for dim in args.dim:
                variants[f"dims{dim}"] = (lambda dim: lambda: ix.match_knn_batch(pairs, dim=dim, return_d2=True))(dim)
            if args.only:
                variants = {k: v for k, v in variants.items() if k in args.only}
            # the checks (the largest pairs are left to the tests: their distance matrices do not fit a quick NumPy pass)
            if "batch3" in variants and "dims3" in variants:
                old, (new, _d2) = variants["batch3"](), variants["dims3"]()
                assert all(np.array_equal(o, n) for o, n in zip(old, new)), f"{name} {family}: dim 3 differs from pcc_match_knn_batch"
            for dim in args.dim:
                if f"dims{dim}" not in variants:
                    continue
                rows, d2 = variants[f"dims{dim}"]()
                for p, (a, b) in enumerate(pairs):
                    if len(a) * len(b) <= 4_000_000:
                        w_row, w_d2 = chain_rows(a, b, dim)
                        assert np.array_equal(rows[p], w_row) and np.array_equal(d2[p].view(np.uint32), w_d2.view(np.uint32)), (name, family, dim, p)
            t = {k: [] for k in variants}
            for _ in range(args.rounds):  # interleaved: one window of every variant per round
                for k, fn in variants.items():
                    t[k].append(window(fn, args.window))
            for k in variants:
                dim = 3 if k in ("batch3", "dims3") else int(k[4:])
                print(f"{name:9s} {family:9s} {k:7s} pairs {len(pairs):4d} dist {n_dist:9.3g} valu-ops {(3 * dim + 3) * n_dist:9.3g} | {med(t[k])}", flush=True)
            if args.cpu:
                from scipy.spatial import cKDTree
                for dim in args.dim:
                    def tree():
                        return [cKDTree(a[:, :dim]).query(b[:, :dim], k=1, workers=1) for a, b in pairs]

                    def brute():
                        out = []
                        for a, b in pairs:
                            x, y = a[:, :dim], b[:, :dim]
                            for q0 in range(0, len(y), 2048):   # (blocks of queries: the matrix of the largest pair is 2.5 GB)
                                yy = y[q0:q0 + 2048]
                                out.append(((yy * yy).sum(1)[:, None] - 2 * (yy @ x.T) + (x * x).sum(1)[None, :]).argmin(1))
                        return out
                    t0 = time.perf_counter(); tree(); t_tree = time.perf_counter() - t0
                    t0 = time.perf_counter(); brute(); t_brute = time.perf_counter() - t0
                    print(f"{name:9s} {family:9s} cpu dim {dim:2d}: cKDTree (1 thread, per pair) {t_tree * 1e6:11.1f} us, NumPy brute force {t_brute * 1e6:11.1f} us (one pass each)", flush=True)
    ix.close()


if args.dim:
    dims_table()
    sys.exit(0)

ix = capi.Index(np.zeros((4, 32), np.float32), auto_sync=False)
print(f"{'workload':9s} {'family':9s} {'ties':6s} {'pairs':>5s} {'dist pairs':>10s} | {'batch us':>9s} {'loop us':>9s} {'loop again':>10s} {'cpu us':>9s} | tied changed")
for name in args.workload or ["results", "cuarto2", "drawn300"]:
    sizes = drawn() if name == "drawn300" else recorded[name]["pairs"]
    for family in args.family or synth.DESCRIPTOR_FAMILIES:
        pairs = synth.descriptor_pairs(sizes, family, seed=7)
        want = [oracle.match_rift_knn(a, b) for a, b in pairs]
        for ties, label in ((capi.TIES_LOWEST_INDEX, "lowest"), (capi.TIES_FLANN, "flann")):
            ix.set_tie_order(ties)

            def batch():
                key = f"batch calls, {label}, {'with' if ties == capi.TIES_FLANN and family == 'quantised' else 'without'} tied queries"
                CALLS[key] = CALLS.get(key, 0) + 1
                return ix.match_knn_batch(pairs)

            def loop():
                CALLS["single calls (set_input + match_knn)"] = CALLS.get("single calls (set_input + match_knn)", 0) + len(pairs)
                out = []
                for a, b in pairs:
                    ix.set_input(a)
                    out.append(ix.match_knn(b))
                return out

            def cpu():
                return [oracle.match_rift_knn(a, b) for a, b in pairs]

            got = batch()
            st = ix.stats()
            ref = want if ties == capi.TIES_FLANN else loop()
            bad = [p for p in range(len(pairs)) if not np.array_equal(got[p], ref[p])]
            assert not bad, f"{name} {family} {label}: rows {bad[:5]} differ"
            t = [0.0, 0.0, 0.0, 0.0]
            for rep in range(2):  # alternating, two rounds; the figure is the mean of the two windows
                t[0] += window(batch, args.window) / 2
                t[1 + rep] = window(loop, args.window)
                if not args.no_cpu:
                    t[3] += window(cpu, args.window) / 2
            print(f"{name:9s} {family:9s} {label:6s} {len(pairs):5d} {sum(len(a) * len(b) for a, b in pairs):10.3g} | "
                  f"{t[0]:9.1f} {t[1]:9.1f} {t[2]:10.1f} {t[3]:9.1f} | {st[5]} {st[6]}", flush=True)
ix.close()
for k in sorted(CALLS):
    print(f"{k}: {CALLS[k]}")
