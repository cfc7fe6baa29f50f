"""dev helper: pcc_match_knn_batch against the loop it replaces, per comparison (all gated pairs of one cluster-matching loop,
reference src/comparator.cpp:1296-1365).  For each workload, descriptor family and tie order, in ONE process, alternating:
  batch   one pcc_match_knn_batch for all pairs
  loop    set_input + match_knn per pair on one re-pointed handle (what pcc::matchRIFTFeaturesKnn does), timed twice: the
          difference between its two columns is the run-to-run spread the other differences have to beat
  cpu     oracle.match_rift_knn per pair (the CPU kd-tree)
Every row of the batch is checked against the oracle (FLANN order) or the loop (lowest index) before anything is timed.
Host clock around calls that end in a synchronise; every shape warmed up; each figure from a window of at least 0.2 s.
usage: exp_match_batch.py [--workload results|cuarto2|drawn300] [--family uniform|quantised] [--window SECONDS]"""
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
