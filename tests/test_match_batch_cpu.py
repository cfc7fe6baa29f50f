"""pcc_match_knn_batch without a GPU: the entry point is declared, exported and bound; it refuses bad arguments before it
looks at any device; the replayed workloads in tests/golden/match_workloads.json are what the reference's two recorded
result files give; and the seeded tie-laden descriptors the GPU tests use really contain ties FLANN resolves differently."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import match_batch_util as mbu  # noqa: E402

# a checkout of the project this one was modelled on (PCC_REFERENCE_DIR, or a `reference` directory beside this repository)
REFERENCE = Path(os.environ.get("PCC_REFERENCE_DIR", ROOT.parent / "reference"))
HAVE_REFERENCE = (REFERENCE / "build" / "results.txt").exists() and (REFERENCE / "build" / "cuarto2MLSSmoothing.txt~").exists()


def test_entry_point_is_declared_exported_and_bound():
    from pointcloudcomparator_amd import capi
    header = (ROOT / "include" / "pcc_nn.h").read_text()
    assert re.search(r"\bint\s+pcc_match_knn_batch\s*\(", header)
    assert "src/comparator.cpp:1296-1365" in header          # the header cites the reference lines it replaces
    assert "pcc_match_knn_batch" in capi.SYMBOLS
    fn = capi.LIB.pcc_match_knn_batch
    assert fn.restype is C.c_int and len(fn.argtypes) == 11
    assert callable(capi.match_knn_batch) and callable(capi.Index.match_knn_batch)


def test_argument_validation_needs_no_gpu():
    from pointcloudcomparator_amd import capi
    L = capi.LIB
    a = np.zeros((4, 32), np.float32)
    ptrs, ns = (C.c_void_p * 1)(a.ctypes.data), (C.c_size_t * 1)(4)
    nulls = (C.c_void_p * 1)(None)
    out, off = np.zeros(8, np.int32), np.full(2, 99, np.uintp)
    o, f = out.ctypes.data, off.ctypes.data
    thr = np.float32(0.05)

    def err():
        return L.pcc_last_error()

    # the arguments are checked first, the handle after them: a null handle with good arguments is the last refusal
    assert L.pcc_match_knn_batch(None, 1, ptrs, ns, ptrs, ns, 128, 0, thr, o, f) == -1 and b"null index" in err()
    assert L.pcc_match_knn_batch(None, 0, None, None, None, None, 128, 0, thr, None, f) == -1 and b"null index" in err()
    for bad in ((None, ns, ptrs, ns, o, f), (ptrs, None, ptrs, ns, o, f), (ptrs, ns, None, ns, o, f), (ptrs, ns, ptrs, None, o, f),
                (ptrs, ns, ptrs, ns, None, f), (ptrs, ns, ptrs, ns, o, None)):
        d1, n1, d2, n2, oo, ff = bad
        assert L.pcc_match_knn_batch(None, 1, d1, n1, d2, n2, 128, 0, thr, oo, ff) == -1
        assert b"null" in err() and b"null index" not in err()
    assert L.pcc_match_knn_batch(None, 1, nulls, ns, ptrs, ns, 128, 0, thr, o, f) == -1 and b"null point pointer" in err()
    assert L.pcc_match_knn_batch(None, 1, ptrs, ns, nulls, ns, 128, 0, thr, o, f) == -1 and b"null point pointer" in err()
    for stride in (0, 8, 10, 126):
        assert L.pcc_match_knn_batch(None, 1, ptrs, ns, ptrs, ns, stride, 0, thr, o, f) == -1 and b"stride" in err()
    assert L.pcc_match_knn_batch(None, 1, ptrs, ns, ptrs, ns, 128, capi.MEM_DEVICE, thr, o, f) == -5 and b"PCC_MEM_HOST" in err()
    assert L.pcc_match_knn_batch(None, 1, ptrs, ns, ptrs, ns, 128, 7, thr, o, f) == -1 and b"mem space" in err()
    # totals beyond 2^31 - 1 (nothing is read: the sizes alone decide)
    big = (C.c_size_t * 2)(2 ** 30, 2 ** 30)
    two = (C.c_void_p * 2)(a.ctypes.data, a.ctypes.data + 128)
    small = (C.c_size_t * 2)(4, 3)
    assert L.pcc_match_knn_batch(None, 2, two, big, two, small, 128, 0, thr, o, f) == -5 and b"2^31" in err()
    assert L.pcc_match_knn_batch(None, 2, two, small, two, big, 128, 0, thr, o, f) == -5 and b"2^31" in err()
    assert L.pcc_match_knn_batch(None, 1, ptrs, (C.c_size_t * 1)(2 ** 31), ptrs, ns, 128, 0, thr, o, f) == -5
    assert off.tolist() == [99, 99] and not out.any()         # nothing was written by any refused call


def test_plan_header_alone():
    """tests/cpp/test_match_plan.cpp compiles csrc/match_plan.hpp, the plan match_knn_batch() and the two other descriptor
    searches build their tables with, on its own: the tables frozen in tests/golden/match_plan_tables.txt word for word, the
    3-D plan equal to the frozen dp = 4 tables, 2^31 records or items refused without an allocation"""
    subprocess.check_call(["make", "build/test_match_plan"], cwd=ROOT)
    r = subprocess.run([str(ROOT / "build" / "test_match_plan"), str(ROOT / "tests" / "golden" / "match_plan_tables.txt")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_match_plan: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    csrc = ROOT / "pointcloudcomparator_amd" / "csrc"
    batch = (csrc / "match_batch.hip").read_text()
    assert "match_plan(n_pairs, des1, n1, n2, match_slice_max_3d()" in batch and "stable_sort" not in batch   # no planner of its own
    for user in ("match_dims_plan.hpp", "cluster_match_plan.hpp"):
        assert "stable_sort" not in (csrc / user).read_text()
    mk = (ROOT / "Makefile").read_text()
    assert re.search(r"^hosttest:.*build/test_match_plan\b", mk, flags=re.M)
    assert re.search(r"^asan:.*build/asan/test_match_plan\b", mk, flags=re.M)
    assert re.search(r"^build/asan/test_match_plan:.*\n.*\n\t\$\(CXX\).*\$\(SANFLAGS\)", mk, flags=re.M)
    assert "build/asan/test_match_plan\n" in mk                                                             # ... and asan runs it


def test_committed_workloads_match_the_recorded_runs():
    doc = json.loads(mbu.GOLDEN.read_text())
    assert "printed" in doc["note"].lower() and "six" in doc["note"]    # a replay of the PRINTED centroids
    table = {"results": (74, 65, 7, 1685, 142, 4.0e4), "cuarto2": (102, 105, 88, 102639, 115073, 1.35e9)}
    for name, (c1, c2, n_pairs, sum1, sum2, work) in table.items():
        w = doc["workloads"][name]
        pairs = w["pairs"]
        assert (w["clusters1"], w["clusters2"], len(pairs)) == (c1, c2, n_pairs)
        assert sum(p[2] for p in pairs) == sum1 and sum(p[3] for p in pairs) == sum2
        assert abs(sum(p[2] * p[3] for p in pairs) / work - 1) < 0.01
        for i, j, n1, n2 in pairs:                                       # every recorded pair passes the descriptor gate
            assert n1 > 3 and n2 > 3 and 0 <= i < c1 and 0 <= j < c2
            assert n1 in w["descriptor_counts"] and n2 in w["descriptor_counts"]
        assert len({(p[0], p[1]) for p in pairs}) == n_pairs
        per_cluster = {}
        for p in pairs:
            per_cluster[p[0]] = per_cluster.get(p[0], 0) + 1
        assert max(per_cluster.values()) <= 3                           # at most three candidates per cluster of cloud 1
    c2pairs = doc["workloads"]["cuarto2"]["pairs"]
    assert max(c2pairs, key=lambda p: p[2] * p[3])[2:] == [23528, 26308]
    # 88 calls over 67 distinct clusters of cloud 1 (63 distinct descriptor COUNTS among them)
    assert len({p[0] for p in c2pairs}) == 67 and len({p[2] for p in c2pairs}) == 63


def test_regenerating_the_fixture_gives_the_committed_file():
    if not HAVE_REFERENCE:
        pytest.skip("the reference's result files are not on this machine")
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "gen_match_workloads.py"), str(REFERENCE), "--check"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "tests/golden/match_workloads.json is not what tools/gen_match_workloads.py writes\n" + r.stdout + r.stderr


def test_the_gates_pass_for_every_recorded_pair_when_replayed():
    """the full gate (descriptor counts AND the integer quotient of the point counts) from the reference files, where present"""
    if not HAVE_REFERENCE:
        pytest.skip("the reference's result files are not on this machine")
    sys.path.insert(0, str(ROOT / "tools"))
    import gen_match_workloads as g
    for name, rel in g.FILES.items():
        clusters = g.parse((REFERENCE / rel).read_text(errors="replace"))
        for i, j, n1, n2 in mbu.workloads()[name]["pairs"]:
            assert clusters[1][i][1] == n1 and clusters[2][j][1] == n2 and n1 > 3 and n2 > 3
            assert clusters[2][j][0] // clusters[1][i][0] == 1


def _d2(a, b):
    """the library's arithmetic on the three bins the search reads: d = dx * dx; d += dy * dy; d += dz * dz, all float32"""
    d = b[:, None, :3] - a[None, :, :3]
    d = d * d
    return (d[..., 0] + d[..., 1]) + d[..., 2]


def test_the_quantised_family_has_ties_flann_resolves_differently():
    """before any GPU run: with the seed the GPU tests use, the CPU oracle (FLANN's order) names another reference than the
    lowest index for at least one query of the small recorded workload -- so a GPU test on it exercises the tie walk"""
    import oracle
    from pointcloudcomparator_amd import synth
    pairs = synth.descriptor_pairs(mbu.workloads()["results"]["pairs"], "quantised", seed=7)
    differs = tied = 0
    for a, b in pairs:
        d2 = _d2(a, b)
        assert d2.dtype == np.float32
        lowest, best = d2.argmin(1), d2.min(1)                           # (argmin: the first, i.e. lowest, index)
        tied += int(((d2 == best[:, None]).sum(1) > 1).sum())
        keep = best < np.float32(0.05)
        want = np.concatenate([[0], lowest[keep]]).astype(np.int32)
        got = oracle.match_rift_knn(a, b)
        assert len(got) == len(want)
        assert (d2[np.arange(len(b))[keep], got[1:]] == best[keep]).all()   # the oracle's choice is AT the minimum distance
        differs += int((got != want).sum())
    assert tied > 0 and differs > 0
    # ... and the uniform family has none
    for a, b in synth.descriptor_pairs(mbu.workloads()["results"]["pairs"], "uniform", seed=7):
        d2 = _d2(a, b)
        assert ((d2 == d2.min(1)[:, None]).sum(1) == 1).all()
