"""pcc_cluster_matching without a GPU: the symbol, every refusal that happens before the handle is looked at (a NULL handle comes
last, so no device is needed) in the documented order, the Python wrapper's argument handling, the host decisions and tables
(tests/cpp/test_cluster_match_plan.cpp), and the Python restatement of the loop against the recorded runs
(tests/golden/cluster_tables.json, tests/golden/match_workloads.json), in the manner of tests/test_cluster_desc_cpu.py."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import cluster_matching_util as cmu
import match_batch_util as mbu
from cluster_matching_util import CLUSTER_MATCHING_REFUSALS, RawClusterMatching

ROOT = Path(__file__).resolve().parent.parent


def test_symbol_is_exported():
    from pointcloudcomparator_amd import capi
    assert "pcc_cluster_matching" in capi.SYMBOLS and hasattr(capi.LIB, "pcc_cluster_matching")
    assert callable(capi.Index.cluster_matching)


@pytest.mark.parametrize("kw,status,message", CLUSTER_MATCHING_REFUSALS)
def test_refused_before_the_handle_is_looked_at(kw, status, message):
    from pointcloudcomparator_amd import capi
    call = RawClusterMatching()
    assert call(None, **kw) == status
    assert call.untouched()
    assert message in capi.LIB.pcc_last_error() and b"null index" not in capi.LIB.pcc_last_error()


def test_null_handle_is_refused_last():
    from pointcloudcomparator_amd import capi
    call = RawClusterMatching()
    assert call(None) == -1 and call.untouched()
    assert capi.LIB.pcc_last_error() == b"null index"
    # nothing else wrong, other layouts: still the handle
    assert call(None, mem=1) == -1                                            # (device memory is taken)
    assert call(None, dim=1, stride=4) == -1 and call(None, dim=32) == -1
    assert call(None, threshold=float("nan")) == -1 and call(None, threshold=-1.0) == -1  # (no threshold is refused)
    assert call(None, n_clusters2=0, offsets2=None, centroids2=None, points2=None, des2=None) == -1  # (an empty scene 2 needs no arrays)
    empty1, empty2 = np.array([4, 4, 4], np.uintp), np.array([7, 7, 7, 7], np.uintp)
    assert call(None, offsets1=empty1.ctypes.data, des1=None) == -1           # (no cluster holds a record: no array needed)
    assert call(None, offsets2=empty2.ctypes.data, des2=None) == -1
    assert capi.LIB.pcc_last_error() == b"null index" and call.untouched()


def test_no_clusters_is_ok_without_a_handle_or_a_device():
    call = RawClusterMatching()
    assert call(None, n_clusters1=0) == 0 and call.untouched()
    assert call(None, n_clusters1=0, offsets1=None, centroids1=None, points1=None, des1=None, candidates=None, state=None,
                correspondences=None, matches=None) == 0
    # ... but a fault in front of it is still a fault
    assert call(None, n_clusters1=0, dim=0) == -5
    assert call(None, n_clusters1=0, stride=6) == -1
    assert call(None, n_clusters1=0, offsets2=None) == -1
    assert call.untouched()


def test_two_faults_resolve_in_the_documented_order():
    from pointcloudcomparator_amd import capi
    call = RawClusterMatching()
    err = capi.LIB.pcc_last_error
    decreasing, huge = np.array([0, 7, 5], np.uintp), np.array([0, 5, 2 ** 31], np.uintp)
    # 1 the width, 2 the memory space, 3 null arrays, 4 stride and alignment, 5 offsets (decreasing, then the span), 7 the handle
    assert call(None, dim=0, mem=7) == -5 and b"dimensions" in err()
    assert call(None, dim=40, stride=10) == -5 and b"dimensions" in err()
    assert call(None, mem=7, offsets1=None) == -1 and b"bad mem space" in err()
    assert call(None, points2=None, stride=10) == -1 and b"null argument" in err()
    assert call(None, matches=None, offsets1=decreasing.ctypes.data) == -1 and b"null argument" in err()
    assert call(None, stride=10, offsets1=decreasing.ctypes.data) == -1 and b"stride 10" in err()
    assert call(None, des1=2, offsets1=huge.ctypes.data) == -1 and b"4-byte aligned" in err()
    huge2 = np.array([0, 5, 10, 2 ** 31], np.uintp)
    assert call(None, offsets1=decreasing.ctypes.data, offsets2=huge2.ctypes.data) == -1 and b"must not decrease" in err()
    decreasing2 = np.array([0, 5, 3, 15], np.uintp)
    assert call(None, offsets1=huge.ctypes.data, offsets2=decreasing2.ctypes.data) == -1 and b"must not decrease" in err()
    assert call(None, offsets1=huge.ctypes.data) == -5 and b"2^31" in err()
    assert call.untouched()


def test_python_wrapper_argument_handling():
    from pointcloudcomparator_amd import capi
    ix = capi.Index.__new__(capi.Index)  # (no handle: the checks below come first)
    ix._h, ix.auto_sync = None, True
    raw = RawClusterMatching()
    good = dict(des1=raw.des1, offsets1=[0, 5, 10], des2=raw.des2, offsets2=[0, 5, 10, 15], centroids1=raw.centroids1, centroids2=raw.centroids2,
                points1=[100, 100], points2=[150, 120, 100])

    def call(**kw):
        return ix.cluster_matching(**{**good, **kw})

    with pytest.raises(AssertionError, match="float32"):
        call(des1=raw.des1.astype(np.float64))
    with pytest.raises(AssertionError, match="same row stride"):
        call(des2=np.ascontiguousarray(raw.des2[:, :16]))
    with pytest.raises(AssertionError, match="offsets"):
        call(offsets1=None)
    with pytest.raises(AssertionError, match="beyond"):
        call(offsets2=[0, 5, 10, 16])
    with pytest.raises(AssertionError, match="one centroid and one point count"):
        call(points1=[100])
    with pytest.raises(AssertionError, match="one centroid and one point count"):
        call(centroids2=raw.centroids2[:2])
    with pytest.raises(capi.PccError) as e:
        call(offsets1=[0, 7, 5])
    assert e.value.status == -1 and "must not decrease" in str(e.value)
    with pytest.raises(capi.PccError) as e:
        call(dim=33)
    assert e.value.status == -5
    with pytest.raises(capi.PccError) as e:
        call(des1=np.ascontiguousarray(raw.des1[:, :2]), des2=np.ascontiguousarray(raw.des2[:, :2]))
    assert e.value.status == -1 and "stride 8" in str(e.value)
    for kw in (dict(), dict(dim=32), dict(threshold=0.2)):
        with pytest.raises(capi.PccError) as e:  # all arguments good: the NULL handle
            call(**kw)
        assert e.value.status == -1 and "null index" in str(e.value)
    res = call(des1=raw.des1[:0], offsets1=[0], centroids1=np.zeros((0, 3), np.float32), points1=[])  # no clusters: no handle needed
    assert res["candidates"].shape == (0, 3) and res["state"].shape == (0, 3) and res["correspondences"].shape == (0, 3) and len(res["matches"]) == 0
    ix._h = None  # (nothing for __del__ to destroy)


def test_host_decisions_and_tables():
    exe = ROOT / "build" / "test_cluster_match_plan"
    assert exe.exists(), "build/test_cluster_match_plan: run `make hosttest`"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("name,n_pairs", [("results", 7), ("cuarto2", 88)])
def test_restated_gates_are_the_recorded_workloads(name, n_pairs):
    """the pairs the restatement searches on the recorded tables are match_workloads.json's, exactly and in order"""
    o1, o2, c1, c2, p1, p2 = cmu.run_tables(name)
    res = cmu.restate(None, o1, None, o2, c1, c2, p1, p2, counts=False)
    n1, n2 = np.diff(o1), np.diff(o2)
    pairs = [[int(i), int(res["candidates"][i, k]), int(n1[i]), int(n2[res["candidates"][i, k]])]
             for i, k in zip(*np.nonzero(res["state"] == cmu.SEARCHED))]
    assert len(pairs) == n_pairs and pairs == mbu.workloads()[name]["pairs"]
    w = mbu.workloads()[name]
    assert (len(c1), len(c2)) == (w["clusters1"], w["clusters2"])


def test_recorded_matches_are_among_the_candidates():
    """every match the reference recorded is one of the three candidates of its cluster (the size gate is not asserted: four of
    the 55 fail today's gate and stem from an older program version); the other run records none"""
    assert cmu.runs()["results"]["matched"] == []
    matched = cmu.runs()["cuarto2"]["matched"]
    assert len(matched) == 55
    o1, o2, c1, c2, p1, p2 = cmu.run_tables("cuarto2")
    cand = cmu.candidates(c1, c2)
    assert all(j in cand[i] for i, j in matched)


def test_restatement_pins_what_it_has_to():
    """the count is strict in the threshold, skips invalid records on both sides and overflowed distances, and ignores what lies
    beyond dim"""
    a = np.zeros((4, 32), np.float32)
    b = np.zeros((4, 32), np.float32)
    b[:, 0] = 0.5
    assert cmu.count(a, b, 1, 0.25) == 1 and cmu.count(a, b, 1, np.nextafter(np.float32(0.25), np.float32(1))) == 5
    b[1, 0] = np.nan
    b[2, 5] = np.nan
    assert cmu.count(a, b, 1, 1.0) == 4 and cmu.count(a, b, 6, 1.0) == 3
    a[:, 0] = np.inf
    assert cmu.count(a, b, 1, 1.0) == 1
    a[:, 0] = 3e38
    b[:, 0] = -3e38
    assert cmu.count(a, b, 1, np.inf) == 1
