"""pcc_match_colour_elements without a GPU: the symbol, every refusal that happens before the handle is looked at (a NULL handle
comes last, so no device is needed) in the documented order, the two cases that need no handle at all, the Python wrapper's
argument handling, the host decisions (tests/cpp/test_match_colour_plan.cpp), and the Python restatement of the match loop's
counting against a hand-written table, in the manner of tests/test_cluster_matching_cpu.py."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import match_colours_util as mcu
from match_colours_util import MATCH_COLOURS_REFUSALS, RawMatchColours

ROOT = Path(__file__).resolve().parent.parent


def test_symbol_is_exported():
    from pointcloudcomparator_amd import capi
    assert "pcc_match_colour_elements" in capi.SYMBOLS and hasattr(capi.LIB, "pcc_match_colour_elements")
    assert callable(capi.Index.match_colour_elements)


@pytest.mark.parametrize("kw,status,message", MATCH_COLOURS_REFUSALS)
def test_refused_before_the_handle_is_looked_at(kw, status, message):
    from pointcloudcomparator_amd import capi
    call = RawMatchColours()
    assert call(None, **kw) == status
    assert call.untouched()
    assert message in capi.LIB.pcc_last_error() and b"null index" not in capi.LIB.pcc_last_error()


def test_bad_match_is_refused_with_its_index():
    from pointcloudcomparator_amd import capi
    call = RawMatchColours()
    for bad, i in ((np.array([0, 3], np.int32), 1), (np.array([3, 0], np.int32), 0), (np.array([1, -7], np.int32), 1),
                   (np.array([2 ** 31 - 1, 0], np.int32), 0)):
        assert call(None, matches=bad.ctypes.data) == -1 and call.untouched()
        assert f"matches[{i}] = {int(bad[i])}".encode() in capi.LIB.pcc_last_error()
    # scene 2 without a cluster: every entry but -1 is outside
    one = np.array([0, -1], np.int32)
    assert call(None, matches=one.ctypes.data, n_clusters2=0, offsets2=None, pts2=None, rgb2=None) == -1
    assert b"matches[0] = 0" in capi.LIB.pcc_last_error() and call.untouched()


def test_null_handle_is_refused_last():
    from pointcloudcomparator_amd import capi
    call = RawMatchColours()
    assert call(None) == -1 and call.untouched()
    assert capi.LIB.pcc_last_error() == b"null index"
    # nothing else wrong, other layouts: still the handle
    assert call(None, mem=1) == -1                                            # (device memory is taken)
    assert call(None, stride=12, rgb_stride=4) == -1 and call(None, min_points=0) == -1
    assert call(None, region_nn=129) == -1 and call(None, min_size=1, region_colour=0.0) == -1
    only_first = np.array([0, -1], np.int32)                                   # cluster 1 of scene 2 is not named and may lack records
    empty1, empty2 = np.array([4, 4, 9], np.uintp), np.array([7, 7, 7, 7], np.uintp)
    assert call(None, offsets2=empty2.ctypes.data, pts2=None, rgb2=None) == -1  # (no matched cluster of scene 2 holds a record)
    assert call(None, matches=only_first.ctypes.data, offsets1=empty1.ctypes.data, pts1=None, rgb1=None) == -1
    assert capi.LIB.pcc_last_error() == b"null index" and call.untouched()


def test_no_clusters_and_no_match_are_ok_without_a_handle_or_a_device():
    call = RawMatchColours()
    assert call(None, n_clusters1=0) == 0 and call.untouched()
    assert call(None, n_clusters1=0, offsets1=None, matches=None, elements=None, pts1=None, rgb1=None) == 0
    assert call(None, n_clusters1=0, n_clusters2=0, offsets2=None, pts2=None, rgb2=None) == 0
    # ... but a fault in front of it is still a fault
    assert call(None, n_clusters1=0, mem=9) == -1
    assert call(None, n_clusters1=0, stride=6) == -1
    assert call(None, n_clusters1=0, offsets2=None) == -1
    assert call(None, n_clusters1=0, nn=0) == -5
    assert call.untouched()
    # no entry of matches is >= 0: the table is -1 throughout, in either memory space, with no array of points at all
    for kw in (dict(), dict(mem=1), dict(pts1=None, rgb1=None, pts2=None, rgb2=None), dict(n_clusters2=0, offsets2=None)):
        assert call(None, matches=mcu.NO_MATCH.ctypes.data, **kw) == 0
        assert (call.out["elements"] == -1).all()
    # ... and a fault in front of it is still a fault, and writes nothing
    assert call(None, matches=mcu.NO_MATCH.ctypes.data, rgb_stride=2) == -1 and call.untouched()
    assert call(None, matches=mcu.NO_MATCH.ctypes.data, distance=-1.0) == -1 and call.untouched()


def test_two_faults_resolve_in_the_documented_order():
    from pointcloudcomparator_amd import capi
    call = RawMatchColours()
    err = capi.LIB.pcc_last_error
    dec, huge, bad = mcu.DECREASING.ctypes.data, mcu.HUGE.ctypes.data, mcu.BAD_MATCH_HIGH.ctypes.data
    # 1 the memory space, 2 null arrays, 3 strides and alignment, 4 offsets (decreasing, then the span), 5 matches, 6 parameters, 7 the handle
    assert call(None, mem=7, offsets1=None) == -1 and b"bad mem space" in err()
    assert call(None, elements=None, stride=10) == -1 and b"null argument" in err()
    assert call(None, pts2=None, rgb_stride=2) == -1 and b"null argument" in err()
    assert call(None, stride=10, rgb_stride=2) == -1 and b"stride 10" in err()
    assert call(None, rgb_stride=2, pts1=2) == -1 and b"colour words must be 4-byte aligned, stride 2" in err()
    assert call(None, stride=10, offsets1=dec) == -1 and b"stride 10" in err()
    assert call(None, rgb1=2, offsets1=huge) == -1 and b"4-byte aligned" in err()
    assert call(None, offsets1=dec, offsets2=mcu.HUGE2.ctypes.data) == -1 and b"must not decrease" in err()
    assert call(None, offsets1=huge, offsets2=mcu.DECREASING2.ctypes.data) == -1 and b"must not decrease" in err()
    assert call(None, offsets1=huge, matches=bad) == -5 and b"2^31" in err()
    assert call(None, offsets2=mcu.DECREASING2.ctypes.data, matches=bad) == -1 and b"must not decrease" in err()
    assert call(None, matches=bad, distance=-1.0) == -1 and b"matches[1] = 3" in err()
    assert call(None, matches=bad, nn=0) == -1 and b"matches[1] = 3" in err()
    assert call(None, distance=-1.0, nn=0) == -1 and b"bad threshold" in err()
    assert call(None, nn=0) == -5 and b"neighbours" in err()
    assert call.untouched()


def test_python_wrapper_argument_handling():
    from pointcloudcomparator_amd import capi
    ix = capi.Index.__new__(capi.Index)  # (no handle: the checks below come first)
    ix._h, ix.auto_sync = None, True
    raw = RawMatchColours()
    good = dict(points1=raw.rec1, offsets1=[0, 5, 10], points2=raw.rec2, offsets2=[0, 5, 10, 15], matches=[2, 0])

    def call(**kw):
        return ix.match_colour_elements(**{**good, **kw})

    with pytest.raises(AssertionError):
        call(points1=raw.rec1.astype(np.float64))
    with pytest.raises(AssertionError, match="colour word in column 4"):
        call(points1=np.ascontiguousarray(raw.rec1[:, :3]))
    with pytest.raises(AssertionError, match="one colour per point"):
        call(rgb1=np.zeros((9, 3), np.uint8))
    with pytest.raises(AssertionError, match="same row stride"):
        call(points2=np.ascontiguousarray(raw.rec2[:, :6]))
    with pytest.raises(AssertionError, match="same row stride"):
        call(rgb1=np.zeros((10, 3), np.uint8))                               # (4-byte words on one side, in the records on the other)
    with pytest.raises(AssertionError, match="offsets"):
        call(offsets1=None)
    with pytest.raises(AssertionError, match="beyond"):
        call(offsets2=[0, 5, 10, 16])
    with pytest.raises(AssertionError, match="one match per cluster"):
        call(matches=[2])
    with pytest.raises(capi.PccError) as e:
        call(offsets1=[0, 7, 5])
    assert e.value.status == -1 and "must not decrease" in str(e.value)
    with pytest.raises(capi.PccError) as e:
        call(matches=[0, 3])
    assert e.value.status == -1 and "matches[1] = 3" in str(e.value)
    with pytest.raises(capi.PccError) as e:
        call(region_nn=0)
    assert e.value.status == -5
    separate = dict(points1=np.ascontiguousarray(raw.rec1[:, :4]), rgb1=np.zeros((10, 3), np.uint8), points2=np.ascontiguousarray(raw.rec2[:, :4]),
                    rgb2=np.zeros(15, np.uint32))
    for kw in (dict(), dict(min_size=1, region_colour=0.0), dict(max_size=10), separate):
        with pytest.raises(capi.PccError) as e:  # all arguments good: the NULL handle
            call(**kw)
        assert e.value.status == -1 and "null index" in str(e.value)
    res = call(matches=[-1, -1])                                              # no match: no handle needed
    assert res.shape == (2, 2) and res.dtype == np.int32 and (res == -1).all()
    res = call(points1=raw.rec1[:0], offsets1=[0], matches=[])                # no clusters: the same
    assert res.shape == (0, 2)
    res = call(points2=raw.rec2[:0], offsets2=[0], matches=[-1, -1])          # scene 2 without a cluster
    assert (res == -1).all()
    ix._h = None  # (nothing for __del__ to destroy)


def test_host_decisions():
    exe = ROOT / "build" / "test_match_colour_plan"
    assert exe.exists(), "build/test_match_colour_plan: run `make hosttest`"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_restatement_against_a_hand_written_table():
    """the gate counts finite points and is strict, a cluster is counted once however many rows name it, rows without a match
    are (-1, -1), and the count is the cluster's own: here simply its number of distinct colours"""
    nan = np.nan
    pts = lambda n, bad=0: np.concatenate([np.zeros((n - bad, 3), np.float32), np.full((bad, 3), nan, np.float32)])
    col = lambda n, k: (np.arange(n) % k).astype(np.uint8)[:, None].repeat(3, 1)
    scene1 = [(pts(12), col(12, 3)), (pts(11), col(11, 5)), (pts(10), col(10, 4)), (pts(14, 3), col(14, 2)), (pts(13, 3), col(13, 2)),
              (pts(0), col(0, 1))]
    scene2 = [(pts(20), col(20, 7)), (pts(5), col(5, 2)), (pts(30, 30), col(30, 3))]
    calls = []

    def count_of(p, c):
        calls.append(len(p))
        return len(np.unique(c, axis=0))

    table, distinct, saved = mcu.restate(scene1, scene2, [0, 0, 1, 2, -1, 0], count_of)
    want = [[3, 7],    # 12 points pass the gate; scene 2's cluster 0 is counted here ...
            [5, 7],    # ... and handed on here; 11 points pass
            [0, 0],    # 10 points do not, 5 do not
            [2, 0],    # 14 points, 3 of them NaN: 11 finite pass; 30 NaNs do not
            [-1, -1],  # no match (13 points, 3 of them NaN, would not pass: never looked at)
            [0, 7]]    # an empty cluster; cluster 0 of scene 2 a third time
    assert table.tolist() == want
    assert (distinct, saved) == (8, 2)
    assert calls == [12, 20, 11, 14]                                           # one count per cluster that passed the gate, in first-use order
    table0, _, _ = mcu.restate(scene1, scene2, [0, 0, 1, 2, 2, 0], count_of, min_points=0)
    assert table0.tolist() == [[3, 7], [5, 7], [4, 2], [2, 0], [2, 0], [0, 7]]   # (gate 0: everything with a finite point)


def test_record_layouts():
    rng = np.random.default_rng(1)
    clusters = [mcu.two_level_cloud(rng, n) for n in (3, 0, 5)]
    rec, off = mcu.records(clusters)
    assert rec.shape == (8, 8) and off.tolist() == [0, 3, 3, 8]
    assert (rec[3:, :3] == clusters[2][0]).all() and (rec[:, 3] == 1).all()
    r, g, b = (int(v) for v in clusters[2][1][1])
    assert int(rec[4, 4].view(np.uint32)) == (r << 16 | g << 8 | b)
    p4, w, off2 = mcu.separate(clusters)
    assert p4.shape == (8, 4) and w.dtype == np.uint32 and (w == rec[:, 4].view(np.uint32)).all() and (off2 == off).all()
