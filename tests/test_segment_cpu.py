"""pcc_extract_clusters and pcc_region_growing_segmentation without a GPU: the symbols, and every refusal that happens before the
handle is looked at (a NULL handle comes last, so no device is needed), in the manner of tests/test_plane_removal_cpu.py."""
import numpy as np
import pytest

from segment_util import EXTRACT_REFUSALS, SEGMENT_REFUSALS, RawExtract, RawSegment


def test_symbols_are_exported():
    from pointcloudcomparator_amd import capi
    for name in ("pcc_extract_clusters", "pcc_region_growing_segmentation"):
        assert name in capi.SYMBOLS and hasattr(capi.LIB, name)
    assert callable(capi.Index.extract_clusters) and callable(capi.Index.region_growing_segmentation)


@pytest.mark.parametrize("kw,status,message", EXTRACT_REFUSALS)
def test_extract_refused_before_the_handle_is_looked_at(kw, status, message):
    from pointcloudcomparator_amd import capi
    call = RawExtract()
    assert call(None, **kw) == status
    assert call.untouched()
    assert message in capi.LIB.pcc_last_error() and b"null index" not in capi.LIB.pcc_last_error()


@pytest.mark.parametrize("kw,status,message", SEGMENT_REFUSALS)
def test_segmentation_refused_before_the_handle_is_looked_at(kw, status, message):
    from pointcloudcomparator_amd import capi
    call = RawSegment()
    assert call(None, **kw) == status
    assert call.untouched()
    assert message in capi.LIB.pcc_last_error() and b"null index" not in capi.LIB.pcc_last_error()


def test_extract_null_handle_is_refused_last():
    from pointcloudcomparator_amd import capi
    call = RawExtract()
    assert call(None) == -1 and call.untouched()
    assert capi.LIB.pcc_last_error() == b"null index"
    # nothing else wrong, optional outputs left out, nothing to do: still the handle
    assert call(None, out=None, index=None) == -1
    assert call(None, out=None, records=None, stride=0, record=0, out_stride=0) == -1  # (read only with out_records)
    assert call(None, n=0, records=None, labels=None) == -1
    assert call(None, n_clusters=0) == -1
    assert capi.LIB.pcc_last_error() == b"null index" and call.untouched()
    # two faults: the earlier check wins
    assert call(None, n=2 ** 31, n_clusters=-1) == -5
    assert call(None, n_clusters=-1, offsets=None) == -1 and b"n_clusters" in capi.LIB.pcc_last_error()


def test_segmentation_null_handle_is_refused_last():
    from pointcloudcomparator_amd import capi
    call = RawSegment()
    assert call(None) == -1 and call.untouched()
    assert capi.LIB.pcc_last_error() == b"null index"
    assert call(None, normals=None, labels=None, cpoints=None, cindex=None) == -1
    assert call(None, normals=None, labels=None, cpoints=None, cindex=None, max_clusters=0) == -1  # (no cluster output: no room needed)
    assert call(None, n=0, pts=None) == -1
    assert call(None, has_rgb=0, stride=12, out_stride=12) == -1
    assert capi.LIB.pcc_last_error() == b"null index" and call.untouched()
    # two faults: the earlier check of the documented order wins (the voxel grid's, then the outputs, the thresholds, the counts)
    assert call(None, n=2 ** 31, leaf=0.0) == -5
    assert call(None, leaf=0.0, k=0) == -1
    assert call(None, smooth=float("nan"), k=0) == -1 and b"finite" in capi.LIB.pcc_last_error()
    assert call(None, max_clusters=0, normal_k=0) == -1 and b"max_clusters" in capi.LIB.pcc_last_error()


def test_python_wrapper_argument_handling():
    from pointcloudcomparator_amd import capi
    ix = capi.Index.__new__(capi.Index)  # (no handle: the checks below come first)
    ix._h, ix.auto_sync = None, True
    pts = np.zeros((8, 8), np.float32)
    labels = np.zeros(8, np.int32)
    with pytest.raises(AssertionError):
        ix.extract_clusters(np.zeros((8, 2), np.float32), labels, 1)
    with pytest.raises(AssertionError):
        ix.extract_clusters(pts, np.zeros(7, np.int32), 1)
    with pytest.raises(AssertionError, match="n_clusters"):
        ix.extract_clusters(pts, labels, -1)
    for bad in (8, 10, 36):
        with pytest.raises(AssertionError, match="record_bytes"):
            ix.extract_clusters(pts, labels, 1, record_bytes=bad)
    with pytest.raises(capi.PccError) as e:  # all arguments good: the NULL handle
        ix.extract_clusters(pts, labels, 1, record_bytes=16)
    assert e.value.status == -1 and "null index" in str(e.value)
    with pytest.raises(AssertionError):
        ix.region_growing_segmentation(pts.astype(np.float64))
    with pytest.raises(AssertionError, match="max_clusters"):
        ix.region_growing_segmentation(pts, max_clusters=-1)
    with pytest.raises(capi.PccError) as e:
        ix.region_growing_segmentation(pts, leaf=0.0)
    assert e.value.status == -1 and "leaf size" in str(e.value) and e.value.partial["n_clusters"] == 0
    with pytest.raises(capi.PccError) as e:
        ix.region_growing_segmentation(pts, k=0)
    assert e.value.status == -5
    with pytest.raises(capi.PccError) as e:
        ix.region_growing_segmentation(pts, has_rgb=True)
    assert e.value.status == -1 and "null index" in str(e.value)
    ix._h = None  # (nothing for __del__ to destroy)
