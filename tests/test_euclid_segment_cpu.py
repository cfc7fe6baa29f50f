"""pcc_euclidean_cluster_segmentation without a GPU: the symbol, every refusal that happens before the handle is looked at (a NULL
handle comes last, so no device is needed) in the documented order, and the Python wrapper's argument handling, in the manner of
tests/test_segment_cpu.py."""
import numpy as np
import pytest

from euclid_segment_util import EUCLID_REFUSALS, RawEuclid


def test_symbol_is_exported():
    from pointcloudcomparator_amd import capi
    assert "pcc_euclidean_cluster_segmentation" in capi.SYMBOLS and hasattr(capi.LIB, "pcc_euclidean_cluster_segmentation")
    assert callable(capi.Index.euclidean_cluster_segmentation)


@pytest.mark.parametrize("kw,status,message", EUCLID_REFUSALS)
def test_refused_before_the_handle_is_looked_at(kw, status, message):
    from pointcloudcomparator_amd import capi
    call = RawEuclid()
    assert call(None, **kw) == status
    assert call.untouched()
    assert message in capi.LIB.pcc_last_error() and b"null index" not in capi.LIB.pcc_last_error()


def test_null_handle_is_refused_last():
    from pointcloudcomparator_amd import capi
    call = RawEuclid()
    assert call(None) == -1 and call.untouched()
    assert capi.LIB.pcc_last_error() == b"null index"
    # nothing else wrong, optional outputs left out, nothing to do: still the handle
    assert call(None, labels=None, cpoints=None, cindex=None, its=None, ended=None) == -1
    assert call(None, labels=None, cpoints=None, cindex=None, max_clusters=0) == -1  # (no cluster output: no room needed)
    assert call(None, max_planes=0, coeff=None, sizes=None) == -1                    # (no room for planes: no tables needed)
    assert call(None, n=0, pts=None) == -1
    assert call(None, has_rgb=0, stride=12, out_stride=12) == -1
    assert call(None, tol=0.0) == -1 and call(None, stop=0.0) == -1 and call(None, thr=0.0) == -1 and call(None, its_max=0) == -1
    assert capi.LIB.pcc_last_error() == b"null index" and call.untouched()


def test_two_faults_resolve_in_the_documented_order():
    from pointcloudcomparator_amd import capi
    call = RawEuclid()
    err = capi.LIB.pcc_last_error
    # 1 the voxel grid's before 2 the plane loop's before 3 the tolerance before 4 the null counts before 5 the room for clusters
    assert call(None, n=2 ** 31, leaf=0.0) == -5
    assert call(None, leaf=0.0, prob=1.0) == -1 and b"leaf size" in err()
    assert call(None, out_stride=8, stop=-1.0) == -1 and b"bad output stride" in err()
    assert call(None, prob=1.0, stop=-1.0) == -1 and b"bad RANSAC" in err()
    assert call(None, stop=float("nan"), coeff=None) == -1 and b"stop_fraction" in err()
    assert call(None, thr=-1.0, tol=-1.0) == -1 and b"bad RANSAC" in err()
    assert call(None, sizes=None, tol=-1.0) == -1 and b"null output" in err()
    assert call(None, tol=float("nan"), n_filtered=None) == -1 and b"bad tolerance" in err()
    assert call(None, tol=-1.0, max_clusters=0) == -1 and b"bad tolerance" in err()
    assert call(None, n_remaining=None, max_clusters=0) == -1 and b"null output" in err()
    assert call(None, offsets=None, max_clusters=0) == -1 and b"null output" in err()
    assert call.untouched()


def test_python_wrapper_argument_handling():
    from pointcloudcomparator_amd import capi
    ix = capi.Index.__new__(capi.Index)  # (no handle: the checks below come first)
    ix._h, ix.auto_sync = None, True
    pts = np.zeros((8, 8), np.float32)
    with pytest.raises(AssertionError):
        ix.euclidean_cluster_segmentation(pts.astype(np.float64))
    with pytest.raises(AssertionError):
        ix.euclidean_cluster_segmentation(np.zeros((8, 2), np.float32))
    with pytest.raises(AssertionError, match="max_clusters"):
        ix.euclidean_cluster_segmentation(pts, max_clusters=-1)
    with pytest.raises(AssertionError, match="max_planes"):
        ix.euclidean_cluster_segmentation(pts, max_planes=-1)
    with pytest.raises(capi.PccError) as e:
        ix.euclidean_cluster_segmentation(pts, leaf=0.0)
    assert e.value.status == -1 and "leaf size" in str(e.value)
    assert e.value.partial["n_clusters"] == 0 and e.value.partial["n_filtered"] == 0 and len(e.value.partial["points"]) == 0
    with pytest.raises(capi.PccError) as e:
        ix.euclidean_cluster_segmentation(pts, tolerance=-0.5)
    assert e.value.status == -1 and "bad tolerance" in str(e.value)
    with pytest.raises(capi.PccError) as e:
        ix.euclidean_cluster_segmentation(pts, probability=1.0)
    assert e.value.status == -1 and "RANSAC" in str(e.value)
    with pytest.raises(capi.PccError) as e:  # all arguments good: the NULL handle
        ix.euclidean_cluster_segmentation(pts, has_rgb=True, max_planes=0, max_clusters=0)
    assert e.value.status == -1 and "null index" in str(e.value)
    ix._h = None  # (nothing for __del__ to destroy)
