"""pcc_plane_removal without a GPU: the refusals that happen before the handle is looked at (a NULL handle comes last, so no
device is needed), in the manner of tests/test_cloud_batch_cpu.py, and the argument handling of Index.plane_removal."""
import numpy as np
import pytest

from plane_removal_util import REFUSALS, RawCall


@pytest.mark.parametrize("kw,status", REFUSALS)
def test_refused_before_the_handle_is_looked_at(kw, status):
    from pointcloudcomparator_amd import capi
    call = RawCall()
    assert call(None, **kw) == status
    assert call.untouched()
    assert b"null index" not in capi.LIB.pcc_last_error()


def test_null_handle_is_refused_last():
    from pointcloudcomparator_amd import capi
    call = RawCall()
    assert call(None) == -1 and call.untouched()
    assert capi.LIB.pcc_last_error() == b"null index"
    # nothing else wrong, optional outputs left out, no turn due, n == 0: still the handle
    assert call(None, its=None, ended=None, pop=None, rem=None, points=None) == -1
    assert call(None, stop=1.0, max_planes=0, coeff=None, sizes=None) == -1
    assert call(None, n=0, pts=None, max_planes=0, coeff=None, sizes=None) == -1
    assert call(None, points=None, record=0, out_stride=0) == -1  # (record_bytes is read only with out_points)
    assert capi.LIB.pcc_last_error() == b"null index" and call.untouched()
    # the messages are pcc_sac_plane's where the fault is one it refuses
    assert call(None, stride=10) == -1
    assert capi.LIB.pcc_last_error() == b"stride 10 must be a multiple of 4 and >= 12"
    assert call(None, prob=1.0) == -1
    assert capi.LIB.pcc_last_error() == b"bad RANSAC parameters"
    # two faults: the earlier check of the documented order wins
    assert call(None, n=2 ** 31, stop=-1.0) == -5
    assert call(None, stop=-1.0, n_planes=None) == -1 and b"stop_fraction" in capi.LIB.pcc_last_error()


def test_python_wrapper_argument_handling():
    from pointcloudcomparator_amd import capi
    assert "pcc_plane_removal" in capi.SYMBOLS
    ix = capi.Index.__new__(capi.Index)  # (no handle: the checks below come first)
    ix._h, ix.auto_sync = None, True
    pts = np.zeros((8, 8), np.float32)
    with pytest.raises(AssertionError):
        ix.plane_removal(np.zeros((8, 2), np.float32))
    with pytest.raises(AssertionError):
        ix.plane_removal(pts.astype(np.float64))
    with pytest.raises(AssertionError, match="max_planes"):
        ix.plane_removal(pts, max_planes=-1)
    for bad in (8, 10, 36):
        with pytest.raises(AssertionError, match="record_bytes"):
            ix.plane_removal(pts, with_points=True, record_bytes=bad)
    # a refusal of the library's raises with its status; nothing was found
    with pytest.raises(capi.PccError) as e:
        ix.plane_removal(pts, stop_fraction=-1.0)
    assert e.value.status == -1 and "stop_fraction" in str(e.value) and len(e.value.partial[1]) == 0
    with pytest.raises(capi.PccError) as e:  # all arguments good: the NULL handle
        ix.plane_removal(pts, with_points=True, record_bytes=16)
    assert e.value.status == -1 and "null index" in str(e.value)
    ix._h = None  # (nothing for __del__ to destroy)
