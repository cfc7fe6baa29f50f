"""pcc_shot_descriptors on the GPU (reference src/comparator.cpp:941-986, the deterministic part of processSHOT) against the host
mirror of the same pipeline (build/shot_host: the headers the kernels are compiled from, exhaustive rows, one core): the kept
point indices are equal, and every descriptor and every frame carries the mirror's BITS, with NaN in the same words -- same
headers, same order of operations, same lm_acos and lm_atan2.  What the mirror itself is worth is tests/test_shot_cpu.py's
subject.  Also: host and device memory, 12-byte points and 32-byte pcl::PointXYZRGB records, numpy and torch, out_rf NULL;
other radii (one CSR walked as a prefix, two CSRs, equal radii); refusals on a live handle; pcc::processSHOT through a C++
driver; FPFH, RIFT and SHOT alternated on one handle."""
import numpy as np
import pytest

import fpfh_util
import rift_util
import shot_util
from pointcloudcomparator_amd import capi

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_words(got, want, what):
    """uint32 views where both are finite, isnan masks elsewhere"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, the mirror's {want.shape}"
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN in other words ({int((gn != wn).sum())} words, first row {int(np.argmax((gn != wn).any(1)))})"
    differ = ((_bits(got) != _bits(want)) & ~wn).any(1)
    assert not differ.any(), f"{what}: {int(differ.sum())} of {len(want)} rows differ in their bits, first {int(np.argmax(differ))}"


def _assert_same(got, want, what=""):
    gd, gr, gi = got
    wd, wr, wi = want
    assert np.array_equal(np.asarray(gi), wi), f"{what}: kept point indices differ"
    assert wd.shape == (len(wi), 352) and wr.shape == (len(wi), 9)
    if gr is not None:
        _same_words(gr, wr, what + ", rf")
    _same_words(gd, wd, what + ", descriptors")


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    """name -> (desc, rf, index) of build/shot_host, computed once"""
    tmp = tmp_path_factory.mktemp("shot_host")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = shot_util.run_host(shot_util.scene(name), tmp, tag=name.replace("-", "_"))[:3]
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(shot_util.SMALL) + list(shot_util.BIG))
def test_descriptors_carry_the_host_mirrors_bits(gpu, mirror, name):
    p = shot_util.scene(name)
    want = mirror(name)
    assert len(want[2]) > 0
    with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
        got = ix.shot_descriptors()
        _assert_same(got, want, name)
        again = ix.shot_descriptors()  # the handle's buffers reused
        _assert_same(again, want, f"{name}, second call")
    assert got[0].dtype == np.float32 and got[1].dtype == np.float32 and got[2].dtype == np.int32
    assert (np.diff(got[2]) > 0).all()  # ascending original indices
    finite = np.isfinite(got[0]).all(1)
    assert finite.any() and (np.isnan(got[0][~finite]).all())  # a row is finite or NaN as a whole
    if name in ("isolated", "five-rule"):
        assert (~finite).any()


def test_memory_spaces_strides_torch_and_null_rf(gpu, mirror):
    import torch
    p = shot_util.scene("five-rule")
    want = mirror("five-rule")
    rec = shot_util.xyzrgb_records(p)  # pcl::PointXYZRGB: 32-byte stride
    with capi.Index(rec, engine=capi.ENGINE_GRID, device=0) as ix:
        d, r, i = ix.shot_descriptors()
        assert isinstance(d, np.ndarray) and isinstance(r, np.ndarray) and isinstance(i, np.ndarray)
        _assert_same((d, r, i), want, "numpy records")
        d, r, i = ix.shot_descriptors(with_rf=False)  # out_rf NULL
        assert r is None
        _assert_same((d, r, i), want, "numpy records, no rf")
    with capi.Index(torch.from_numpy(p), engine=capi.ENGINE_GRID, device=0) as ix:
        d, r, i = ix.shot_descriptors()
        assert isinstance(d, np.ndarray)
        _assert_same((d, r, i), want, "torch host points")
    for name, arr in (("device points", p), ("device records", rec)):
        t = torch.from_numpy(arr).cuda()
        with capi.Index(t, engine=capi.ENGINE_GRID, device=0) as ix:
            for with_rf in (True, False):
                d, r, i = ix.shot_descriptors(with_rf=with_rf)
                assert d.is_cuda and i.is_cuda and d.shape == (len(want[2]), 352) and i.shape == (len(want[2]),)
                assert (r is None) if not with_rf else (r.is_cuda and r.shape == (len(want[2]), 9))
                torch.cuda.synchronize()
                _assert_same((d.cpu().numpy(), None if r is None else r.cpu().numpy(), i.cpu().numpy()), want, f"{name}, rf {with_rf}")


def test_other_radii(gpu, tmp_path):
    """(0.05, 0.04): one CSR, the SHOT stages walk a prefix of its rows; (0.03, 0.05): two CSRs; (0.04, 0.04): one CSR, whole rows"""
    p = shot_util.scene("volume300")
    for radii in ((0.05, 0.04), (0.03, 0.05), (0.04, 0.04)):
        want = shot_util.run_host(p, tmp_path, radii=radii)[:3]
        assert len(want[2]) > 250 and np.isfinite(want[0]).all(1).sum() > 250
        with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
            _assert_same(ix.shot_descriptors(*radii), want, f"radii {radii}")


def test_refusals_on_a_live_handle(gpu, mirror):
    p = shot_util.scene("volume300")
    with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
        for kw in (dict(shot_radius=0.0), dict(normal_radius=-1.0), dict(shot_radius=float("nan")), dict(normal_radius=float("inf"))):
            with pytest.raises(Exception, match="bad radius"):
                ix.shot_descriptors(**kw)
        _assert_same(ix.shot_descriptors(), mirror("volume300"), "after the refusals")  # and the handle still works


def test_cpp_processSHOT_equals_the_python_result(gpu, mirror, tmp_path):
    for name in ("isolated", "non-finite"):
        p = shot_util.scene(name)
        d, r, i, out = shot_util.run_driver(p, tmp_path, tag=name.replace("-", "_"))
        assert f"Point cloud normals size after removing NaNs: {len(i)}\n" in out
        with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
            _assert_same(ix.shot_descriptors(), (d, r, i), f"pcc::processSHOT, {name}")
        _assert_same((d, r, i), mirror(name), f"pcc::processSHOT vs mirror, {name}")


def test_cpp_processSHOT_falls_back_to_one_all_zero_descriptor(gpu, tmp_path):
    """four scattered points: no normal, an empty result, and the reference's fallback (:977-985)"""
    p = np.array([[0.1, 0.1, 0.1], [1.1, 0.2, 0.3], [0.4, 1.5, 0.2], [0.3, 0.2, 1.7]], np.float32)
    d, r, i, out = shot_util.run_driver(p, tmp_path, tag="four")
    assert "Point cloud normals size after removing NaNs: 0\n" in out
    assert d.shape == (1, 352) and r.shape == (1, 9) and list(i) == [-1]
    assert (_bits(d) == 0).all() and (_bits(r) == 0).all()
    with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
        assert [len(a) for a in ix.shot_descriptors()] == [0, 0, 0]


def test_fpfh_rift_and_shot_on_the_same_handle_keep_their_bits(gpu, mirror, tmp_path):
    """the scratch areas are independent: RIFT, FPFH and SHOT alternated on one handle"""
    p, rgb = rift_util.scene("isolated")
    rh, ri, _ = rift_util.run_tool(rift_util.HOST, p, rgb, tmp_path)
    fh, fi, _ = fpfh_util.run_host(p, tmp_path, tag="fpfh")
    want = mirror("isolated")
    with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
        for turn in range(2):
            gh, gi = ix.rift_descriptors(rgb)
            assert np.array_equal(gi, ri) and np.array_equal(_bits(gh), _bits(rh)), f"RIFT, turn {turn}"
            _assert_same(ix.shot_descriptors(), want, f"SHOT, turn {turn}")
            gh, gi = ix.fpfh_descriptors()
            assert np.array_equal(gi, fi) and np.array_equal(_bits(gh), _bits(fh)), f"FPFH, turn {turn}"
