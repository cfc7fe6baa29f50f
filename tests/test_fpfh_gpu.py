"""pcc_fpfh_descriptors on the GPU (reference src/comparator.cpp:824-875, processFPFH) against the host mirror of the same
pipeline (build/fpfh_host: the headers the kernels are compiled from, exhaustive rows, one core): the kept point indices are
equal and every histogram carries the mirror's BITS -- same header, same order of operations, same acosf and atan2f.  What the
mirror itself is worth is tests/test_fpfh_cpu.py's subject (NumPy restatement in float64).  Also: both layouts of the two
kernels, host and device memory, 12-byte points and 32-byte pcl::PointXYZRGB records, numpy and torch; other radii and the
single-CSR path; refusals on a live handle; pcc::processFPFH through a C++ driver; RIFT and the normals on the same handle."""
from pathlib import Path

import numpy as np
import pytest

import fpfh_util
import oracle
import rift_util
from pointcloudcomparator_amd import capi

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_same(got, want, what=""):
    gh, gi = got
    wh, wi = want
    assert np.array_equal(np.asarray(gi), wi), f"{what}: kept point indices differ"
    assert gh.shape == wh.shape == (len(wi), 33)
    differ = (_bits(gh) != _bits(wh)).any(1)
    assert not differ.any(), f"{what}: {int(differ.sum())} of {len(wi)} histograms differ in their bits, first {int(np.argmax(differ))}"


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    """name -> (hist, index) of build/fpfh_host, computed once"""
    tmp = tmp_path_factory.mktemp("fpfh_host")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = fpfh_util.run_host(fpfh_util.scene(name), tmp, tag=name.replace("-", "_"))[:2]
        return cache[name]
    return get


@pytest.mark.parametrize("layout", [1, 0])
@pytest.mark.parametrize("name", list(fpfh_util.SMALL) + list(fpfh_util.BIG))
def test_descriptors_carry_the_host_mirrors_bits(gpu, mirror, name, layout):
    p = fpfh_util.scene(name)
    want = mirror(name)
    assert len(want[1]) > 0
    with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
        ix.set_option(capi.OPT_FPFH_LAYOUT, layout)
        assert ix.get_option(capi.OPT_FPFH_LAYOUT) == layout
        got = ix.fpfh_descriptors()
        _assert_same(got, want, f"{name}, layout {layout}")
        again = ix.fpfh_descriptors()  # the handle's buffers reused
        _assert_same(again, want, f"{name}, layout {layout}, second call")
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32
    assert (np.diff(got[1]) > 0).all()  # ascending original indices
    assert np.isfinite(got[0]).all()


def test_memory_spaces_strides_and_torch(gpu, mirror):
    import torch
    p = fpfh_util.scene("isolated")
    want = mirror("isolated")
    rec = fpfh_util.xyzrgb_records(p)  # pcl::PointXYZRGB: 32-byte stride
    with capi.Index(rec, engine=capi.ENGINE_GRID, device=0) as ix:
        h, i = ix.fpfh_descriptors()
        assert isinstance(h, np.ndarray) and isinstance(i, np.ndarray)
        _assert_same((h, i), want, "numpy records")
    with capi.Index(torch.from_numpy(p), engine=capi.ENGINE_GRID, device=0) as ix:
        h, i = ix.fpfh_descriptors()
        assert isinstance(h, np.ndarray)
        _assert_same((h, i), want, "torch host points")
    for name, arr in (("device points", p), ("device records", rec)):
        d = torch.from_numpy(arr).cuda()
        with capi.Index(d, engine=capi.ENGINE_GRID, device=0) as ix:
            h, i = ix.fpfh_descriptors()
            assert h.is_cuda and i.is_cuda and h.shape == (len(want[1]), 33) and i.shape == (len(want[1]),)
            torch.cuda.synchronize()
            _assert_same((h.cpu().numpy(), i.cpu().numpy()), want, name)


def test_other_radii_and_equal_radii(gpu, tmp_path):
    """(0.025, 0.045): two CSRs at radii of the call's own; (0.04, 0.04): the normals and both FPFH stages share one CSR"""
    p = fpfh_util.scene("volume300")
    for radii in ((0.025, 0.045), (0.04, 0.04)):
        want = fpfh_util.run_host(p, tmp_path, radii=radii)[:2]
        assert len(want[1]) > 250
        with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
            for layout in (1, 0):
                ix.set_option(capi.OPT_FPFH_LAYOUT, layout)
                _assert_same(ix.fpfh_descriptors(*radii), want, f"radii {radii}, layout {layout}")


def test_refusals_on_a_live_handle(gpu, mirror):
    p = fpfh_util.scene("volume300")
    with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
        with pytest.raises(Exception, match=r"only 11 \+ 11 \+ 11 bins"):
            ix.fpfh_descriptors(nr_bins=(11, 11, 10))
        with pytest.raises(Exception, match="bad radius"):
            ix.fpfh_descriptors(fpfh_radius=0.0)
        _assert_same(ix.fpfh_descriptors(), mirror("volume300"), "after the refusals")  # and the handle still works


def test_cpp_processFPFH_equals_the_python_result(gpu, mirror, tmp_path):
    for name in ("isolated", "non-finite"):
        p = fpfh_util.scene(name)
        h, i, out = fpfh_util.run_driver(p, tmp_path, tag=name.replace("-", "_"))
        assert f"Point cloud normals size after removing NaNs: {len(i)}\n" in out
        assert f"Computed {len(i)} FPFH descriptors\n" in out
        with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
            _assert_same(ix.fpfh_descriptors(), (h, i), f"pcc::processFPFH, {name}")
        _assert_same((h, i), mirror(name), f"pcc::processFPFH vs mirror, {name}")


def test_rift_and_normals_on_the_same_handle_keep_their_bits(gpu, mirror, tmp_path):
    """the scratch areas are independent: RIFT and FPFH alternated on one handle, pcc_normals_radius in between"""
    p, rgb = rift_util.scene("isolated")
    rh, ri, _ = rift_util.run_tool(rift_util.HOST, p, rgb, tmp_path)
    want = mirror("isolated")
    normals = oracle.normals_radius(p, 0.03)
    with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
        for turn in range(2):
            gh, gi = ix.rift_descriptors(rgb)
            assert np.array_equal(gi, ri) and np.array_equal(_bits(gh), _bits(rh)), f"RIFT, turn {turn}"
            _assert_same(ix.fpfh_descriptors(), want, f"FPFH, turn {turn}")
            got = ix.normals_radius(0.03)
            assert ((_bits(got) == _bits(normals)) | (np.isnan(got) & np.isnan(normals))).all(), f"normals, turn {turn}"
    assert np.array_equal(want[1], np.nonzero(np.isfinite(normals[:, :3]).all(1))[0])
