"""pcc_vfh_descriptor and pcc_match_vfh on the GPU (reference src/comparator.cpp:482-516 processVHF, :471-480 matchVHF) against
the host mirror of the same arithmetic (build/vfh_host: the headers the kernels are compiled from, exhaustive rows, one core):
the descriptor and the distances carry the mirror's BITS -- same header, same order of operations, votes counted in integers.
What the mirror itself is worth is tests/test_vfh_cpu.py's subject (NumPy restatement in float64).  Also: the wave edges and
the tile edge of the centroid chains, many workgroups merging their counters, a second call on the same handle (the counters
are zeroed again), host and device memory, 12-byte points and 32-byte pcl::PointXYZRGB records, numpy and torch, another
radius, empty and refused clouds on a live handle, FPFH and the normals on the same handle, pcc::processVHF / pcc::matchVHF
through a C++ driver."""
from pathlib import Path

import numpy as np
import pytest

import fpfh_util
import oracle
import vfh_util
from pointcloudcomparator_amd import capi

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
BIT_SCENES = ["volume300", "slab", "isolated", "duplicates", "centroid-hit", "n2", "n63", "n64", "n65", "n511", "n512", "n513", "volume20000"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_same(got, want, what=""):
    got = np.asarray(got)
    assert got.shape == (308,) and got.dtype == np.float32, what
    differ = _bits(got) != _bits(want)
    assert not differ.any(), f"{what}: {int(differ.sum())} of 308 bins differ in their bits, first {int(np.argmax(differ))}: {got[differ][:4]} vs {want[differ][:4]}"


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    """name -> (308,) of build/vfh_host, its own normals, computed once"""
    tmp = tmp_path_factory.mktemp("vfh_host")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = vfh_util.run_host(vfh_util.scene(name), tmp, tag=name.replace("-", "_"))["hist"][0]
        return cache[name]
    return get


@pytest.mark.parametrize("name", BIT_SCENES)
def test_descriptor_carries_the_host_mirrors_bits(gpu, mirror, name):
    p = vfh_util.scene(name)
    want = mirror(name)
    with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
        got = ix.vfh_descriptor()
        _assert_same(got, want, name)
        again = ix.vfh_descriptor()  # the handle's buffers reused, the counters zeroed again
        _assert_same(again, want, f"{name}, second call")
    assert np.isfinite(got).all() and (_bits(got[135:180]) == 0).all()
    assert abs(got[180:].sum(dtype=np.float64) - 100.0) < 1e-2


def test_empty_and_refused_clouds_on_a_live_handle(gpu, mirror):
    p = vfh_util.scene("volume300")
    with capi.Index(p[:1], engine=capi.ENGINE_GRID, device=0) as ix:
        got = ix.vfh_descriptor()
        assert isinstance(got, np.ndarray) and got.shape == (0, 308)
        hist = np.full(308, 7.0, np.float32)
        n_out = capi.C.c_size_t(77)
        assert capi.LIB.pcc_vfh_descriptor(ix._h, capi.MEM_HOST, 0.03, hist.ctypes.data, capi.C.byref(n_out)) == 0
        assert n_out.value == 0 and (hist == 7.0).all()  # zero descriptors, the output untouched
        ix.set_input(p)
        _assert_same(ix.vfh_descriptor(), mirror("volume300"), "after the one-point cloud")
        bad = p.copy()
        bad[17, 1] = np.nan
        ix.set_input(bad)
        with pytest.raises(capi.PccError, match="non-finite") as e:
            ix.vfh_descriptor()
        assert e.value.status == -5
        with pytest.raises(capi.PccError, match="bad radius"):
            ix.vfh_descriptor(normal_radius=0.0)
        ix.set_input(p)
        _assert_same(ix.vfh_descriptor(), mirror("volume300"), "after the refusals")  # and the handle still works


def test_memory_spaces_strides_torch_and_another_radius(gpu, mirror, tmp_path):
    import torch
    p = vfh_util.scene("isolated")
    want = mirror("isolated")
    wide = vfh_util.run_host(p, tmp_path, tag="wide", radius=0.045)["hist"][0]
    assert (_bits(wide) != _bits(want)).any()
    rec = vfh_util.xyzrgb_records(p)  # pcl::PointXYZRGB: 32-byte stride
    with capi.Index(rec, engine=capi.ENGINE_GRID, device=0) as ix:
        h = ix.vfh_descriptor()
        assert isinstance(h, np.ndarray)
        _assert_same(h, want, "numpy records")
        _assert_same(ix.vfh_descriptor(0.045), wide, "numpy records, radius 0.045")
    with capi.Index(torch.from_numpy(p), engine=capi.ENGINE_GRID, device=0) as ix:
        h = ix.vfh_descriptor()
        assert isinstance(h, np.ndarray)
        _assert_same(h, want, "torch host points")
    for name, arr in (("device points", p), ("device records", rec)):
        d = torch.from_numpy(arr).cuda()
        with capi.Index(d, engine=capi.ENGINE_GRID, device=0) as ix:
            h = ix.vfh_descriptor()
            assert h.is_cuda and h.shape == (308,) and h.dtype == torch.float32
            w = ix.vfh_descriptor(0.045)
            torch.cuda.synchronize()
            _assert_same(h.cpu().numpy(), want, name)
            _assert_same(w.cpu().numpy(), wide, f"{name}, radius 0.045")
    with capi.Index(torch.from_numpy(p[:1]).cuda(), engine=capi.ENGINE_GRID, device=0) as ix:
        h = ix.vfh_descriptor()
        assert h.is_cuda and tuple(h.shape) == (0, 308)


def test_fpfh_vfh_and_normals_on_the_same_handle_keep_their_bits(gpu, mirror, tmp_path):
    """the scratch areas are independent: FPFH and VFH alternated on one handle, pcc_normals_radius in between"""
    p = vfh_util.scene("isolated")
    fh, fi = fpfh_util.run_host(p, tmp_path, tag="fpfh")[:2]
    want = mirror("isolated")
    normals = oracle.normals_radius(p, 0.03)
    with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
        for turn in range(2):
            gh, gi = ix.fpfh_descriptors()
            assert np.array_equal(gi, fi) and np.array_equal(_bits(gh), _bits(fh)), f"FPFH, turn {turn}"
            _assert_same(ix.vfh_descriptor(), want, f"VFH, turn {turn}")
            got = ix.normals_radius(0.03)
            assert ((_bits(got) == _bits(normals)) | (np.isnan(got) & np.isnan(normals))).all(), f"normals, turn {turn}"


@pytest.fixture(scope="module")
def descriptors(mirror):
    """130 descriptors: the mirror's of eight scenes, then copies of them with a few bins moved (every row distinct)"""
    base = np.stack([mirror(name) for name in ("volume300", "slab", "isolated", "duplicates", "centroid-hit", "n63", "n511", "n513")])
    rng = np.random.default_rng(53)
    rows = [base[k % len(base)].copy() for k in range(130)]
    for k in range(len(base), 130):
        at = rng.choice(308, 12, replace=False)
        rows[k][at] = (rows[k][at] + rng.uniform(0, 3, 12)).astype(np.float32)
    return np.stack(rows).astype(np.float32)


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (70, 130)])
def test_match_carries_the_host_mirrors_bits(gpu, descriptors, tmp_path, shape):
    import torch
    n1, n2 = shape
    h1, h2 = descriptors[::-1][:n1].copy(), descriptors[:n2].copy()
    want = vfh_util.run_match(h1, h2, tmp_path)
    assert want.shape == shape and np.isfinite(want).all() and (want > 0).sum() >= want.size - min(n1, n2)
    got = capi.match_vfh(h1, h2)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == shape
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), f"host memory: {int((got != want).sum())} of {want.size} distances differ"
    with capi.Index(vfh_util.scene("n63"), engine=capi.ENGINE_GRID, device=0) as ix:
        dev = ix.match_vfh(torch.from_numpy(h1).cuda(), torch.from_numpy(h2).cuda())
        assert dev.is_cuda and dev.dtype == torch.float64 and tuple(dev.shape) == shape
        torch.cuda.synchronize()
        assert np.array_equal(dev.cpu().numpy().view(np.uint64), want.view(np.uint64)), "device memory"
        again = ix.match_vfh(h1, h2)  # the same handle from host memory, its staging reused
        assert np.array_equal(again.view(np.uint64), want.view(np.uint64))


def test_match_nan_rows_and_empty_sides(gpu, descriptors):
    h1, h2 = descriptors[:4].copy(), descriptors[4:9]
    h1[2, 200] = np.nan
    got = capi.match_vfh(h1, h2)
    assert np.isnan(got[2]).all() and np.isfinite(got[[0, 1, 3]]).all()
    assert capi.match_vfh(h1[:0], h2).shape == (0, 5) and capi.match_vfh(h1, h2[:0]).shape == (4, 0)
    assert capi.match_vfh(h1[0], h2[0]).shape == (1, 1)  # single (308,) descriptors


def test_cpp_processVHF_and_matchVHF_equal_the_python_results(gpu, mirror, tmp_path):
    a, b = vfh_util.scene("isolated"), vfh_util.scene("slab")
    for name, p in (("isolated", a), ("slab", b)):
        h, out = vfh_util.run_driver(p, tmp_path, tag=name)
        assert f"vfh_driver n={len(p)} out=1\n" in out
        _assert_same(h[0], mirror(name), f"pcc::processVHF, {name}")
    h, out = vfh_util.run_driver(a[:1], tmp_path, tag="one")
    assert h.shape == (0, 308) and "out=0" in out
    dis = vfh_util.run_driver_match(a, b, tmp_path)
    want = capi.match_vfh(mirror("isolated"), mirror("slab"))
    assert want.shape == (1, 1) and np.float64(dis).view(np.uint64) == want.view(np.uint64)[0, 0] and dis > 0
