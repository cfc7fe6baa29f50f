"""pcc_sift_keypoints on the GPU (reference src/comparator.cpp:435-469, processSift) against the host mirror of the same
detector (build/sift_host: the header the kernels are compiled from, exhaustive rows, one core): the keypoint list carries the
mirror's BITS (x, y, z, scale) in the mirror's order -- same header, same order of operations, same expf.  What the mirror
itself is worth is tests/test_sift_cpu.py's subject (NumPy restatement in float64).  Also: both scale-space kernel layouts,
host and device memory, packed colours and 32-byte pcl::PointXYZRGB records, numpy and torch; other parameters; the capacity
protocol; the context handle left as it was; pcc::processSift / pcc::processRIFTwithSIFT through a C++ driver; the CLI's
--sift switch."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sift_util
from ply_util import write_ply
from pointcloudcomparator_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "build" / "comparator"
ALL = list(sift_util.SMALL) + list(sift_util.EDGE) + list(sift_util.BIG)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_same(got, want, what=""):
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape, f"{what}: {got.shape[0]} keypoints, the mirror has {want.shape[0]}"
    differ = (_bits(got) != _bits(want)).any(1)
    assert not differ.any(), f"{what}: {int(differ.sum())} of {len(want)} keypoints differ in their bits, first {int(np.argmax(differ))}"


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    """(name, params) -> build/sift_host's result, computed once"""
    tmp = tmp_path_factory.mktemp("sift_host")
    cache = {}

    def get(name, params=sift_util.DEFAULTS):
        key = (name, tuple(params))
        if key not in cache:
            p, rgb = sift_util.scene(name)
            cache[key] = sift_util.run_host(p, rgb, tmp, tag=f"{name.replace('-', '_')}_{len(cache)}", params=params)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def ctx(gpu):
    """a context handle over a cloud that has nothing to do with the scenes"""
    p, _ = synth.rift_cloud(200, 3)
    with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
        yield ix


@pytest.mark.parametrize("layout", [1, 0])
@pytest.mark.parametrize("name", ALL)
def test_keypoints_carry_the_host_mirrors_bits(ctx, mirror, name, layout):
    p, rgb = sift_util.scene(name)
    want = mirror(name)["keypoints"]
    # (tiny24 stops at the gate; in tiny25 every row and every k-NN row is the whole cloud, so all points share their column
    # minima and maxima and none is a keypoint -- with any colouring: what the call must survive there is K = n = 25)
    assert (len(want) > 0) == (name not in ("tiny24", "tiny25"))
    if name in ("tiny24", "tiny25"):
        assert mirror(name)["info"]["octaves"] == ("0" if name == "tiny24" else "1")
    ctx.set_option(capi.OPT_SIFT_LAYOUT, layout)
    try:
        _assert_same(ctx.sift_keypoints(p, rgb), want, f"{name}, layout {layout}")
        _assert_same(ctx.sift_keypoints(p, synth.pack_rgb(rgb)), want, f"{name}, layout {layout}, second call")  # buffers reused
    finally:
        ctx.set_option(capi.OPT_SIFT_LAYOUT, 1)


def test_big_scene_meets_the_input_condition(mirror):
    """sift8000 is there for the rows no small scene has: longer than a wave's 64 entries many times over (more than 1024),
    beside rows below 64"""
    info = mirror("sift8000")["info"]
    assert int(info["rows_max"]) > 1024 and int(info["rows_min"]) < 64
    assert info["stop"] == "count" and int(info["octaves"]) == 5 and int(info["keypoints"]) > 100


def test_memory_spaces_strides_and_torch(ctx, mirror):
    import torch
    p, rgb = sift_util.scene("sift600")
    want = mirror("sift600")["keypoints"]
    rec = synth.xyzrgb_records(p, rgb)  # pcl::PointXYZRGB: 32-byte stride, colour word at offset 16
    _assert_same(ctx.sift_keypoints(rec, rec), want, "numpy records")
    _assert_same(ctx.sift_keypoints(rec, rgb), want, "numpy records, r g b")
    k = ctx.sift_keypoints(torch.from_numpy(rec), torch.from_numpy(rec))
    assert isinstance(k, np.ndarray) or not k.is_cuda
    _assert_same(np.asarray(k), want, "torch host records")
    _assert_same(np.asarray(ctx.sift_keypoints(torch.from_numpy(p), torch.from_numpy(rgb))), want, "torch host points, r g b")
    drec = torch.from_numpy(rec).cuda()
    k = ctx.sift_keypoints(drec, drec)
    assert k.is_cuda and tuple(k.shape) == want.shape
    torch.cuda.synchronize()
    _assert_same(k.cpu().numpy(), want, "device records")
    dp = torch.from_numpy(p).cuda()
    dw = torch.from_numpy(synth.pack_rgb(rgb).view(np.int32)).cuda()
    k = ctx.sift_keypoints(dp, dw)
    torch.cuda.synchronize()
    _assert_same(k.cpu().numpy(), want, "device points, packed words")
    k = ctx.sift_keypoints(dp, torch.from_numpy(rgb).cuda())
    torch.cuda.synchronize()
    _assert_same(k.cpu().numpy(), want, "device points, r g b")


@pytest.mark.parametrize("params", [(0.005, 5, 3, 0.001), (0.005, 2, 5, 0.001), (0.004, 3, 13, 0.0), (0.006, 4, 1, 0.002)])
def test_other_parameters(ctx, mirror, params):
    p, rgb = sift_util.scene("sift600")
    want = mirror("sift600", params)["keypoints"]
    assert len(want) > 0
    for layout in (1, 0):
        ctx.set_option(capi.OPT_SIFT_LAYOUT, layout)
        try:
            _assert_same(ctx.sift_keypoints(p, rgb, *params), want, f"{params}, layout {layout}")
        finally:
            ctx.set_option(capi.OPT_SIFT_LAYOUT, 1)


def test_capacity_one_short_overflows_and_the_handle_still_works(ctx, mirror):
    p, rgb = sift_util.scene("sift300")
    want = mirror("sift300")["keypoints"]
    m = len(want)
    words = synth.pack_rgb(rgb)
    out = np.full((m, 4), -7.0, np.float32)
    found = ctypes.c_size_t(0)

    def call(capacity):
        return capi.LIB.pcc_sift_keypoints(ctx._h, p.ctypes.data, len(p), 12, words.ctypes.data, 4, capi.MEM_HOST, 0.005, 5, 5, 0.001,
                                           out.ctypes.data, capacity, ctypes.byref(found))
    assert call(m - 1) == -6 and found.value == m  # PCC_ERR_OVERFLOW, the number needed
    assert b"keypoints, room for" in capi.LIB.pcc_last_error()
    assert (out == -7.0).all()  # nothing written
    assert call(m) == 0 and found.value == m
    _assert_same(out, want, "capacity exactly met")
    # the binding starts with room for 256 and asks again: sift8000 needs more
    _assert_same(ctx.sift_keypoints(*sift_util.scene("sift8000")), mirror("sift8000")["keypoints"], "retry with the needed capacity")


def test_empty_and_all_non_finite_inputs_give_no_keypoints(ctx):
    assert ctx.sift_keypoints(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8)).shape == (0, 4)
    p = np.full((40, 3), np.nan, np.float32)
    assert ctx.sift_keypoints(p, np.zeros((40, 3), np.uint8)).shape == (0, 4)


def test_first_octave_lattice_beyond_the_voxel_grids_limit_is_refused(ctx):
    p, rgb = sift_util.scene("sift300")
    with pytest.raises(capi.PccError, match="too small for this cloud") as e:
        ctx.sift_keypoints(p, rgb, min_scale=1e-4)  # 0.12 / 1e-4 = 1200 voxels per axis
    assert e.value.status == -5  # PCC_ERR_UNSUPPORTED, as pcc_voxel_grid answers
    assert len(ctx.sift_keypoints(p, rgb)) > 0  # and the handle still works


def test_the_context_handles_own_cloud_is_untouched(gpu, mirror):
    own, _ = synth.rift_cloud(5000, 23)
    q, _ = synth.rift_cloud(700, 29)
    p, rgb = sift_util.scene("sift600")
    with capi.Index(own, engine=capi.ENGINE_GRID, device=0) as ix:
        i0, d0 = ix.nn1(q)
        _assert_same(ix.sift_keypoints(p, rgb), mirror("sift600")["keypoints"], "context over another cloud")
        i1, d1 = ix.nn1(q)
        assert ix.n_original == 5000
    assert np.array_equal(i0, i1) and np.array_equal(_bits(d0), _bits(d1))


def test_cpp_surface_equals_the_python_result(ctx, mirror, tmp_path):
    from test_rift_gpu import _assert_same as assert_same_descriptors
    for name in ("sift600", "non-finite"):
        p, rgb = sift_util.scene(name)
        kp, hist, index, out = sift_util.run_driver(p, rgb, tmp_path, tag=name.replace("-", "_"))
        assert f"keypoints={len(kp)} descriptors={len(index)}" in out
        got = ctx.sift_keypoints(p, rgb)
        _assert_same(kp, np.asarray(got), f"pcc::processSift, {name}")
        _assert_same(kp, mirror(name)["keypoints"], f"pcc::processSift vs mirror, {name}")
        # processRIFTwithSIFT by hand: snap every keypoint to the first cloud point within 0.05, RIFT over the snapped cloud
        with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as tree:
            first = tree.first_within(np.ascontiguousarray(got[:, :3]), 0.05)
        first = first[first >= 0]
        assert len(first) > 0.5 * len(got)
        sp, srgb = np.ascontiguousarray(p[first]), np.ascontiguousarray(rgb[first])
        with capi.Index(sp, engine=capi.ENGINE_GRID, device=0) as snapped:
            want = snapped.rift_descriptors(srgb)
        assert_same_descriptors((hist, index), want, f"pcc::processRIFTwithSIFT, {name}")


# ---- the CLI: --sift sends the large clusters through the keypoints -----------------------------------------------------------
def _cli_scene_with_a_large_block(seed):
    """test_rift_gpu._cli_scene's floor with two of its blocks and one block of 9 x 9 x 9 = 729 filtered points (above the
    reference's 700) built the same way; the floor still holds more than 70 % of the filtered points"""
    from test_rift_gpu import _cli_scene
    pts, rgb = _cli_scene(seed, boxes=2)
    rng = np.random.default_rng(seed + 100)
    k = np.arange(9)[:, None] * 0.025 + np.array([0.004, 0.0165])[None, :]
    c = np.stack(np.meshgrid(k.reshape(-1), k.reshape(-1), k.reshape(-1), indexing="ij"), -1).reshape(-1, 3) + np.asarray((0.3, 1.2, 0.6))
    c = c + rng.uniform(-0.001, 0.001, c.shape)
    f = 128 + 100 * np.sin(40 * c[:, 0]) * np.cos(30 * c[:, 1] + 20 * c[:, 2])
    col = np.clip(np.stack([f, 0.8 * f, 255 - f], 1) + rng.normal(0, 4, (len(c), 3)), 0, 255).astype(np.uint8)
    pts, rgb = np.concatenate([pts, c.astype(np.float32)]), np.concatenate([rgb, col])
    order = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[order]), np.ascontiguousarray(rgb[order])


def _run(args, timeout=300):
    if not EXE.exists():
        subprocess.check_call(["make", "cli"], cwd=ROOT)
    r = subprocess.run([str(EXE)] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 1, r.stdout[-2000:] + r.stderr[-2000:]  # the reference always returns 1
    return r.stdout


def test_cli_sift_takes_the_large_cluster_through_keypoints(gpu, tmp_path):
    a, ca = _cli_scene_with_a_large_block(1)
    b, cb = _cli_scene_with_a_large_block(2)
    fa, fb = tmp_path / "a.ply", tmp_path / "b.ply"
    write_ply(fa, a, rgb=ca, fmt="binary")
    write_ply(fb, b, rgb=cb, fmt="binary")
    dense_res, sift_res = tmp_path / "dense.txt", tmp_path / "sift.txt"
    dense_out = _run(["--rift", "-e", fa, fb, "--results", dense_res])
    assert "SIFT Keypoints" not in dense_out
    assert _run(["--rift", "-e", fa, fb, "--results", tmp_path / "dense2.txt"]) == dense_out  # --rift alone: unchanged, repeatable
    assert (tmp_path / "dense2.txt").read_text() == dense_res.read_text()
    sift_out = _run(["--rift", "--sift", "-e", fa, fb, "--results", sift_res])
    found = [int(x) for x in re.findall(r"Computed (\d+) SIFT Keypoints", sift_out)]
    assert len(found) == 2 and all(n > 0 for n in found), found  # one large cluster per scene (scene 1 first), nothing for the 343-point blocks
    txt = sift_res.read_text()
    assert "no verdict" not in sift_out and "no verdict" not in txt
    assert "points score pcl1: " in txt and "descriptors score pcl1: " in txt and "Total number of matches found: " in txt
    assert sum(s in sift_out for s in ("The first point cloud has more information", "The second point cloud has more information",
                                       "Both point clouds have the same information")) == 1
    dense = [int(x) for x in re.findall(r"Number of descriptors: (\d+)", dense_res.read_text())]
    sparse = [int(x) for x in re.findall(r"Number of descriptors: (\d+)", txt)]
    assert len(dense) == len(sparse) == 6  # 3 clusters of PCL2, then 3 of PCL 1
    changed = [i for i in range(6) if dense[i] != sparse[i]]
    assert len(changed) == 2 and changed[0] < 3 <= changed[1], (dense, sparse)  # the large cluster of each scene, no other
    for i in changed:
        assert dense[i] > 343 and sparse[i] < dense[i] and sparse[i] <= found[1 if i < 3 else 0], (dense, sparse, found)  # (343: a small block)


def test_cli_sift_needs_rift_and_the_help_names_it(gpu, tmp_path):
    out = _run(["-h"])
    assert "--sift" in out and "--rift" in out and "700 points" in out and "processRIFTwithSIFT" in out
    r = subprocess.run([str(EXE), "--sift", "-e", "a.ply", "b.ply"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--sift needs --rift" in r.stderr
