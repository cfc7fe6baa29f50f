"""pcc_sift_keypoints_batch on the GPU (the front of the reference's processRIFTwithSIFT, src/comparator.cpp:686-822, for every
cluster at once) against the host mirror of the detector run per cloud (build/sift_host, independent of the code under test):
every slice carries the mirror's BITS in the mirror's order, whatever else is in the batch -- clouds that overlap in space,
empty clouds, clouds that leave at different octaves, a cloud above the row builder's LDS tile --, under both scale-space
layouts, on both routes of PCC_OPT_SIFT_BATCH_BRUTE_MAX, with other parameters, record layouts and strides.  The snapped
indices equal pcc_first_within's per cloud and a NumPy restatement of the reference's scan.  Also: octave rounds that do not
depend on the number of clouds, the capacity protocol, the context handle left as it was, the C++ surface through a driver,
the CLI with and without --rift-loop."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

import rift_util
import sift_util
from ply_util import write_ply
from pointcloudcomparator_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "build" / "comparator"
DRIVER = ROOT / "build" / "sift_batch_driver"
EMPTY = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))
MIXED = ["sift300", "empty", "tiny24", "tiny25", "sift600", "dups", "non-finite", "sift300", "sift2000"]
# the cloud of the LDS tile test: sparse enough that nearly every point keeps a voxel of its own at the first leaf
TILE_CLOUD = dict(n=2600, seed=31, extent=0.3)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_same(got, want, what=""):
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape, f"{what}: {got.shape[0]} keypoints, the mirror has {want.shape[0]}"
    differ = (_bits(got) != _bits(want)).any(1)
    assert not differ.any(), f"{what}: {int(differ.sum())} of {len(want)} keypoints differ in their bits, first {int(np.argmax(differ))}"


def _scene(name):
    if name == "empty":
        return EMPTY
    if name == "tile":
        return synth.rift_cloud(TILE_CLOUD["n"], TILE_CLOUD["seed"], extent=TILE_CLOUD["extent"])
    return sift_util.scene(name)


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    """(name, params, dump) -> build/sift_host's result for that scene alone, computed once"""
    tmp = tmp_path_factory.mktemp("sift_batch_host")
    cache = {}

    def get(name, params=sift_util.DEFAULTS, dump=False):
        key = (name, tuple(params), dump)
        if key not in cache:
            if name == "empty":
                cache[key] = dict(keypoints=np.zeros((0, 4), np.float32), info=dict(octaves="0"), octaves=[])
            else:
                p, rgb = _scene(name)
                cache[key] = sift_util.run_host(p, rgb, tmp, tag=f"{name.replace('-', '_')}_{len(cache)}", params=params, dump=dump)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def ctx(gpu):
    """a context handle over a cloud that has nothing to do with the scenes"""
    p, _ = synth.rift_cloud(200, 3)
    with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
        yield ix


def _batch(names):
    scenes = [_scene(n) for n in names]
    return [s[0] for s in scenes], [s[1] for s in scenes]


def _assert_slices(kp, off, names, mirror, what, params=sift_util.DEFAULTS):
    assert off.shape == (len(names) + 1,) and off[0] == 0 and off[-1] == len(kp) and (np.diff(off) >= 0).all()
    for c, name in enumerate(names):
        _assert_same(kp[off[c]:off[c + 1]], mirror(name, params)["keypoints"], f"{what}: cloud {c} ({name})")


# ---- 1. the mixed batch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [1, 0])
def test_mixed_batch_carries_the_mirrors_bits_cloud_by_cloud(ctx, mirror, layout):
    """clouds near the origin that overlap in space (the isolation check), leaving the batch in different rounds"""
    pts, rgbs = _batch(MIXED)
    octaves = {int(mirror(n)["info"]["octaves"]) for n in MIXED}
    assert len(octaves) >= 3, octaves
    ctx.set_option(capi.OPT_SIFT_LAYOUT, layout)
    try:
        kp, off = ctx.sift_keypoints_batch(pts, rgbs)
    finally:
        ctx.set_option(capi.OPT_SIFT_LAYOUT, 1)
    _assert_slices(kp, off, MIXED, mirror, f"layout {layout}")
    first, second = [i for i, n in enumerate(MIXED) if n == "sift300"]
    assert np.array_equal(_bits(kp[off[first]:off[first + 1]]), _bits(kp[off[second]:off[second + 1]])) and off[first + 1] > off[first]
    for name in ("empty", "tiny24", "tiny25"):
        c = MIXED.index(name)
        assert off[c + 1] == off[c], name


# ---- 2. a cloud above the row builder's LDS tile -----------------------------------------------------------------------------
def test_a_first_octave_cloud_beyond_one_lds_tile(ctx, mirror):
    names = ["sift300", "tile", "sift300"]
    first = mirror("tile", dump=True)["octaves"][0]
    assert len(first["cloud"]) > 2048, len(first["cloud"])  # RB_TILE: the builders stage this cloud in two tiles
    assert int(mirror("tile")["info"]["rows_min"]) < 25  # ... and some of its points have to scan for their 25 neighbours
    pts, rgbs = _batch(names)
    kp, off = ctx.sift_keypoints_batch(pts, rgbs)
    assert off[2] > off[1]
    _assert_slices(kp, off, names, mirror, "tile")


# ---- 3. both routes ----------------------------------------------------------------------------------------------------------
def test_both_routes_give_the_same_bits(ctx, mirror):
    pts, rgbs = _batch(MIXED)
    sizes = [len(p) for p in pts]
    default = ctx.get_option(capi.OPT_SIFT_BATCH_BRUTE_MAX)
    try:
        for limit in (500, 0, default):
            ctx.set_option(capi.OPT_SIFT_BATCH_BRUTE_MAX, limit)
            kp, off, snap = ctx.sift_keypoints_batch(pts, rgbs, snap_radius=0.05)
            stats = ctx.stats()
            _assert_slices(kp, off, MIXED, mirror, f"brute limit {limit}")
            assert (int(stats[0]), int(stats[1])) == (sum(s for s in sizes if s <= limit), sum(s for s in sizes if s > limit)), limit
            for c, p in enumerate(pts):
                if off[c + 1] > off[c]:
                    with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as tree:
                        want = tree.first_within(np.ascontiguousarray(kp[off[c]:off[c + 1], :3]), 0.05)
                    assert np.array_equal(snap[off[c]:off[c + 1]], want), (limit, c)
    finally:
        ctx.set_option(capi.OPT_SIFT_BATCH_BRUTE_MAX, default)


# ---- 4. rounds, not clouds ---------------------------------------------------------------------------------------------------
def test_octave_rounds_do_not_depend_on_the_number_of_clouds(ctx, mirror):
    pts, rgbs = _batch(MIXED)
    kp, off = ctx.sift_keypoints_batch(pts, rgbs)
    rounds = int(ctx.stats()[2])
    assert 1 <= rounds <= sift_util.DEFAULTS[1]
    kp4, off4 = ctx.sift_keypoints_batch(pts * 4, rgbs * 4)
    assert int(ctx.stats()[2]) == rounds
    assert len(off4) == 37 and len(kp4) == 4 * len(kp)
    _assert_slices(kp4, off4, MIXED * 4, mirror, "36 clouds")


# ---- 5. other parameters -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", [(0.004, 3, 13, 0.0), (0.006, 4, 1, 0.002)])
def test_other_parameters(ctx, mirror, params):
    names = ["sift600", "sift300"]
    pts, rgbs = _batch(names)
    assert len(mirror("sift600", params)["keypoints"]) > 0
    kp, off = ctx.sift_keypoints_batch(pts, rgbs, *params)
    _assert_slices(kp, off, names, mirror, f"{params}", params=params)


# ---- 6. the snap -------------------------------------------------------------------------------------------------------------
def _first_within_numpy(cloud, keypoints, radius):
    """the reference's scan (src/comparator.cpp:696-713): float differences, float64 squares, sum and sqrt, the first index"""
    out = np.full(len(keypoints), -1, np.int32)
    for k, q in enumerate(np.asarray(keypoints[:, :3], np.float32)):
        d = (q[None, :] - cloud).astype(np.float32).astype(np.float64)  # the difference is taken in float32
        with np.errstate(invalid="ignore", over="ignore"):
            hit = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]) < radius
        if hit.any():
            out[k] = int(np.argmax(hit))
    return out


@pytest.mark.parametrize("radius", [0.05, 0.004])
def test_snap_equals_first_within_and_the_references_scan(ctx, mirror, radius):
    pts, rgbs = _batch(MIXED)
    kp, off, snap = ctx.sift_keypoints_batch(pts, rgbs, snap_radius=radius)
    _assert_slices(kp, off, MIXED, mirror, f"snap {radius}")
    assert snap.dtype == np.int32 and snap.shape == (len(kp),)
    for c, p in enumerate(pts):
        mine = kp[off[c]:off[c + 1]]
        if len(mine) == 0:
            continue
        with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as tree:
            want = tree.first_within(np.ascontiguousarray(mine[:, :3]), radius)
        assert np.array_equal(snap[off[c]:off[c + 1]], want), (radius, c)
        assert np.array_equal(snap[off[c]:off[c + 1]], _first_within_numpy(p, mine, radius)), (radius, c)
    if radius == 0.004:
        assert (snap == -1).any() and (snap >= 0).any()
    else:
        assert (snap >= 0).any()


# ---- 7. capacity -------------------------------------------------------------------------------------------------------------
def test_capacity_one_short_overflows_and_the_handle_still_works(gpu, mirror):
    own, _ = synth.rift_cloud(5000, 23)
    q, _ = synth.rift_cloud(700, 29)
    pts, rgbs = _batch(MIXED)
    words = [np.ascontiguousarray(synth.pack_rgb(c)) for c in rgbs]
    true_off = np.concatenate([[0], np.cumsum([len(mirror(n)["keypoints"]) for n in MIXED])])
    m = int(true_off[-1])
    nc = len(MIXED)
    pp = (ctypes.c_void_p * nc)(*[p.ctypes.data if len(p) else None for p in pts])
    cp = (ctypes.c_void_p * nc)(*[w.ctypes.data if len(w) else None for w in words])
    nn = (ctypes.c_size_t * nc)(*[len(p) for p in pts])
    kp, snap, off = np.full((m, 4), -7.0, np.float32), np.full(m, -7, np.int32), np.full(nc + 1, 99, np.uintp)
    with capi.Index(own, engine=capi.ENGINE_GRID, device=0) as ix:
        i0, d0 = ix.nn1(q)

        def call(capacity):
            return capi.LIB.pcc_sift_keypoints_batch(ix._h, nc, pp, nn, 12, cp, 4, capi.MEM_HOST, 0.005, 5, 5, 0.001, 0.05, kp.ctypes.data,
                                                     snap.ctypes.data, capacity, off.ctypes.data)
        assert call(m - 1) == -6  # PCC_ERR_OVERFLOW
        assert b"keypoints, room for" in capi.LIB.pcc_last_error()
        assert np.array_equal(off.astype(np.int64), true_off)  # the offsets that would have been returned
        assert (kp == -7.0).all() and (snap == -7).all()  # nothing else written
        off[:] = 99
        assert call(m) == 0 and np.array_equal(off.astype(np.int64), true_off)
        _assert_slices(kp, off.astype(np.int64), MIXED, mirror, "capacity exactly met")
        assert (snap >= -1).all() and (snap >= 0).any()  # (written: the sentinel is gone)
        i1, d1 = ix.nn1(q)
        assert ix.n_original == 5000
    assert np.array_equal(i0, i1) and np.array_equal(_bits(d0), _bits(d1))  # the context's own index is as it was


# ---- 8. records and strides --------------------------------------------------------------------------------------------------
def test_records_packed_words_and_rgb_triples_give_the_same_bits(ctx, mirror):
    names = ["sift300", "non-finite", "empty", "sift600"]
    pts, rgbs = _batch(names)
    kp_a, off_a = ctx.sift_keypoints_batch(pts, rgbs)  # 12-byte points, (n, 3) uint8 colours
    _assert_slices(kp_a, off_a, names, mirror, "r g b")
    kp_b, off_b = ctx.sift_keypoints_batch(pts, [synth.pack_rgb(c) for c in rgbs])  # packed words
    recs = [synth.xyzrgb_records(p, c) for p, c in zip(pts, rgbs)]  # pcl::PointXYZRGB: 32-byte stride, rgb = pts + 16
    kp_c, off_c = ctx.sift_keypoints_batch(recs)
    for kp, off, what in ((kp_b, off_b, "packed words"), (kp_c, off_c, "records")):
        assert np.array_equal(off, off_a) and np.array_equal(_bits(kp), _bits(kp_a)), what


# ---- 9. C++ ------------------------------------------------------------------------------------------------------------------
def test_cpp_batch_functions_equal_the_per_cloud_functions(gpu, mirror, tmp_path):
    if not DRIVER.exists():
        subprocess.check_call(["make", "build/sift_batch_driver"], cwd=ROOT)
    names = ["sift600", "non-finite", "tiny25"]
    files = []
    for name in names:
        files.append(tmp_path / f"{name.replace('-', '_')}.in")
        rift_util.write_cloud(files[-1], *_scene(name))
    r = subprocess.run([str(DRIVER), str(tmp_path / "out")] + [str(f) for f in files], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    total = sum(len(mirror(n)["keypoints"]) for n in names)
    assert f"clouds=3 keypoints={total} " in r.stdout and total > 0
    batch, loop = (tmp_path / "out.batch").read_bytes(), (tmp_path / "out.loop").read_bytes()
    assert batch == loop and len(batch) > 3 * 8 + total * 16
    # and the keypoints in the file are the mirror's
    at = 0
    for name in names:
        m = int(np.frombuffer(batch[at:at + 4], np.int32)[0])
        _assert_same(np.frombuffer(batch[at + 4:at + 4 + m * 16], np.float32).reshape(m, 4), mirror(name)["keypoints"], f"pcc::processSiftBatch, {name}")
        k = int(np.frombuffer(batch[at + 4 + m * 16:at + 8 + m * 16], np.int32)[0])
        assert k <= m
        at += 8 + m * 16 + k * 16
    assert at == len(batch)


# ---- 10. the CLI -------------------------------------------------------------------------------------------------------------
def test_cli_sift_batch_and_loop_print_and_write_the_same(gpu, tmp_path):
    import re
    from test_rift_batch_gpu import _cli_scene
    a, ca = _cli_scene(1, boxes=2, big=True)
    b, cb = _cli_scene(2, boxes=2, big=True)
    fa, fb = tmp_path / "a.ply", tmp_path / "b.ply"
    write_ply(fa, a, rgb=ca, fmt="binary")
    write_ply(fb, b, rgb=cb, fmt="binary")
    if not EXE.exists():
        subprocess.check_call(["make", "cli"], cwd=ROOT)
    outs = []
    for tag, extra in (("batch", []), ("loop", ["--rift-loop"])):
        r = subprocess.run([str(EXE), "--rift", "--sift"] + extra + ["-e", str(fa), str(fb), "--results", str(tmp_path / f"{tag}.txt")],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 1, r.stdout[-2000:] + r.stderr[-2000:]  # the reference always returns 1
        outs.append(r.stdout)
    assert outs[0] == outs[1]  # (the CLI prints no timing line)
    assert (tmp_path / "batch.txt").read_text() == (tmp_path / "loop.txt").read_text()
    found = [int(x) for x in re.findall(r"Computed (\d+) SIFT Keypoints", outs[0])]
    assert len(found) == 2 and all(f > 0 for f in found), found  # one cluster above 700 points per scene
