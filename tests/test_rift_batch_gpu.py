"""pcc_rift_descriptors_batch on the GPU (the reference's per-cluster descriptor loop, src/comparator.cpp:1224-1272, each turn
processRIFT, :590-684).  The expected values come from the host mirror of the pipeline (build/rift_host: the headers the
kernels are compiled from, exhaustive rows, one core) run on each cloud ALONE: every slice of a batch -- histogram bits and
local point indices -- equals the mirror's, in both layouts of the unchanged histogram kernel.  The GPU is never compared with
the code under test.  No tolerance anywhere."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import rift_util
from ply_util import write_ply
from pointcloudcomparator_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "build" / "comparator"
BATCH_DRIVER = ROOT / "build" / "rift_batch_driver"
EMPTY = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))
NOTHING = (np.zeros((0, 32), np.float32), np.zeros(0, np.int32))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_same(got, want, what=""):
    gh, gi = got
    wh, wi = want
    assert np.array_equal(np.asarray(gi), wi), f"{what}: kept point indices differ"
    assert gh.shape == wh.shape == (len(wi), 32)
    differ = (_bits(gh) != _bits(wh)).any(1)
    assert not differ.any(), f"{what}: {int(differ.sum())} of {len(wi)} histograms differ in their bits, first {int(np.argmax(differ))}"


def _cloud(n, seed=None):
    """the generator of the single call's scenes at their density (600 points per 0.12 m cube), in the same corner of space
    whatever n: clouds of one batch overlap, so a neighbour from another cloud would change bits"""
    return synth.rift_cloud(n, 100 + n if seed is None else seed, extent=0.12 * (n / 600) ** (1 / 3))


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    """tag, cloud -> (hist, index) of build/rift_host on that cloud alone, computed once per tag and left unchanged"""
    tmp = tmp_path_factory.mktemp("rift_batch_host")
    cache = {}

    def get(tag, cloud, radii=()):
        if tag not in cache:
            p, rgb = cloud
            got = NOTHING if len(p) == 0 else rift_util.run_tool(rift_util.HOST, p, rgb, tmp, tag=tag, radii=radii)[:2]
            got[0].setflags(write=False)
            got[1].setflags(write=False)
            cache[tag] = got
        return cache[tag]
    return get


@pytest.fixture(scope="module")
def ctx(gpu):
    """one context handle for the module: it indexes a cloud of its own, which no batch may read or change"""
    pts = synth.corridor_cloud(5000, synth.SEED_A)
    with capi.Index(pts, engine=capi.ENGINE_GRID, device=0) as ix:
        yield ix, pts


SIZES = (1, 2, 3, 63, 64, 65, 257, 700, 701, 2049)


@pytest.mark.parametrize("layout", [1, 0])
def test_overlapping_clouds_carry_the_mirrors_bits(ctx, mirror, layout):
    """sizes around the wave width, the largest query block and the 2048-point LDS tile, an empty cloud in the middle and one with
    non-finite points: all in the same corner of space"""
    ix, _ = ctx
    clouds = [(f"n{n}", _cloud(n)) for n in SIZES]
    clouds.insert(5, ("empty", EMPTY))
    clouds.append(("non_finite", rift_util.scene("non-finite")))
    want = [mirror(tag, c) for tag, c in clouds]
    # the mirror first: no comparison of empty sets by accident
    for (tag, c), w in zip(clouds, want):
        if tag.startswith("n") and tag != "non_finite":
            n = len(c[0])
            assert len(w[1]) == (0 if n < 3 else n), tag
    assert 0 < len(want[-1][1]) < 500
    ix.set_option(capi.OPT_RIFT_LAYOUT, layout)
    try:
        got = ix.rift_descriptors_batch([c[0] for _, c in clouds], [c[1] for _, c in clouds])
    finally:
        ix.set_option(capi.OPT_RIFT_LAYOUT, 1)
    assert len(got) == len(clouds)
    for (tag, _), g, w in zip(clouds, got, want):
        _assert_same(g, w, f"{tag}, layout {layout}")
        assert g[0].dtype == np.float32 and g[1].dtype == np.int32
        assert (np.diff(g[1]) > 0).all()  # ascending local indices


def test_the_same_cloud_several_times(ctx, mirror):
    ix, _ = ctx
    a, iso = _cloud(257), rift_util.scene("isolated")
    got = ix.rift_descriptors_batch([a[0], iso[0], a[0], a[0], iso[0]], [a[1], iso[1], a[1], a[1], iso[1]])
    wa, wi = mirror("n257", a), mirror("isolated", iso)
    assert len(wa[1]) == 257 and 0 < len(wi[1]) < len(iso[0])
    for k, w in zip(range(5), (wa, wi, wa, wa, wi)):
        _assert_same(got[k], w, f"cloud {k}")


def test_long_rows_and_several_lds_tiles(ctx, mirror):
    """4000 points in the 0.12 m cube: most 5 cm rows are longer than the 512 entries the register sort takes (the long-row
    sort), and the cloud is two LDS tiles; alone and beside a small cloud"""
    ix, _ = ctx
    big, small = synth.rift_cloud(4000, 31, extent=0.12), _cloud(300)
    p = big[0].astype(np.float32)
    rows = np.zeros(len(p), np.int64)
    for s in range(0, len(p), 500):  # the library's arithmetic: ((dx * dx) + dy * dy) + dz * dz in float32
        d = p[s:s + 500, None, :] - p[None, :, :]
        d = d * d
        rows[s:s + 500] = (((d[..., 0] + d[..., 1]) + d[..., 2]) < np.float32(0.05 * 0.05)).sum(1)
    assert (rows > 512).sum() > 1000 and rows.max() > 512
    wb, ws = mirror("big4000", big), mirror("n300", small)
    assert len(wb[1]) == 4000 and len(ws[1]) == 300
    alone = ix.rift_descriptors_batch([big[0]], [big[1]])
    _assert_same(alone[0], wb, "4000 points alone")
    both = ix.rift_descriptors_batch([small[0], big[0]], [small[1], big[1]])
    _assert_same(both[0], ws, "300 points beside 4000")
    _assert_same(both[1], wb, "4000 points beside 300")


def test_many_small_clouds(ctx, mirror):
    """200 clouds of 24 ... 40 points: table indexing and bases"""
    ix, _ = ctx
    clouds = [_cloud(24 + k % 17, seed=1000 + k) for k in range(200)]
    want = [mirror(f"small{k}", c) for k, c in enumerate(clouds)]
    assert sum(len(w[1]) for w in want) > 0.9 * sum(len(c[0]) for c in clouds)
    got = ix.rift_descriptors_batch([c[0] for c in clouds], [c[1] for c in clouds])
    for k, (g, w) in enumerate(zip(got, want)):
        _assert_same(g, w, f"cloud {k} of 200")


def test_full_query_blocks(ctx, mirror):
    """96 clouds of 700 points: the one batch of this file large enough for the table to keep its blocks of 64 queries (1056
    items; every smaller batch above runs on blocks of 4 to 32)"""
    ix, _ = ctx
    clouds = [_cloud(700, seed=3000 + k) for k in range(96)]
    want = [mirror(f"full{k}", c) for k, c in enumerate(clouds)]
    assert sum(len(w[1]) for w in want) == 96 * 700
    got = ix.rift_descriptors_batch([c[0] for c in clouds], [c[1] for c in clouds])
    for k, (g, w) in enumerate(zip(got, want)):
        _assert_same(g, w, f"cloud {k} of 96")


def test_other_radii(ctx, mirror):
    """gradient radius != normal radius: a third CSR"""
    ix, _ = ctx
    radii = (0.025, 0.035, 0.045)
    clouds = [_cloud(300), _cloud(65), rift_util.scene("isolated")]
    want = [mirror(f"radii{k}", c, radii=radii) for k, c in enumerate(clouds)]
    assert len(want[0][1]) > 250 and len(want[2][1]) > 0
    got = ix.rift_descriptors_batch([c[0] for c in clouds], [c[1] for c in clouds], *radii)
    for k, (g, w) in enumerate(zip(got, want)):
        _assert_same(g, w, f"radii 0.025 / 0.035 / 0.045, cloud {k}")


def test_work_handle_route_gives_the_same_bits(ctx, mirror):
    ix, _ = ctx
    clouds = [_cloud(300), _cloud(600), _cloud(700)]
    want = [mirror(f"n{len(c[0])}", c) for c in clouds]
    assert [len(w[1]) for w in want] == [300, 600, 700]
    default = ix.get_option(capi.OPT_RIFT_BATCH_BRUTE_MAX)
    assert default >= 700
    ix.set_option(capi.OPT_RIFT_BATCH_BRUTE_MAX, 500)
    try:
        got = ix.rift_descriptors_batch([c[0] for c in clouds], [c[1] for c in clouds])
        stats = ix.stats()
    finally:
        ix.set_option(capi.OPT_RIFT_BATCH_BRUTE_MAX, default)
    for k, (g, w) in enumerate(zip(got, want)):
        _assert_same(g, w, f"brute limit 500, cloud {k}")
    assert (int(stats[0]), int(stats[1])) == (300, 1300)
    got = ix.rift_descriptors_batch([c[0] for c in clouds], [c[1] for c in clouds])  # the same handle, the limit set back
    for k, (g, w) in enumerate(zip(got, want)):
        _assert_same(g, w, f"brute limit back, cloud {k}")
    stats = ix.stats()
    assert (int(stats[0]), int(stats[1])) == (1600, 0)


def test_refusals_on_a_live_handle(ctx, mirror):
    ix, _ = ctx
    c = _cloud(300)
    with pytest.raises(Exception, match="only 4 distance x 8 gradient bins"):
        ix.rift_descriptors_batch([c[0]], [c[1]], nr_distance_bins=8, nr_gradient_bins=4)
    with pytest.raises(Exception, match="bad radius"):
        ix.rift_descriptors_batch([c[0]], [c[1]], rift_radius=0.0)
    assert ix.rift_descriptors_batch([], []) == []
    got = ix.rift_descriptors_batch([c[0]], [c[1]])  # and the handle still works
    _assert_same(got[0], mirror("n300", c), "after the refusals")


def test_the_call_changes_nothing_else(ctx, mirror):
    """between two ordinary searches on the context handle: its own cloud answers as before"""
    import oracle
    ix, pts = ctx
    q = synth.corridor_cloud(1000, synth.SEED_B)
    oi, od = oracle.nn1_exhaustive(pts, q)
    i0, d0 = ix.nn1(q)
    c = synth.xyzrgb_records(*_cloud(257))  # pcl::PointXYZRGB records: the colour word read in place
    got = ix.rift_descriptors_batch([c, c[:65]])
    i1, d1 = ix.nn1(q)
    _assert_same(got[0], mirror("n257", _cloud(257)), "records")
    assert len(got[1][1]) > 0
    for i, d in ((i0, d0), (i1, d1)):
        assert np.array_equal(i, oi) and np.array_equal(_bits(d), _bits(od))
    assert ix.size == 5000
    # and the module-level form with a handle of its own
    own = capi.rift_descriptors_batch([c])
    _assert_same(own[0], got[0], "one-point context")


def test_cpp_processRIFTBatch_equals_the_loop_and_the_mirror(gpu, mirror, tmp_path):
    if not BATCH_DRIVER.exists():
        subprocess.check_call(["make", "build/rift_batch_driver"], cwd=ROOT)
    clouds = [("isolated", rift_util.scene("isolated")), ("empty", EMPTY), ("n65", _cloud(65)), ("non_finite", rift_util.scene("non-finite"))]
    files = []
    for tag, (p, rgb) in clouds:
        files.append(tmp_path / f"{tag}.in")
        rift_util.write_cloud(files[-1], p, rgb)
    r = subprocess.run([str(BATCH_DRIVER), str(tmp_path / "out")] + [str(f) for f in files], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "clouds=4" in r.stdout and "differ_from_loop=0" in r.stdout  # pcc::processRIFT per cloud, compared in the driver
    for k, (tag, c) in enumerate(clouds):
        _assert_same(rift_util.read_result(tmp_path / f"out.{k}"), mirror(tag, c), f"pcc::processRIFTBatch vs mirror, {tag}")


# ---- the CLI: one batch call or the per-cluster loop, same files -----------------------------------------------------------
def _cli_scene(seed, boxes=4, big=False):
    """tests/test_rift_gpu.py's scene: a floor the plane loop removes and `boxes` coloured blocks that become the clusters,
    7 x 7 x 7 points each after the VoxelGrid.  big: tests/test_sift_gpu.py's scene -- one more block of 9 x 9 x 9 = 729 filtered
    points, a cluster above the reference's 700, where the third small block would stand."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(62), np.arange(62), indexing="ij"), -1).reshape(-1, 2) * 0.03
    floor = np.concatenate([g + 0.01, np.full((len(g), 1), 0.01)], 1)

    def block(m):
        k = np.arange(m)[:, None] * 0.025 + np.array([0.004, 0.0165])[None, :]
        return np.stack(np.meshgrid(k.reshape(-1), k.reshape(-1), k.reshape(-1), indexing="ij"), -1).reshape(-1, 3)
    origins = [(0.3, 0.3, 0.3), (1.2, 0.3, 0.45), (0.3, 1.2, 0.6), (1.2, 1.2, 0.3)][:boxes]
    blocks = [block(7) + np.asarray(o) for o in origins]
    if big:
        blocks.append(block(9) + np.asarray((0.3, 1.2, 0.6)))
    pts = np.concatenate([floor] + blocks)
    pts = pts + rng.uniform(-0.001, 0.001, pts.shape)
    f = 128 + 100 * np.sin(40 * pts[:, 0]) * np.cos(30 * pts[:, 1] + 20 * pts[:, 2])
    rgb = np.clip(np.stack([f, 0.8 * f, 255 - f], 1) + rng.normal(0, 4, (len(pts), 3)), 0, 255).astype(np.uint8)
    order = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[order].astype(np.float32)), np.ascontiguousarray(rgb[order])


def _run(args, timeout=300):
    if not EXE.exists():
        subprocess.check_call(["make", "cli"], cwd=ROOT)
    r = subprocess.run([str(EXE)] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 1, r.stdout[-2000:] + r.stderr[-2000:]  # the reference always returns 1
    return r.stdout


@pytest.mark.parametrize("sift", [False, True])
def test_cli_batch_and_loop_write_the_same_files(gpu, tmp_path, sift):
    a, ca = _cli_scene(1, boxes=2 if sift else 4, big=sift)
    b, cb = _cli_scene(2, boxes=2 if sift else 3, big=sift)
    fa, fb = tmp_path / "a.ply", tmp_path / "b.ply"
    write_ply(fa, a, rgb=ca, fmt="binary")
    write_ply(fb, b, rgb=cb, fmt="binary")
    flags = ["--rift", "--sift"] if sift else ["--rift"]
    out_b = _run(flags + ["-e", fa, fb, "--results", tmp_path / "batch.txt", "--dump-descriptors", tmp_path / "batch"])
    out_l = _run(flags + ["--rift-loop", "-e", fa, fb, "--results", tmp_path / "loop.txt", "--dump-descriptors", tmp_path / "loop"])
    txt = (tmp_path / "batch.txt").read_text()
    assert txt == (tmp_path / "loop.txt").read_text()
    for k in (1, 2):
        assert (tmp_path / f"batch_{k}.txt").read_bytes() == (tmp_path / f"loop_{k}.txt").read_bytes()
    counts = [int(x) for x in re.findall(r"Number of descriptors: (\d+)", txt)]
    assert len(counts) == (6 if sift else 7) and sum(c > 0 for c in counts) >= 4, counts  # (the 343-point blocks at least)
    assert "no verdict" not in out_b and out_b == out_l  # printed lines, the keypoint counts among them, and the verdict
    if sift:
        found = [int(x) for x in re.findall(r"Computed (\d+) SIFT Keypoints", out_b)]
        assert len(found) == 2 and all(f > 0 for f in found), found  # one cluster above 700 points per scene
        assert max(counts) < 700  # ... described at its keypoints, not densely
    else:
        assert all(c > 0 for c in counts), counts


def test_cli_help_names_the_loop_switch(gpu):
    out = _run(["-h"])
    assert "--rift-loop" in out and "processRIFTBatch" in out
