"""pcc_region_growing_rgb_batch on the GPU (csrc/region_rgb_batch.hip; reference src/comparator.cpp:1456-1495 calling
src/segmentation.cpp:161-216 twice per accepted match): every cloud's slice of Index.region_growing_rgb_batch against the
oracle's restatement fed the rows of a FRESH index over that cloud alone, and against the single call on that index -- bit for
bit, no tolerance.  Every test that means to cover the batch kernels also holds stats[2] / stats[3] to the expected split, so
that a call which quietly took the single path fails."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle
from pointcloudcomparator_amd import capi

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import rgb_device_util as util  # noqa: E402
from ply_util import write_ply  # noqa: E402
from test_rgb_gpu import _scenes  # noqa: E402

pytestmark = pytest.mark.gpu

RB_TILE = 2048  # csrc/rift_batch_plan.hpp: points of a cloud a workgroup holds in LDS at a time


def _alone(pts, rgb, **kw):
    """cloud c alone: ((labels, n) the oracle gives over a fresh index's rows, stats of the single call on that index), the single
    call held to the oracle on the way.  Non-finite points: the oracle sees the stripped cloud, they get -1."""
    pts = np.ascontiguousarray(pts, np.float32)
    keep = np.isfinite(pts).all(1)
    if len(pts) == 0 or not keep.any():
        return (np.full(len(pts), -1, np.int32), 0), None
    fp, frgb = np.ascontiguousarray(pts[keep]), rgb[keep]
    with capi.Index(fp) as ix:
        ki, kd = ix.knn(fp, min(kw.get("region_nn", 100), len(fp)))
    want_f = oracle.region_growing_rgb(fp, frgb, neighbours=ki, neighbour_d2=kd, **kw)
    labels = np.full(len(pts), -1, np.int32)
    labels[keep] = want_f[0]
    with capi.Index(pts) as ix:
        got = ix.region_growing_rgb(rgb, **kw)
        stats = ix.stats()
    assert got[1] == want_f[1] and (got[0] == labels).all(), "the single call differs from the oracle"
    return (labels, want_f[1]), stats


def _same(got, want, what):
    assert len(got) == len(want), what
    for c, (g, w) in enumerate(zip(got, want)):
        assert g[1] == w[1], (what, "cloud", c, "clusters", g[1], w[1])
        assert g[0].dtype == np.int32 and g[0].shape == w[0].shape, (what, c)
        assert (g[0] == w[0]).all(), (what, "cloud", c, np.nonzero(g[0] != w[0])[0][:10])


def _batch(ctx, clouds, rgbs, split, **kw):
    """the batch call on ctx; split = (points through the batch kernels, points through the work handle)"""
    got = ctx.region_growing_rgb_batch(clouds, rgbs, **kw)
    stats = ctx.stats()
    assert (stats[2], stats[3]) == split, (stats[2], stats[3], split)
    return got, stats


@pytest.fixture(scope="module")
def ctx(gpu):
    with capi.Index(np.zeros((1, 3), np.float32)) as ix:
        yield ix


@pytest.fixture(scope="module")
def fix_scenes(gpu):
    return {name: (pts, rgb) for name, pts, rgb in util.fixpoint_scenes()}


@pytest.fixture(scope="module")
def mixed(gpu, fix_scenes):
    """the six scenes of the order-free argument and the painted room, growing stage alone (region_colour = 0, min_size = 1:
    the clusters are the grown segments): name -> (points, colours, oracle result, single call's stats)"""
    out = {}
    room = next(s for s in _scenes() if s[0] == "room")
    for name, (pts, rgb) in list(fix_scenes.items()) + [("room", (room[1], room[2]))]:
        want, stats = _alone(pts, rgb, region_colour=0.0, min_size=1)
        out[name] = (pts, rgb, want, stats)
    return out


def test_mixed_scenes_in_one_call(ctx, mixed):
    """noise fills the pair table, patches and cascade need several sweeps, room (30 000 points) goes through the work handle in
    the same call: every slice is its cloud's own result; segments and pairs are the sums over the batch route's clouds.  One
    sweep loop serves all clouds, so it cannot end before the cascades' (their count does not vary: the test below); the count
    itself is decided by patches here, whose long label chains settle in 3 or 4 sweeps from run to run, alone (4 in 21 of 25 runs
    on an MI355X, 3 in 4) and in the batch (4 in 20 of 25, 3 in 5) -- a label may travel more than one edge within a sweep when
    the waves happen to run in that order -- so no equality is asked of it."""
    names = ["patches", "near", "noise", "tiny", "cascade", "cascade_rev", "room"]
    on_route = names[:-1]
    n_route = sum(len(mixed[k][0]) for k in on_route)
    got, stats = _batch(ctx, [mixed[k][0] for k in names], [mixed[k][1] for k in names], (n_route, len(mixed["room"][0])),
                        region_colour=0.0, min_size=1)
    _same(got, [mixed[k][2] for k in names], names)
    single = {k: mixed[k][3] for k in on_route}
    print("single sweeps", {k: single[k][7] for k in on_route}, "batch sweeps", stats[7], "segments", stats[0], "pairs", stats[1])
    assert stats[0] == sum(single[k][0] for k in on_route)
    assert stats[1] == sum(single[k][1] for k in on_route)
    assert stats[1] > 0 and single["noise"][1] > 0
    assert stats[7] >= max(single["cascade"][7], single["cascade_rev"][7]) > 1


def test_cascades_share_one_sweep_loop(ctx, mixed):
    """cascade and cascade_rev in the same call: one settles in one sweep, the other needs several, so the one loop that serves
    both runs for the larger of their single-call sweep counts"""
    names = ["cascade", "cascade_rev"]
    got, stats = _batch(ctx, [mixed[k][0] for k in names], [mixed[k][1] for k in names], (480, 0), region_colour=0.0, min_size=1)
    _same(got, [mixed[k][2] for k in names], names)
    alone = [mixed[k][3][7] for k in names]
    print("single sweeps", alone, "batch sweeps", stats[7])
    assert min(alone) == 1 and max(alone) > 1
    assert stats[7] == max(alone)
    assert stats[0] == sum(mixed[k][3][0] for k in names) and stats[1] == sum(mixed[k][3][1] for k in names)


def _two_level(rng, n):
    return (rng.integers(0, 2, (n, 3)) * 50).astype(np.uint8)


def test_row_clamp_and_padding(ctx):
    """clouds below, at and above K = 100 and the 64- and 128-key lists of the merge network, all in one call: rows are clamped to
    the cloud's own points and padded with the empty key"""
    rng = np.random.default_rng(21)
    sizes = [1, 2, 11, 63, 64, 65, 100, 101, 127, 128, 129]
    clouds = [rng.random((n, 3)).astype(np.float32) for n in sizes]
    rgbs = [_two_level(rng, n) for n in sizes]
    want = [_alone(p, c, min_size=1)[0] for p, c in zip(clouds, rgbs)]
    got, _ = _batch(ctx, clouds, rgbs, (sum(sizes), 0), min_size=1)
    _same(got, want, sizes)
    assert all(w[1] >= 1 for w in want)


def _lattice(rng, n):
    """n points on a 0.01 lattice of 12 x 12 x 12 nodes: many exact-distance ties, and every node several times over"""
    return (rng.integers(0, 12, (n, 3)) * 0.01).astype(np.float32)


@pytest.mark.parametrize("kw", [dict(region_colour=0.0, min_size=1), dict()], ids=["growing", "defaults"])
def test_tile_edges_with_ties(ctx, kw):
    """one, one, two and three LDS tiles; equal distances and repeated points all over, so that the order of equal keys -- lowest
    index first -- is decided across tile boundaries"""
    rng = np.random.default_rng(22)
    sizes = [RB_TILE - 1, RB_TILE, RB_TILE + 1, 2 * RB_TILE + 4]
    clouds = [_lattice(rng, n) for n in sizes]
    rgbs = [(rng.integers(0, 3, (n, 3)) * 20).astype(np.uint8) for n in sizes]
    want = [_alone(p, c, **kw)[0] for p, c in zip(clouds, rgbs)]
    got, _ = _batch(ctx, clouds, rgbs, (sum(sizes), 0), **kw)
    _same(got, want, (sizes, kw))


def test_overlapping_clouds_share_nothing(ctx, fix_scenes):
    """the same 3000 coordinates three times under three colourings, and once more shifted by 1e-4: every slice is its cloud's own
    result, so no row, segment or pair crosses a cloud"""
    pts = fix_scenes["patches"][0]
    clouds = [pts, pts, pts, (pts + np.float32(1e-4)).astype(np.float32)]
    rgbs = [fix_scenes["patches"][1], fix_scenes["near"][1], fix_scenes["noise"][1], fix_scenes["patches"][1]]
    kw = dict(min_size=15)
    want = [_alone(p, c, **kw)[0] for p, c in zip(clouds, rgbs)]
    got, _ = _batch(ctx, clouds, rgbs, (4 * len(pts), 0), **kw)
    _same(got, want, "overlap")
    assert len({w[1] for w in want[:3]}) > 1, "the colourings must differ in their clusters"


def test_non_finite_points_and_empty_clouds(ctx, fix_scenes):
    """NaN / inf at the first, a middle and the last index of the middle cloud of three; a cloud without a finite point; a cloud
    without a point between two others"""
    pts, rgb = fix_scenes["patches"]
    a, b, c = pts[:900].copy(), pts[900:1900].copy(), pts[1900:].copy()
    b[0, 0] = np.nan
    b[500, 2] = np.inf
    b[-1] = np.nan
    nan_cloud = np.full((37, 3), np.nan, np.float32)
    none = np.zeros((0, 3), np.float32)
    clouds = [a, b, c, nan_cloud, a, none, c]
    rgbs = [rgb[:900], rgb[900:1900], rgb[1900:], rgb[:37], rgb[:900], rgb[:0], rgb[1900:]]
    kw = dict(min_size=15)
    want = [_alone(p, col, **kw)[0] for p, col in zip(clouds, rgbs)]
    got, _ = _batch(ctx, clouds, rgbs, (sum(len(p) for p in clouds), 0), **kw)
    _same(got, want, "non-finite")
    assert (got[1][0][[0, 500, -1]] == -1).all() and got[1][1] >= 1
    assert (got[3][0] == -1).all() and got[3][1] == 0 and len(got[3][0]) == 37
    assert len(got[5][0]) == 0 and got[5][1] == 0
    # a batch of nothing but such clouds
    got, stats = _batch(ctx, [nan_cloud, none], [rgb[:37], rgb[:0]], (37, 0), **kw)
    _same(got, [want[3], want[5]], "nothing finite")
    assert stats[0] == 0 and stats[1] == 0


@pytest.mark.parametrize("kw,on_route", [(dict(region_nn=3), True), (dict(nn=5, region_nn=100), True), (dict(region_nn=128), True),
                                         (dict(region_nn=129), False)], ids=["region_nn3", "nn5", "region_nn128", "region_nn129"])
def test_neighbour_counts(ctx, fix_scenes, kw, on_route):
    """rows of 3 (one register of the top list), a growing prefix of 5, rows of 128 (both registers full), and rows of 129, which
    the batch kernel does not build: the work handle, same results"""
    pts, rgb = fix_scenes["patches"]
    clouds, rgbs = [pts[:1200], pts[1200:], pts[:150]], [rgb[:1200], rgb[1200:], rgb[:150]]
    kw = dict(min_size=15, **kw)
    want = [_alone(p, c, **kw)[0] for p, c in zip(clouds, rgbs)]
    total = sum(len(p) for p in clouds)
    got, _ = _batch(ctx, clouds, rgbs, (total, 0) if on_route else (0, total), **kw)
    _same(got, want, kw)


def test_routes_give_the_same_results(ctx):
    """PCC_OPT_RGB_BATCH_BRUTE_MAX = 256: clouds of 200 and 256 points keep to the batch kernels, those of 300 and 257 go through
    the work handle, inside one call -- and nothing differs from the call at the default"""
    rng = np.random.default_rng(23)
    sizes = [200, 300, 256, 257]
    clouds = [rng.random((n, 3)).astype(np.float32) * 0.3 for n in sizes]
    rgbs = [(rng.integers(0, 3, (n, 3)) * 20).astype(np.uint8) for n in sizes]
    kw = dict(min_size=5)
    want = [_alone(p, c, **kw)[0] for p, c in zip(clouds, rgbs)]
    default = ctx.get_option(capi.OPT_RGB_BATCH_BRUTE_MAX)
    assert default == 8192
    at_default, _ = _batch(ctx, clouds, rgbs, (sum(sizes), 0), **kw)
    try:
        ctx.set_option(capi.OPT_RGB_BATCH_BRUTE_MAX, 256)
        limited, _ = _batch(ctx, clouds, rgbs, (200 + 256, 300 + 257), **kw)
        ctx.set_option(capi.OPT_RGB_BATCH_BRUTE_MAX, 0)
        none, _ = _batch(ctx, clouds, rgbs, (0, sum(sizes)), **kw)
    finally:
        ctx.set_option(capi.OPT_RGB_BATCH_BRUTE_MAX, default)
    for what, got in (("default", at_default), ("256", limited), ("0", none)):
        _same(got, want, what)


def test_the_context_is_left_as_it_was(gpu, fix_scenes):
    """two different batches on one context; then a context that indexes a cloud of its own and keeps its self k-NN rows
    (PCC_OPT_KNN_CACHE_K = 100): its own region growing and k-NN answer as before the batch; the module-level form"""
    pts, rgb = fix_scenes["patches"]
    noise = fix_scenes["noise"][1]
    kw = dict(min_size=15)
    first = ([pts[:700], pts[700:1500]], [rgb[:700], rgb[700:1500]])
    second = ([pts[1500:], pts[:40], pts[100:400]], [noise[1500:], noise[:40], noise[100:400]])
    want1 = [_alone(p, c, **kw)[0] for p, c in zip(*first)]
    want2 = [_alone(p, c, **kw)[0] for p, c in zip(*second)]
    with capi.Index(np.zeros((1, 3), np.float32)) as one:
        for _ in range(2):
            _same(_batch(one, *first, (1500, 0), **kw)[0], want1, "first")
            _same(_batch(one, *second, (1840, 0), **kw)[0], want2, "second")
    rng = np.random.default_rng(24)
    own = rng.random((20000, 3)).astype(np.float32)
    own_rgb = (rng.integers(0, 3, (20000, 3)) * 20).astype(np.uint8)
    q = own[:500]
    with capi.Index(own) as big:
        big.set_option(capi.OPT_KNN_CACHE_K, 100)
        before = big.region_growing_rgb(own_rgb, **kw)
        ki, kd = big.knn(q, 10)
        _same(_batch(big, *second, (1840, 0), **kw)[0], want2, "own cloud, kept rows")
        after = big.region_growing_rgb(own_rgb, **kw)
        ki2, kd2 = big.knn(q, 10)
    assert before[1] == after[1] and (before[0] == after[0]).all()
    assert (ki == ki2).all() and (kd.view(np.uint32) == kd2.view(np.uint32)).all()
    _same(capi.region_growing_rgb_batch(*first, **kw), want1, "module level, ctx=None")
    assert capi.region_growing_rgb_batch([], []) == []


def _run(exe, *args):
    assert exe.exists(), "make cli"
    out = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


def test_batch_tool_prints_what_the_single_tool_prints(gpu, tmp_path):
    """build/rgb_segments_batch over three PLY files: the output of build/rgb_segments for each, one after the other, from one
    batch call (the middle file below the reference's gate of more than 10 points)"""
    scenes = {name: (pts, rgb, par) for name, pts, rgb, par in _scenes()}
    par = scenes["patches"][2]
    files = []
    for k, (pts, rgb) in enumerate([(scenes["patches"][0][:2500], scenes["patches"][1][:2500]), (scenes["tiny"][0][:9], scenes["tiny"][1][:9]),
                                    (scenes["near"][0][:1500], scenes["near"][1][:1500])]):
        ply = tmp_path / f"c{k}.ply"
        write_ply(ply, pts, rgb)
        files.append(ply)
    single = "".join(_run(ROOT / "build" / "rgb_segments", f, *par) for f in files)
    batch = _run(ROOT / "build" / "rgb_segments_batch", *files, *par)
    assert single.count("segments ") == 3
    assert batch == single


def test_cli_rgb_batch_writes_the_same_report(gpu, tmp_path):
    """examples/comparator_main.cpp --rgb-batch: the colour segmentations of all accepted matches through one
    pcc_region_growing_rgb_batch call before the match sections are written; results file and console output are those of the
    run without the flag, byte for byte"""
    import test_cli_gpu as cli
    a, b = cli._scene(1), cli._scene(2, shift=(0.004, -0.003, 0.002))
    fa, fb = tmp_path / "a.ply", tmp_path / "b.ply"
    write_ply(fa, a, fmt="binary")
    write_ply(fb, b, fmt="binary")
    exe = ROOT / "build" / "comparator"
    assert exe.exists(), "make cli"
    r = subprocess.run([str(exe), "-e", str(fa), str(fb), "--results", str(tmp_path / "r0.txt"), "--dump-clusters", str(tmp_path / "cl")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1
    cen = [[cli._centroid_f32(cli._read_cluster_ply(tmp_path / f"cl_{k}_{j}.ply")) for j in range(4)] for k in (1, 2)]
    twin = [int(np.argmin([np.linalg.norm(cen[0][i] - c2) for c2 in cen[1]])) for i in range(4)]
    rng = np.random.default_rng(9)
    des = [rng.random((10, 32)).astype(np.float32) for _ in range(4)]
    cli._write_descriptors(tmp_path / "d1.txt", {i: des[i] for i in range(4)})
    cli._write_descriptors(tmp_path / "d2.txt", {twin[i]: des[i].copy() for i in range(4)})
    runs = []
    for tag, extra in (("host", []), ("batch", ["--rgb-batch"])):
        res = tmp_path / f"{tag}.txt"
        r = subprocess.run([str(exe), "-e", str(fa), str(fb), "--results", str(res), "--descriptors1", str(tmp_path / "d1.txt"),
                            "--descriptors2", str(tmp_path / "d2.txt")] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 1, r.stderr[-1000:]
        runs.append((res.read_bytes(), r.stdout.replace(str(res), "RESULTS")))
    assert runs[0][0].count(b"color differences") >= 2, "the report must hold matches, or the flag is not exercised"
    assert runs[1][0] == runs[0][0]
    assert runs[1][1] == runs[0][1]
