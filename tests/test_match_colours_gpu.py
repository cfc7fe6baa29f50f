"""pcc_match_colour_elements on the GPU (csrc/match_colour.hip; reference src/comparator.cpp:1379-1509 calling
src/segmentation.cpp:161-216 twice per accepted match): the table of Index.match_colour_elements against the restatement of
the loop's counting (tests/match_colours_util.py) fed, per cluster, the count of the single call on a FRESH index over that
cluster alone -- and in the first test the oracle's over a fresh index's rows as well.  Integers, no tolerance.  The parity
tests run the growing stage alone (min_size = 1, region_colour = 0: the clusters are the grown segments) unless they say
otherwise, and assert first that the expected counts hold at least two different values above 1."""
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle
from pointcloudcomparator_amd import capi

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import match_colours_util as mcu  # noqa: E402
import rgb_device_util as util  # noqa: E402
from match_colours_util import RB_TILE  # noqa: E402
from test_rgb_gpu import _scenes  # noqa: E402

pytestmark = pytest.mark.gpu

GROW = dict(min_size=1, region_colour=0.0)


def _single(pts, rgb, **kw):
    """the cluster alone, past the gate: the count of the single call on a fresh handle"""
    with capi.Index(np.ascontiguousarray(pts, np.float32)) as ix:
        return ix.region_growing_rgb(rgb, **kw)[1]


def _oracle(pts, rgb, **kw):
    """the same from the oracle's restatement over the rows of a fresh index over the NaN-stripped cluster (as _alone in
    tests/test_rgb_batch_gpu.py)"""
    pts = np.ascontiguousarray(pts, np.float32)
    keep = np.isfinite(pts).all(1)
    fp, frgb = np.ascontiguousarray(pts[keep]), rgb[keep]
    with capi.Index(fp) as ix:
        ki, kd = ix.knn(fp, min(kw.get("region_nn", 100), len(fp)))
    return oracle.region_growing_rgb(fp, frgb, neighbours=ki, neighbour_d2=kd, **kw)[1]


def _expected(scene1, scene2, matches, count_of=_single, min_points=10, **kw):
    table, distinct, saved = mcu.restate(scene1, scene2, matches, lambda p, c: count_of(p, c, **kw), min_points)
    return table, distinct, saved


def _varied(table):
    values = {int(v) for v in np.asarray(table).reshape(-1) if v > 1}
    assert len(values) >= 2, f"the expected counts must hold two different values above 1: {sorted(values)}"


def _call(ctx, scene1, scene2, matches, device=False, **kw):
    rec1, off1 = mcu.records(scene1)
    rec2, off2 = mcu.records(scene2)
    if device:
        import torch
        rec1, rec2 = torch.from_numpy(rec1).cuda(), torch.from_numpy(rec2).cuda()
    got = ctx.match_colour_elements(rec1, off1, rec2, off2, matches, **kw)
    assert got.dtype == np.int32 and got.shape == (len(matches), 2)
    return got, ctx.stats()


def _points_on_routes(scene1, scene2, matches, limit):
    """(points through the batch kernels, points through the work handle) of the distinct clusters the table names"""
    named = {(0, i) for i, j in enumerate(matches) if j >= 0} | {(1, int(j)) for j in matches if j >= 0}
    sizes = [len((scene2 if s else scene1)[c][0]) for s, c in named]
    return sum(n for n in sizes if n <= limit), sum(n for n in sizes if n > limit)


@pytest.fixture(scope="module")
def ctx(gpu):
    with capi.Index(np.zeros((1, 3), np.float32)) as ix:
        yield ix


@pytest.fixture(scope="module")
def mixed(gpu):
    fix = {name: (pts, rgb) for name, pts, rgb in util.fixpoint_scenes()}
    room = next(s for s in _scenes() if s[0] == "room")
    scene1, scene2, matches = mcu.mixed_scenes(fix, (room[1], room[2]))
    assert max(len(p) for p, _ in scene1 + scene2) <= 3000 and len(scene1) == len(scene2) == 6 and (matches == -1).sum() == 2
    want, distinct, saved = _expected(scene1, scene2, matches, **GROW)
    _varied(want)
    return scene1, scene2, matches, want, distinct, saved


@pytest.fixture(scope="module")
def sizes(gpu):
    scene1, scene2, matches = mcu.size_scenes()
    want, distinct, saved = _expected(scene1, scene2, matches, **GROW)
    _varied(want)
    return scene1, scene2, matches, want, distinct, saved


def test_mixed_scenes(ctx, mixed):
    """two scenes of six clusters, two rows without a match: against the single call and the oracle, growing alone and with the
    reference's parameters"""
    scene1, scene2, matches, want, distinct, saved = mixed
    from_oracle, _, _ = _expected(scene1, scene2, matches, count_of=_oracle, **GROW)
    assert (from_oracle == want).all(), "the single call differs from the oracle"
    got, stats = _call(ctx, scene1, scene2, matches, **GROW)
    assert (got == want).all(), (got.tolist(), want.tolist())
    assert (got[matches == -1] == -1).all() and (got[matches >= 0] >= 0).all()
    assert (stats[2], stats[3]) == _points_on_routes(scene1, scene2, matches, 8192) and stats[3] == 0
    assert (stats[4], stats[5]) == (distinct, saved) == (8, 0)
    assert stats[0] == got[matches >= 0].sum() and stats[7] >= 1            # (growing alone: every segment is a colour element)
    reference, _, _ = _expected(scene1, scene2, matches)
    by_oracle, _, _ = _expected(scene1, scene2, matches, count_of=_oracle)
    assert (by_oracle == reference).all()
    got, _ = _call(ctx, scene1, scene2, matches)
    assert (got == reference).all(), (got.tolist(), reference.tolist())
    assert reference[3, 0] == 0                                               # (the 20-point cluster: no segment of 200)


def test_sizes_where_the_pack_and_row_kernels_can_go_wrong(ctx, sizes):
    """11 ... RB_TILE + 1 points, an empty cluster between two others in either scene, seven clusters against six"""
    scene1, scene2, matches, want, distinct, saved = sizes
    assert len(scene1) != len(scene2)
    got, stats = _call(ctx, scene1, scene2, matches, **GROW)
    assert (got == want).all(), (got.tolist(), want.tolist())
    assert got[2].tolist() == [0, 0]                                          # the two empty clusters
    assert (stats[2], stats[3]) == _points_on_routes(scene1, scene2, matches, 8192)
    assert (stats[4], stats[5]) == (distinct, saved) == (13, 1)


def test_the_gate(ctx):
    """more than min_points FINITE points: 13 with 3 NaNs is below it, 14 with 3 NaNs above; nothing but NaNs is 0, not
    PCC_ERR_EMPTY; min_points = 0 lets an 11-point cluster and everything else with a finite point through"""
    rng = np.random.default_rng(32)

    def with_nans(n, bad):
        pts, rgb = mcu.two_level_cloud(rng, n)
        pts[rng.permutation(n)[:bad]] = np.nan
        return pts, rgb

    scene1 = [with_nans(13, 3), with_nans(14, 3), (np.full((40, 3), np.nan, np.float32), mcu.two_level_cloud(rng, 40)[1]), mcu.two_level_cloud(rng, 11),
              mcu.two_level_cloud(rng, 300)]
    scene2 = [mcu.two_level_cloud(rng, 10), with_nans(200, 50), mcu.two_level_cloud(rng, 150)]
    matches = np.array([0, 1, 2, 0, 1], np.int32)
    want, _, _ = _expected(scene1, scene2, matches, **GROW)
    _varied(want)
    assert want[0].tolist() == [0, 0] and want[1, 0] == _single(*scene1[1], **GROW) > 0 and want[2, 0] == 0 and want[3, 0] > 1
    got, _ = _call(ctx, scene1, scene2, matches, **GROW)
    assert (got == want).all(), (got.tolist(), want.tolist())
    want0, _, _ = _expected(scene1, scene2, matches, min_points=0, **GROW)
    assert want0[0, 0] == _single(*scene1[0], **GROW) > 0 and want0[0, 1] > 0 and want0[2, 0] == 0
    got0, _ = _call(ctx, scene1, scene2, matches, min_points=0, **GROW)
    assert (got0 == want0).all(), (got0.tolist(), want0.tolist())
    # one 11-point cluster on its own, gates 0, 10 and 11
    pair = ([scene1[3]], [scene1[3]], np.array([0], np.int32))
    count = _single(*scene1[3], **GROW)
    for gate, value in ((0, count), (10, count), (11, 0)):
        assert _call(ctx, *pair, min_points=gate, **GROW)[0].tolist() == [[value, value]]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_nothing_but_empty_clusters(ctx, device):
    """every named cluster is empty: zeros from a call that has nothing to pack; then one real cluster against an empty one"""
    rng = np.random.default_rng(34)
    none = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))
    got, stats = _call(ctx, [none, none], [none], np.array([0, 0], np.int32), device=device, **GROW)
    assert got.tolist() == [[0, 0], [0, 0]] and (stats[2], stats[3], stats[4], stats[5]) == (0, 0, 3, 1)
    some = mcu.two_level_cloud(rng, 90)
    got, stats = _call(ctx, [none, some], [none, none], np.array([1, 0], np.int32), device=device, **GROW)
    assert got.tolist() == [[0, 0], [_single(*some, **GROW), 0]] and got[1, 0] > 1 and (stats[2], stats[4]) == (90, 4)


def test_deduplication(ctx, mixed):
    """matches = [2, 2, -1, 0]: cluster 2 of scene 2 is segmented once and both rows get its count"""
    scene1, scene2 = mixed[0][:4], mixed[1][:3]
    matches = np.array([2, 2, -1, 0], np.int32)
    want, distinct, saved = _expected(scene1, scene2, matches, **GROW)
    _varied(want)
    got, stats = _call(ctx, scene1, scene2, matches, **GROW)
    assert (got == want).all(), (got.tolist(), want.tolist())
    assert got[0, 1] == got[1, 1] and got[2].tolist() == [-1, -1]
    assert (stats[4], stats[5]) == (5, 1) == (distinct, saved)
    named = [scene1[0], scene1[1], scene1[3], scene2[2], scene2[0]]
    assert stats[2] == sum(len(p) for p, _ in named) and stats[3] == 0       # (the repeated cluster's points count once)


def test_memory_spaces_and_layouts(ctx, mixed):
    """the same table from NumPy records, from torch device records, and from 16-byte points with 4-byte colour words of their
    own in either memory space"""
    import torch
    scene1, scene2, matches, want = mixed[:4]
    host, _ = _call(ctx, scene1, scene2, matches, **GROW)
    device, _ = _call(ctx, scene1, scene2, matches, device=True, **GROW)
    p1, w1, off1 = mcu.separate(scene1)
    p2, w2, off2 = mcu.separate(scene2)
    apart = ctx.match_colour_elements(p1, off1, p2, off2, matches, rgb1=w1, rgb2=w2, **GROW)
    dev = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    apart_device = ctx.match_colour_elements(dev(p1), off1, dev(p2), off2, matches, rgb1=dev(w1), rgb2=dev(w2), **GROW)
    # 12-byte points (no vector load) with (n, 3) uint8 colours
    xyz = ctx.match_colour_elements(np.ascontiguousarray(p1[:, :3]), off1, np.ascontiguousarray(p2[:, :3]), off2, matches,
                                    rgb1=np.concatenate([c for _, c in scene1]), rgb2=np.concatenate([c for _, c in scene2]), **GROW)
    for what, got in (("host", host), ("device", device), ("separate arrays", apart), ("separate arrays, device", apart_device), ("xyz", xyz)):
        assert (got == want).all(), (what, got.tolist(), want.tolist())


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_routes(ctx, sizes, device):
    """PCC_OPT_RGB_BATCH_BRUTE_MAX = 256: the clusters above 256 points go through the work handle; nr_region_neighbours = 129:
    every cluster does; the table is the batch route's"""
    scene1, scene2, matches, want = sizes[:4]
    default = ctx.get_option(capi.OPT_RGB_BATCH_BRUTE_MAX)
    assert default == 8192
    try:
        ctx.set_option(capi.OPT_RGB_BATCH_BRUTE_MAX, 256)
        got, stats = _call(ctx, scene1, scene2, matches, device=device, **GROW)
    finally:
        ctx.set_option(capi.OPT_RGB_BATCH_BRUTE_MAX, default)
    assert (got == want).all(), (got.tolist(), want.tolist())
    small = 11 + 12 + 63 + 64 + 65 + 255 + 256
    large = 257 + RB_TILE - 1 + RB_TILE + RB_TILE + 1
    assert (stats[2], stats[3]) == (small, large) == _points_on_routes(scene1, scene2, matches, 256)
    want129, _, _ = _expected(scene1, scene2, matches, region_nn=129, **GROW)
    got, stats = _call(ctx, scene1, scene2, matches, device=device, region_nn=129, **GROW)
    assert (got == want129).all(), (got.tolist(), want129.tolist())
    assert (stats[2], stats[3]) == (0, small + large) and (stats[0], stats[1], stats[7]) == (0, 0, 0)
    assert (want129 == want).all()                                            # (growing alone reads the first 30 entries of a row)


def test_one_handle_several_calls(gpu, sizes, mixed):
    """the larger call, then the smaller one, on one handle; then the batch call and the single call through the same handle:
    every result is what a fresh handle gives"""
    rng = np.random.default_rng(33)
    pts, rgb = mcu.two_level_cloud(rng, 700)
    with capi.Index(pts) as fresh:
        single = fresh.region_growing_rgb(rgb, **GROW)
    with capi.Index(np.zeros((1, 3), np.float32)) as fresh:
        batch = fresh.region_growing_rgb_batch([pts, pts[:300]], [rgb, rgb[:300]], **GROW)
    assert single[1] > 1
    with capi.Index(pts) as one:
        for _ in range(2):
            assert (_call(one, *sizes[:3], **GROW)[0] == sizes[3]).all()
            assert (_call(one, *mixed[:3], **GROW)[0] == mixed[3]).all()
            assert (_call(one, *mixed[:3], device=True, **GROW)[0] == mixed[3]).all()
        again = one.region_growing_rgb_batch([pts, pts[:300]], [rgb, rgb[:300]], **GROW)
        for (gl, gn), (wl, wn) in zip(again, batch):
            assert gn == wn and (gl == wl).all()
        own = one.region_growing_rgb(rgb, **GROW)                             # (the cloud the handle indexes is as it was)
        assert own[1] == single[1] and (own[0] == single[0]).all()
        assert (_call(one, *mixed[:3], **GROW)[0] == mixed[3]).all()
