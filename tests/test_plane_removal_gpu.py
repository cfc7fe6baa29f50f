"""pcc_plane_removal / Index.plane_removal against the loop it replaces (reference src/segmentation.cpp:79-117): the oracle's
RANSAC (oracle.sac_plane) per turn, np.delete between the turns, original indices tracked.  Everything is compared exactly:
index lists, per-plane sizes and iteration counts as integers, coefficients as uint32 views.

The scenes are tests/plane_removal_util.py's; what the oracle loop gives for them (computed on the CPU):
  three planes, 700 points   stop 0.3: 3 planes (255 / 200 / 149), 96 remain;  stop 0.1: 7 planes, 65 remain, four turns of 101
                             iterations (more than one batch of 32 candidates);  stop 0.0: 19 planes, 2 remain, no model at the end
  255 ... 2049-point prefixes of the scene repeated with further seeds: 3 planes each
  every 9th y = NaN          3 planes, 164 remain, the 78 NaN points among them
  3000 resampled (rng(3))    3 planes, 436 remain; the first sample batch of turn 2 holds a degenerate sample"""
import ctypes as C

import numpy as np
import pytest

import oracle
from plane_removal_util import REFUSALS, RawCall, cached_loop, oracle_loop, three_planes
from pointcloudcomparator_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu):
    with capi.Index(np.zeros((1, 3), np.float32)) as ix:
        yield ix


def _same(got, want):
    rem, pop, coeff, sizes, its, ended = got[:6]
    w_rem, w_pop, w_coeff, w_sizes, w_its, w_ended = want[:6]
    rem, pop = (a.cpu().numpy() if capi._is_torch(a) else a for a in (rem, pop))
    np.testing.assert_array_equal(sizes, w_sizes)
    np.testing.assert_array_equal(its, w_its)
    assert coeff.shape == w_coeff.shape and (coeff.view(np.uint32) == w_coeff.view(np.uint32)).all(), (coeff, w_coeff)
    np.testing.assert_array_equal(rem, w_rem)
    np.testing.assert_array_equal(pop, w_pop)
    assert ended == w_ended


# (scene, stop_fraction, first points or None, planes, remaining, ended_without_model): the last three are the oracle's
CASES = [
    ("three", 0.3, None, 3, 96, False),
    ("three", 0.1, None, 7, 65, False),
    ("three", 0.0, None, 19, 2, True),
    ("three", 1.0, None, 0, 700, False),
    ("long", 0.3, 255, 3, 41, False),
    ("long", 0.3, 256, 3, 41, False),
    ("long", 0.3, 257, 3, 41, False),
    ("long", 0.3, 1024, 3, 146, False),
    ("long", 0.3, 1025, 3, 146, False),
    ("long", 0.3, 2047, 3, 280, False),
    ("long", 0.3, 2048, 3, 280, False),
    ("long", 0.3, 2049, 3, 280, False),
    ("lattice", 0.0, None, 1, 0, False),
    ("three", 0.3, 2, 0, 2, True),
    ("three", 0.3, 0, 0, 0, False),
    ("nans", 0.3, None, 3, 164, False),
]


@pytest.mark.parametrize("scene,stop,head,planes,remain,ended", CASES)
def test_plane_removal_matches_the_oracle_loop(ctx, scene, stop, head, planes, remain, ended):
    pts, want = cached_loop(scene, stop, head)
    assert (len(want[3]), len(want[0]), want[5]) == (planes, remain, ended)  # the oracle's own result, as recorded above
    got = ctx.plane_removal(pts, stop_fraction=stop, max_planes=0 if planes == 0 and not ended else 64)
    _same(got, want)
    assert ctx.stats()[0] == planes
    if scene == "three" and stop == 0.1:
        assert (want[4] > 32).sum() >= 2  # turns that need more than one batch of candidates
    if scene == "nans":
        assert np.isin(np.arange(0, 700, 9), got[0]).all() and (got[1][::9] == -1).all()
    if scene == "lattice":
        assert want[3][0] == 49
    # host memory, no duplicate point: no turn takes a host copy (turn 0 reads the caller's own array)
    if scene in ("three", "long"):
        assert ctx.stats()[1] == 0


def test_plane_removal_in_device_memory(ctx):
    import torch
    for scene, stop, head in (("three", 0.3, None), ("three", 0.1, None), ("long", 0.3, 1025), ("nans", 0.3, None), ("three", 0.3, 2),
                              ("three", 1.0, None), ("three", 0.3, 0), ("lattice", 0.0, None)):
        pts, want = cached_loop(scene, stop, head)
        got = ctx.plane_removal(torch.from_numpy(pts).cuda(), stop_fraction=stop)
        assert got[0].is_cuda and got[1].is_cuda
        _same(got, want)
        assert not any(want[6])  # (the replay of every turn's first batch, and no duplicate point: no degenerate sample)
        assert ctx.stats()[:2] == [len(want[3]), 0]


def test_plane_removal_retries_a_degenerate_turn_on_the_compacted_cloud(ctx):
    """3000 points drawn with repetition from the 700 (rng(3)): samples with p1 == p0 are degenerate, PCL redraws them at once and
    the gathered form cannot.  plane_removal_util.first_batch_degenerate replays the first 32 samples of every turn: turn 2 of
    this scene holds one (turns 0 and 1 do not), so the retry runs on a cloud compacted twice on the device."""
    import torch
    pts, want = cached_loop("dup", 0.3)
    assert len(want[3]) == 3 and len(want[0]) == 436
    assert want[6] == [False, False, True]
    got = ctx.plane_removal(torch.from_numpy(pts).cuda())
    _same(got, want)
    assert ctx.stats()[1] >= sum(want[6]) >= 1
    _same(ctx.plane_removal(pts), want)  # host memory: turn 0 from the caller's array, the later turns as above


def test_plane_removal_records_and_memory_spaces(ctx):
    import torch
    xyz, want = cached_loop("three", 0.3)
    rec = np.zeros((len(xyz), 8), np.float32)
    rec[:, :3] = xyz
    rec[:, 4] = np.random.default_rng(1).integers(0, 1 << 24, len(xyz), dtype=np.uint32).view(np.float32)  # colour words
    rec[:, 5:] = np.random.default_rng(0).random((len(xyz), 3), dtype=np.float32)
    results = {}
    for record_bytes in (32, 16):
        for space, arg in (("host", rec), ("device", torch.from_numpy(rec).cuda())):
            got = ctx.plane_removal(arg, with_points=True, record_bytes=record_bytes)
            _same(got, want)
            points = got[6].cpu().numpy() if space == "device" else got[6]
            assert points.shape == (len(want[0]), record_bytes // 4)
            assert (points.view(np.uint32) == rec[want[0], :record_bytes // 4].view(np.uint32)).all()
            results[(record_bytes, space)] = points
        assert (results[(record_bytes, "host")].view(np.uint32) == results[(record_bytes, "device")].view(np.uint32)).all()
    # 12-byte records of a 12-byte cloud (the 4-byte path of the gather), and a view whose rows are not 16-byte aligned
    got = ctx.plane_removal(torch.from_numpy(xyz).cuda(), with_points=True)
    assert (got[6].cpu().numpy().view(np.uint32) == xyz[want[0]].view(np.uint32)).all()
    shifted = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), rec.reshape(-1)])).cuda()[1:].view(-1, 8)
    got = ctx.plane_removal(shifted, with_points=True)
    _same(got, want)
    assert (got[6].cpu().numpy().view(np.uint32) == rec[want[0]].view(np.uint32)).all()


def test_plane_removal_overflow_keeps_the_planes_found(ctx):
    pts, want = cached_loop("three", 0.3)
    with pytest.raises(capi.PccError) as e:
        ctx.plane_removal(pts, max_planes=1)
    assert e.value.status == -6  # PCC_ERR_OVERFLOW
    coeff, sizes, its, n_remaining = e.value.partial
    assert len(sizes) == 1 and sizes[0] == want[3][0] and its[0] == want[4][0]
    assert (coeff.view(np.uint32) == want[2][:1].view(np.uint32)).all()
    assert n_remaining == len(pts) - want[3][0]
    with pytest.raises(capi.PccError) as e:  # a turn is due and there is room for none
        ctx.plane_removal(pts, max_planes=0)
    assert e.value.status == -6 and len(e.value.partial[1]) == 0 and e.value.partial[3] == len(pts)


def test_plane_removal_feeds_the_clustering_on_the_device(ctx):
    """plane removal -> set_input -> clusters without the cloud leaving the device: the points the call leaves are what
    pcc_index_set_input takes next.  The 700-point scene as it is (its clutter is too sparse for a cluster of 10), and with three
    blobs of 40 points that the planes leave behind as clusters."""
    import torch
    rng = np.random.default_rng(5)
    blobs = np.concatenate([rng.normal(c, 0.02, (40, 3)) for c in ((0.5, 0.5, 1.0), (2.0, 1.0, 1.5), (1.0, 2.5, 2.0))]).astype(np.float32)
    with_blobs = np.concatenate([three_planes(1), blobs])
    with_blobs = np.ascontiguousarray(with_blobs[rng.permutation(len(with_blobs))])
    for pts, least in ((three_planes(1), 0), (with_blobs, 3)):
        want = oracle_loop(pts, 0.3)
        got = ctx.plane_removal(torch.from_numpy(pts).cuda(), with_points=True)
        _same(got, want)
        rest = got[6]
        assert rest.is_cuda and rest.shape == (len(want[0]), 3)
        with capi.Index(rest) as ix:
            labels, ncl, sizes = ix.euclidean_clusters(0.05, 10, 250000, device_out=rest)
        w_labels, w_ncl, w_sizes = oracle.euclidean_clusters(np.ascontiguousarray(pts[want[0]]), 0.05, 10, 250000)
        assert ncl == w_ncl and ncl >= least
        np.testing.assert_array_equal(labels.cpu().numpy(), w_labels)
        np.testing.assert_array_equal(sizes, w_sizes)


def test_plane_removal_on_the_references_own_shape(ctx):
    """the 33 000-point two-plane scene of test_sac_gpu.test_plane_removal_loop_like_the_reference"""
    import torch
    pts, want = cached_loop("room", 0.3)
    assert len(want[3]) == 2 and len(want[0]) < 0.3 * len(pts)
    _same(ctx.plane_removal(pts), want)
    _same(ctx.plane_removal(torch.from_numpy(pts).cuda()), want)


def test_plane_removal_refusals_write_nothing(ctx):
    call = RawCall()
    for kw, status in REFUSALS:
        assert call(ctx._h, **kw) == status, kw
        assert call.untouched(), kw
        assert capi.LIB.pcc_last_error()
    # what pcc_sac_plane says for the same fault
    inl, cnt, coeff = np.zeros(8, np.int32), C.c_size_t(0), np.zeros(4, np.float32)
    for kw in (dict(stride=10), dict(prob=1.0)):
        assert call(ctx._h, **kw) == -1
        mine = capi.LIB.pcc_last_error()
        assert capi.LIB.pcc_sac_plane(ctx._h, call.pts.ctypes.data, 8, kw.get("stride", 32), 0, 100, 0.02, kw.get("prob", 0.99), 1,
                                      inl.ctypes.data, C.byref(cnt), coeff.ctypes.data, None) == -1
        assert capi.LIB.pcc_last_error() == mine
    # nullable outputs left out: the counts alone
    assert call(ctx._h, its=None, ended=None, pop=None, rem=None, points=None, stop=1.0, max_planes=0, coeff=None, sizes=None) == 0
    assert call.out["n_planes"][0] == 0 and call.out["n_rem"][0] == 8
