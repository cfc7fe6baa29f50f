"""The radius search (knn.hip grid_radius and its kernels) where its kernels change form: EVERY row of EVERY query of the scenes of
tests/radius_forms_util.py -- rows of exactly 64, 128, 256 and 512 neighbours and one either side, calls whose mean row is just
on either side of the wave fill's threshold, rows of equal distances that overfill a bucket of the LDS sort, balls of 8 and 9
rows a layer, of 121 rows and more, chunks beyond the flat walk's candidates, counts on either side of the count's choice, waves
that take a second and a third query -- against the exhaustive reference of that file: indices equal, distances equal as uint32,
no tolerance.  tests/test_radius_forms_cpu.py pins that every scene still reaches its threshold; which route a call took cannot
be observed.  The model's grid is held against the handle's cell count wherever a handle is made (PCC_OPT_GRID_TRIM = 0: the model
is that of the untrimmed box)."""
import ctypes as C

import numpy as np
import pytest

import oracle
import radius_forms_util as u
from option_parity_util import FILL_D2_BITS, FILL_IDX, bits, filled, to_numpy

pytestmark = pytest.mark.gpu

NONE_IDX, INF_BITS = np.int32(-1), np.uint32(0x7F800000)


def _index(name, radius=None):
    """a handle over the scene's references with the model's grid"""
    from pointcloudcomparator_amd import capi
    sc = u.scene(name)
    ix = capi.Index(sc.ref, engine=capi.ENGINE_GRID)
    ix.set_option(capi.OPT_GRID_TRIM, 0)
    ix.set_option(capi.OPT_GRID_PPC, sc.ppc)
    ix.set_input(sc.ref)
    want = u.model_of(name, sc.radii[0] if radius is None else radius).ncells
    assert ix.stats()[3] == want, (name, "the model's grid is not the handle's", ix.stats()[3], want)
    return ix


def _by_key(offsets, idx, d2):
    """every row ordered by (d2 bits, index) on the host"""
    row = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    order = np.lexsort((idx, bits(d2), row))
    return idx[order], d2[order]


def _assert_rows(got, want, what, in_order=True):
    offsets, idx, d2 = (to_numpy(a) for a in got)
    w_off, w_idx, w_d2 = want
    assert (offsets == w_off).all(), (what, "offsets differ at queries", np.flatnonzero(np.diff(offsets) != np.diff(w_off))[:5])
    assert len(idx) == len(w_idx) and len(d2) == len(w_d2), what
    if not in_order:
        idx, d2 = _by_key(offsets, idx, d2)
    bad = (idx != w_idx) | (bits(d2) != bits(w_d2))
    if bad.any():
        q = np.searchsorted(w_off, np.flatnonzero(bad)[:5], side="right") - 1
        raise AssertionError((what, "rows differ", int(bad.sum()), "entries; first queries", q.tolist(), "of lengths", np.diff(w_off)[q].tolist()))


def _assert_counts(got, want_offsets, what):
    got = to_numpy(got)
    bad = np.flatnonzero(got != np.diff(want_offsets))
    assert len(bad) == 0, (what, "counts differ at queries", bad[:5].tolist(), got[bad[:5]].tolist(), np.diff(want_offsets)[bad[:5]].tolist())


def _fill(ix, qry, radius, offsets, sorted_=True, want_idx=True, want_d2=True):
    """pcc_radius_fill itself (host memory) into sentinel-filled arrays; a pointer not wanted is null"""
    from pointcloudcomparator_amd import capi
    ptr, n, stride, mem = capi._points(qry)
    offs = np.ascontiguousarray(offsets, dtype=np.int64)
    idx, d2 = filled((int(offs[-1]),))
    capi._check(capi.LIB.pcc_radius_fill(ix._h, ptr, n, stride, mem, C.c_double(radius), int(sorted_), offs.ctypes.data,
                                         idx.ctypes.data if want_idx else None, d2.ctypes.data if want_d2 else None))
    return idx, d2


@pytest.mark.parametrize("name,radius", u.CASES)
def test_every_row_of_every_query(gpu, name, radius):
    """count, sorted and unsorted search, queries in host and in device memory"""
    import torch
    sc, want = u.scene(name), u.reference_of(name, radius)
    what = (name, radius)
    with _index(name, radius) as ix:
        _assert_counts(ix.radius_count(sc.qry, radius), want[0], what + ("count",))
        _assert_rows(ix.radius_search(sc.qry, radius, sorted=True), want, what + ("sorted",))
        _assert_rows(ix.radius_search(sc.qry, radius, sorted=False), want, what + ("unsorted",), in_order=False)
        dq = torch.from_numpy(np.array(sc.qry)).to("cuda:0")
        cnt = ix.radius_count(dq, radius)
        assert cnt.is_cuda
        _assert_counts(cnt, want[0], what + ("count, device memory",))
        _assert_rows(ix.radius_search(dq, radius, sorted=True), want, what + ("sorted, device memory",))
        _assert_rows(ix.radius_search(dq, radius, sorted=False), want, what + ("unsorted, device memory",), in_order=False)
    assert (np.diff(want[0])[~np.isfinite(sc.qry).all(1)] == 0).all()


def test_ladder_rows_are_the_same_on_either_side_of_the_mean(gpu):
    """the same rungs through the wave fill (fused delivery) and through lane fill, memset, k_sort_rows, unpack"""
    long_, short = u.scene("ladder:long"), u.scene("ladder:short")
    assert u.model_of("ladder:long", u.R).wave_fill and not u.model_of("ladder:short", u.R).wave_fill
    with _index("ladder:long") as ix:
        for sorted_ in (True, False):
            a = [to_numpy(x) for x in ix.radius_search(long_.qry, u.R, sorted=sorted_)]
            b = [to_numpy(x) for x in ix.radius_search(short.qry, u.R, sorted=sorted_)]
            n = len(long_.qry)
            assert (a[0] == b[0][:n + 1]).all() and b[0][-1] == a[0][-1]
            if not sorted_:
                a[1], a[2] = _by_key(*a)
                b[1], b[2] = _by_key(*b)
            assert (a[1] == b[1]).all() and (bits(a[2]) == bits(b[2])).all(), ("sorted" if sorted_ else "unsorted")


@pytest.mark.parametrize("name,radius", [("ladder:long", u.R), ("ladder:short", u.R), ("ties", u.R), ("boxes", 0.30)])
def test_fill_with_one_of_the_two_arrays(gpu, name, radius):
    """pcc_radius_fill with idx alone and with d2 alone (Out::stage leaves a null pointer null, every kernel asks before it
    writes): the one array as with both, the other untouched"""
    sc, (offsets, w_idx, w_d2) = u.scene(name), u.reference_of(name, radius)
    with _index(name, radius) as ix:
        idx, d2 = _fill(ix, sc.qry, radius, offsets, want_d2=False)
        assert (idx == w_idx).all() and (bits(d2) == FILL_D2_BITS).all(), (name, "idx alone")
        idx, d2 = _fill(ix, sc.qry, radius, offsets, want_idx=False)
        assert (bits(d2) == bits(w_d2)).all() and (idx == FILL_IDX).all(), (name, "d2 alone")
        idx, d2 = _fill(ix, sc.qry, radius, offsets)
        assert (idx == w_idx).all() and (bits(d2) == bits(w_d2)).all(), (name, "both")


def _roomy(hits, nq_min):
    """slots for every row: a few more than its hits, straddling the steps of the fill (a 255-hit row gets 260, a 257-hit row 270);
    every seventh empty row gets three; and a query count (> nq_min, no multiple of 4) with RAD_WAVE_MEAN * nq beyond those slots"""
    extra = {0: 3, 24: 1, 63: 2, 64: 1, 65: 4, 127: 3, 128: 2, 255: 5, 256: 10, 257: 13, 511: 3, 512: 1, 513: 2, 1023: 2, 1025: 7}
    slots = np.array([h + extra.get(int(h), 0) if h or i % 7 == 0 else 0 for i, h in enumerate(hits)], np.int64)
    nq = max(nq_min + 1, int(slots.sum()) // u.RAD_WAVE_MEAN + 1)
    nq += nq % 4 == 0
    return slots, nq


@pytest.mark.parametrize("side", ["wave", "lane"])
def test_offsets_that_promise_more_than_the_balls_hold(gpu, side):
    """every row's hits in order, then -1 / +inf to the end of its slots; the slots in all exactly RAD_WAVE_MEAN * nq (the
    wave fill: rows of up to 256 SLOTS in LDS, a 255-hit row of 260 slots left as keys) and one fewer (lane fill over the memset)"""
    sc, (w_off, w_idx, w_d2) = u.scene("ladder:short"), u.reference_of("ladder:short", u.R)
    slots, nq = _roomy(np.diff(w_off), len(sc.qry))
    far = sc.qry[len(u.scene("ladder:long").qry):]                       # far queries again: rows of no hits, no slots but the last's
    qry = np.ascontiguousarray(np.concatenate([sc.qry, np.resize(far, (nq - len(sc.qry), 3))]))
    slots = np.concatenate([slots, np.zeros(nq - len(sc.qry), np.int64)])
    slots[-1] = u.RAD_WAVE_MEAN * nq - slots.sum() - (side == "lane")
    assert slots[-1] >= 0 and nq % 4 != 0 and (slots.sum() >= u.RAD_WAVE_MEAN * nq) == (side == "wave")
    offsets = np.concatenate([[0], np.cumsum(slots)])
    hits = np.concatenate([np.diff(w_off), np.zeros(nq - len(sc.qry), np.int64)])
    want_idx, want_d2 = np.full(offsets[-1], NONE_IDX), np.full(offsets[-1], np.inf, np.float32)
    at = np.repeat(offsets[:-1] - np.concatenate([w_off[:-1], np.full(nq - len(sc.qry), w_off[-1])]), hits) + np.arange(w_off[-1])
    want_idx[at], want_d2[at] = w_idx, w_d2
    with _index("ladder:short") as ix:
        for sorted_ in (True, False):
            idx, d2 = _fill(ix, qry, u.R, offsets, sorted_=sorted_)
            if not sorted_:                                              # (the empty slots are the largest keys of their row)
                idx, d2 = _by_key(offsets, idx.view(np.uint32), d2)
                idx = idx.view(np.int32)
            bad = (idx != want_idx) | (bits(d2) != bits(want_d2))
            q = np.searchsorted(offsets, np.flatnonzero(bad)[:5], side="right") - 1
            assert not bad.any(), (side, sorted_, "rows differ at queries", q.tolist(), "hits", hits[q].tolist(), "slots", slots[q].tolist())


def _assert_normals(got, want, tie_free, what):
    """the acceptance of test_normals_gpu.py test_normals_with_radius_search; and every row without two neighbours at one
    distance has one order only: its bits are the oracle's"""
    assert (np.isnan(got).all(1) == np.isnan(want).all(1)).all(), what
    ok = ~(np.isnan(got).all(1) & np.isnan(want).all(1))
    same = (got.view(np.uint32) == want.view(np.uint32)).all(axis=1)
    assert same[ok].mean() > 0.99, what
    dots = np.abs((got[ok, :3].astype(np.float64) * want[ok, :3]).sum(1))
    assert (dots > 1 - 1e-5).all(), what
    np.testing.assert_allclose(got[ok, 3], want[ok, 3], rtol=0, atol=1e-6)
    assert same[ok & tie_free].all(), (what, "rows without a tie differ", np.flatnonzero(ok & tie_free & ~same)[:5].tolist())


@pytest.mark.parametrize("cloud", ["ladder", "boxes", "long"])
def test_normals_radius_takes_the_keys_route_without_fusion(gpu, cloud):
    """normals.hip radius_csr: the wave fill without the caller's arrays, then k_sort_rows over EVERY row (sort_row<1, 2, 4, 8>,
    sort_long_row): the self rows of the ladder's clusters, of the boxes cloud at r = 0.30 (rows to 720), and of a cloud where no
    two neighbours of a point tie -- there every row's normal is the oracle's, bit for bit"""
    from pointcloudcomparator_amd import capi
    pts, radius = {"ladder": (u.scene("ladder:long").ref, u.R), "boxes": (u.scene("boxes").ref, 0.30),
                   "long": (u.normals_long_cloud(), u.NORMALS_LONG_RADIUS)}[cloud]
    offsets, _, d2 = u.reference(pts, pts, radius)
    tie_free = np.ones(len(pts), bool)
    tie_free[u.rows_with_ties(offsets, d2)] = False
    assert tie_free.mean() > 0.99 and (cloud != "long" or tie_free.all())
    with capi.Index(pts, engine=capi.ENGINE_GRID) as ix:
        got = ix.normals_radius(radius)
    want = oracle.normals_radius(pts, radius)
    assert np.isfinite(got).all(1).sum() > 0.9 * len(pts)
    _assert_normals(got, want, tie_free, cloud)


def test_one_handle_long_rows_short_rows_and_another_cloud(gpu):
    """calls in sequence on one handle: long rows, short rows, long rows again (knn_fb, out_packed and the kept count of occupied
    cells are reused); then another cloud with another filling under the same radius: the count changes form with it"""
    boxes, ladder = u.scene("boxes"), u.scene("ladder:short")
    assert not u.model_of("boxes", 0.105).count_by_wave
    on_ladder = u.reference(ladder.ref, boxes.qry, 0.105)
    assert u.model(ladder.ref, boxes.qry, 0.105, rows=on_ladder, per_query=False).count_by_wave
    with _index("boxes") as ix:
        for radius in (0.45, 0.10, 0.45, 0.105):
            want = u.reference_of("boxes", radius)
            _assert_counts(ix.radius_count(boxes.qry, radius), want[0], ("boxes", radius, "count"))
            _assert_rows(ix.radius_search(boxes.qry, radius), want, ("boxes", radius))
        ix.set_input(ladder.ref)
        _assert_counts(ix.radius_count(boxes.qry, 0.105), on_ladder[0], "the boxes queries on the ladder cloud, count")
        _assert_rows(ix.radius_search(boxes.qry, 0.105), on_ladder, "the boxes queries on the ladder cloud")
        want = u.reference_of("ladder:short", u.R)
        _assert_counts(ix.radius_count(ladder.qry, u.R), want[0], "ladder after boxes, count")
        _assert_rows(ix.radius_search(ladder.qry, u.R), want, "ladder after boxes")
        ix.set_input(boxes.ref)
        want = u.reference_of("boxes", 0.105)
        _assert_counts(ix.radius_count(boxes.qry, 0.105), want[0], "boxes again, count")
        _assert_rows(ix.radius_search(boxes.qry, 0.30), u.reference_of("boxes", 0.30), "boxes again")
