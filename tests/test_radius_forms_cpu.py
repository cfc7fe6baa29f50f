"""What the scenes of tests/test_radius_forms_gpu.py must show, held without a GPU: every scene reaches the side of every
threshold it was aimed at, by the route model of tests/radius_forms_util.py with the constants read from knn.hip and
pcc_internal.hpp (a constant that moves fails here and names the scene to aim again, not silently on the GPU), and the
exhaustive reference agrees with the oracle's kd-tree rows and exhaustive counts.

The model's grid is that of tools/bucket_sizes.py.  No host compile of grid_params_block exists (tests/cpp mirrors the public
C++ interface, not the device's grid derivation), so the grid cannot be held against the library's here:
tests/test_radius_forms_gpu.py compares the handle's cell count with the model's for every scene it runs, as
tests/test_cellsort_levels_gpu.py does."""
import numpy as np
import pytest

import oracle
import radius_forms_util as u


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _at(m, queries):
    """positions among the model's finite queries of the given query indices"""
    pos = np.searchsorted(m.finite, queries)
    assert (m.finite[pos] == queries).all()
    return pos


def test_every_constant_is_read_from_the_sources_and_is_what_the_scenes_aim_at():
    assert set(u.CONSTANTS) == set(u.AIMED)
    for name, (value, scenes) in u.AIMED.items():
        assert u.CONSTANTS[name] == value, (name, "moved from", value, "to", u.CONSTANTS[name], "-- aim again:", scenes)
    assert u.ROW_STEPS == u.AIMED_ROW_STEPS, ("the register steps of emit / sort_row moved -- aim again: ladder, ties", u.ROW_STEPS)
    assert u._constant("constexpr unsigned int A = 256, B = 128, C = 3 * 8;", "C") == 24
    assert u._constant("constexpr int RAD_ROWCAP = 11 * 11;", "RAD_ROWCAP") == 121 and u._constant("constexpr unsigned int X = 4 * 1u << 11;", "X") == 8192
    with pytest.raises(LookupError):
        u._constant("constexpr unsigned int A = 256;", "B")
    with pytest.raises(LookupError):
        u._row_steps("if (row_len <= 64) emit(")


def test_the_reference_on_a_hand_made_cloud():
    """strict d2 < r2, rows ascending by (d2, index), non-finite points on either side"""
    ref = np.array([[0.5, 0, 0], [0, 0.25, 0], [np.nan, 0, 0], [0, 0, -0.25], [0, 0, 0], [0.25, 0, 0], [0, 0.499, 0]], np.float32)
    qry = np.array([[0, 0, 0], [np.inf, 0, 0], [3, 3, 3], [0.5, 0, 0]], np.float32)
    offsets, idx, d2 = u.reference(ref, qry, 0.5)
    assert offsets.tolist() == [0, 5, 5, 5, 7]
    assert idx.tolist() == [4, 1, 3, 5, 6, 0, 5]                  # the reference AT 0.5 is no neighbour; 1, 3, 5 tie and go by index
    assert d2.tolist()[:4] == [0.0, 0.0625, 0.0625, 0.0625] and d2.tolist()[5:] == [0.0, 0.0625]
    assert u.rows_with_ties(offsets, d2).tolist() == [0]
    assert u.radius2(0.05) == np.float32(0.05 * 0.05) and u.radius2(0.05) != np.float32(0.05) * np.float32(0.05)


@pytest.mark.parametrize("name", ["ladder:long", "ladder:short", "ties"])
def test_rungs_hold_exactly_their_lengths_and_the_thresholds_lie_between_them(name):
    sc, m = u.scene(name), u.model_of(name, u.R)
    length = m.length[_at(m, sc.rung_query)]
    assert length.tolist() == list(sc.rungs), (name, "a rung does not hold its length -- aim again:", name)
    rest = np.setdiff1d(m.finite, sc.rung_query)
    assert len(rest) >= 9 and (m.length[_at(m, rest)] == 0).all(), (name, "a far query is not alone")
    for t in set(u.ROW_STEPS) | {u.ROW_LDS_MAX, u.ROW_SORT_MAX, u.RAD_WAVE_MEAN}:
        assert {t - 1, t, t + 1} <= set(sc.rungs), (name, "no rung on either side of", t)
    assert {0, 1, 2} <= set(sc.rungs) and max(sc.rungs) > 2 * u.ROW_SORT_MAX       # (sort_long_row beyond one merge level)
    assert m.nq % 4 != 0 and m.turns == 1
    assert not sc.ref.flags.writeable and not sc.qry.flags.writeable and len(sc.ref) < 6200
    assert (~np.isfinite(sc.ref).all(1)).sum() == 3 and (~np.isfinite(sc.qry).all(1)).sum() == 1
    # the centres sit 20 radii apart: every candidate a ball's box holds is a hit or a neighbour cluster's cell away
    assert u.SPACING >= 20 * u.R


def test_ladder_runs_on_either_side_of_the_mean():
    long_, short = u.model_of("ladder:long", u.R), u.model_of("ladder:short", u.R)
    assert long_.total == short.total == sum(u.LADDER)
    assert long_.wave_fill and long_.total < u.RAD_WAVE_MEAN * (long_.nq + 1), ("ladder:long is not the last query count on the wave side", long_.total, long_.nq)
    # (nq + 1 would be the first on the lane side, and is a multiple of 4: the next one)
    assert not short.wave_fill and short.nq == long_.nq + 2 and (long_.nq + 1) % 4 == 0, ("ladder:short", short.total, short.nq)
    a, b = u.scene("ladder:long"), u.scene("ladder:short")
    assert a.ref is not b.ref and (_bits(a.ref) == _bits(b.ref)).all() and (_bits(a.qry) == _bits(b.qry[:len(a.qry)])).all()
    assert np.isfinite(b.qry[len(a.qry):]).all()
    ra, rb = u.reference_of("ladder:long", u.R), u.reference_of("ladder:short", u.R)
    assert (ra[0] == rb[0][:len(ra[0])]).all() and (ra[1] == rb[1]).all() and (_bits(ra[2]) == _bits(rb[2])).all()
    # the rows are generic: no two neighbours of a centre at one distance
    assert len(u.rows_with_ties(ra[0], ra[2])) == 0


def test_ties_fill_one_bucket_to_the_brim_and_beyond():
    sc, m = u.scene("ties"), u.model_of("ties", u.R)
    offsets, idx, d2 = u.reference_of("ties", u.R)
    fullest = dict(zip(sc.rungs, m.bucket_max[_at(m, sc.rung_query)].tolist()))
    assert fullest[40] == u.BUCKET_FULL and fullest[41] == u.BUCKET_FULL + 1, ("aim again: ties, the rungs of 40 and 41", fullest)
    for length in sc.rungs:
        q = sc.rung_query[sc.rungs.index(length)]
        row = d2[offsets[q]:offsets[q + 1]]
        assert len(np.unique(row)) == min(3, sum(k > 0 for k in u.ties_split(length))), (length, "not on its shells")
        assert fullest[length] == max(u.ties_split(length)), (length, "two shells share a bucket")
        if 63 <= length <= u.ROW_LDS_MAX:
            assert fullest[length] > u.BUCKET_FULL            # handed back to the network
        if 23 <= length <= 25:
            assert 2 <= fullest[length] <= u.BUCKET_FULL      # ranked inside the bucket: equal d2, by index
    # exact: every d2 is (an integer) * SHELL_SCALE^2
    units = d2.astype(np.float64) / u.SHELL_SCALE ** 2
    assert (units == np.round(units)).all() and set(np.unique(units).astype(int)) == {k for k, _ in u._shells()}
    assert len(u.rows_with_ties(offsets, d2)) == len(sc.rungs) - 2       # every rung but those of 0 and 1


def test_boxes_reach_both_forms_of_the_row_walk_and_of_the_count():
    sc = u.scene("boxes")
    ms = {r: u.model_of("boxes", r) for r in sc.radii}
    assert 5900 <= len(sc.ref) <= 6100 and len(sc.qry) % 4 != 0
    assert (ms[0.16].ny <= 8).all() and ms[0.16].form8.all() and (ms[0.16].ny == 8).any(), "aim again: boxes, r = 0.16"
    m = ms[0.22]
    assert ((m.ny == 8) & m.form8).any() and (m.ny == 9).any() and (m.ny == 10).any() and not m.form8[m.ny > 8].any(), "aim again: boxes, r = 0.22"
    assert ((m.ny <= 8) & ~m.form8).any()            # (a ball the grid's side cuts to 8 rows a layer, but more than 8 layers)
    assert (ms[0.25].nrow <= u.RAD_ROWCAP).all() and (ms[0.25].nrow == u.RAD_ROWCAP).any(), ("aim again: boxes, r = 0.25", ms[0.25].nrow.max())
    assert ((ms[0.30].nrow > u.RAD_ROWCAP) & (ms[0.30].nrow <= 2 * u.RAD_ROWCAP)).any(), "aim again: boxes, r = 0.30"
    assert (ms[0.45].nrow > 2 * u.RAD_ROWCAP).any() and ms[0.45].length.max() > 4 * u.ROW_SORT_MAX          # three chunks
    assert all(m.cand_box.max() <= u.RAD_FLAT_CAP for m in ms.values())
    # the count: lane form below RAD_COUNT_WAVE_MIN, wave form from it on, a radius within an eighth of it on either side
    lo, hi = ms[0.105].count_expr, ms[0.11].count_expr
    assert 0.875 * u.RAD_COUNT_WAVE_MIN <= lo < u.RAD_COUNT_WAVE_MIN <= hi <= 1.125 * u.RAD_COUNT_WAVE_MIN, ("aim again: boxes, r = 0.105 and 0.11", lo, hi)
    assert not ms[0.10].count_by_wave and all(ms[r].count_by_wave for r in sc.radii if r >= 0.11)
    # the fill on either side of the mean, rows on either side of every step, balls that leave the grid
    assert not ms[0.10].wave_fill and not ms[0.105].wave_fill and all(ms[r].wave_fill for r in sc.radii if r >= 0.11)
    lengths = np.concatenate([m.length for r, m in ms.items() if m.wave_fill])
    for t in set(u.ROW_STEPS) | {u.ROW_LDS_MAX, u.ROW_SORT_MAX}:
        assert (lengths <= t).any() and (lengths > t).any()
    finite = sc.qry[np.isfinite(sc.qry).all(1)]
    assert ((finite < 0) | (finite > 1)).any(1).sum() >= 10 and (~np.isfinite(sc.qry).all(1)).sum() == 1


def test_crowd_has_a_chunk_beyond_the_flat_cap_and_fills_every_bit_plane():
    sc = u.scene("crowd")
    far, near = (u.model_of("crowd", r) for r in sc.radii)
    assert far.ncells == near.ncells == 343 and len(sc.qry) == 25
    # one chunk (a ball of up to RAD_ROWCAP rows) with more HITS than the cap: whatever the chord clip leaves, the walk by windows
    assert (far.nrow <= u.RAD_ROWCAP).all() and (far.length > u.RAD_FLAT_CAP).sum() >= 8, ("aim again: crowd, r = 0.6", far.length.max())
    assert (far.cand_box <= u.RAD_FLAT_CAP).any()                     # (and the flat form beside it, at the grid's corners)
    assert far.cand_box.max() == np.isfinite(sc.ref).all(1).sum()     # a ball over the whole grid sees every reference
    # the other radius: no chunk beyond the cap by the upper bound, candidates in every plane by the lower one
    assert (near.cand_box <= u.RAD_FLAT_CAP).all(), ("aim again: crowd, r = 0.34", near.cand_box.max())
    plane = u.RAD_FLAT_CAP // 4
    for k in (1, 2, 3):
        assert (near.cand_lo > k * plane).any(), ("aim again: crowd, r = 0.34: nothing in bit plane", k)
    assert (near.cand_lo <= near.cand).all() and (near.cand <= near.cand_box).all() and (near.length <= near.cand_lo).all()
    assert (far.cand_lo <= far.cand).all() and (far.cand <= far.cand_box).all() and (far.length <= far.cand_lo).all()


def test_turns_gives_waves_a_second_and_a_third_query():
    m = u.model_of("turns", u.TURNS_RADIUS)
    assert m.turns == 3 and 0 < len(m.finite) % u.MAX_WAVES < 64 and m.nq % 4 != 0
    assert m.wave_fill and m.count_by_wave and m.length.max() <= 128 and m.total < 2_500_000


@pytest.mark.parametrize("name", ["ladder:short", "ties"])
def test_reference_equals_the_kd_tree_rows(name):
    """every query, indices and distance bits (the oracle's rows are sorted by (d2, index))"""
    sc = u.scene(name)
    offsets, idx, d2 = u.reference_of(name, u.R)
    tree = oracle.KdTree(sc.ref)
    for i, q in enumerate(sc.qry):
        oi, od = tree.radius(q, u.R, sorted=True) if np.isfinite(q).all() else (np.empty(0, np.int32), np.empty(0, np.float32))
        assert offsets[i + 1] - offsets[i] == len(oi), (name, i)
        assert (idx[offsets[i]:offsets[i + 1]] == oi).all() and (_bits(d2[offsets[i]:offsets[i + 1]]) == _bits(od)).all(), (name, i)


@pytest.mark.parametrize("name,radius", u.CASES)
def test_reference_equals_the_exhaustive_count(name, radius):
    sc = u.scene(name)
    want = oracle.radius_count_exhaustive(sc.ref, sc.qry, radius)
    assert (np.diff(u.reference_of(name, radius)[0]) == want).all()
    assert (want[~np.isfinite(sc.qry).all(1)] == 0).all()


def test_the_normals_clouds():
    """the keys route without fusion (normals.hip radius_csr): self rows on the wave side of the mean, rows on either side of
    every step of k_sort_rows; the long cloud has no two neighbours of a point at one distance"""
    p = u.normals_long_cloud()
    offsets, _, d2 = u.reference(p, p, u.NORMALS_LONG_RADIUS)
    length = np.diff(offsets)
    assert len(u.rows_with_ties(offsets, d2)) == 0, "aim again: NORMALS_LONG_SEED"
    assert offsets[-1] >= u.RAD_WAVE_MEAN * len(p) and (length > u.ROW_SORT_MAX).sum() > 100 and ((length > u.ROW_LDS_MAX) & (length <= u.ROW_SORT_MAX)).sum() > 100
    for name, radius in (("ladder:long", u.R), ("boxes", 0.30)):
        ref = u.scene(name).ref
        offsets, _, d2 = u.reference(ref, ref, radius)
        length = np.diff(offsets)
        assert offsets[-1] >= u.RAD_WAVE_MEAN * len(ref) and length.max() > u.ROW_SORT_MAX and len(u.rows_with_ties(offsets, d2)) < 0.01 * len(ref)
        for t in set(u.ROW_STEPS) | {u.ROW_SORT_MAX}:
            assert (length <= t).any() and (length > t).any(), (name, t)
