"""What tests/test_option_parity_gpu.py relies on, checked without a GPU: every scene of tests/option_parity_util.py holds what
its test needs (duplicates, non-finite rows, strays, tied distances in the oracle's own answers, a query count no run length
divides, query counts that make the remap's tail clause live, decoy searches whose answers share no row with the answers under
test), so that a later edit cannot quietly make a GPU test trivial; and
the comparison helpers fail on an answer that is wrong by one swapped index, one flipped bit or one unwritten row."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import option_parity_util as u  # noqa: E402

import oracle  # noqa: E402

BUILD_SIZES = (1, 2, 3, 63, 64, 65, 511, 512, 513, 4095, 4096, 8192, 8193, 65024, 65025, 65535, 65536, 73216, 73728)


@pytest.mark.parametrize("n", BUILD_SIZES)
def test_build_cloud_holds_what_the_build_routes_are_tested_with(n):
    a = u.build_cloud(n)
    assert a.shape == (n, 4) and a.dtype == np.float32 and a.strides == (16, 4)
    assert np.isnan(a[::2, 3]).all() and (a[1::2, 3] == 0).all()           # the fourth float: NaN in every other row
    finite = np.isfinite(a[:, :3]).all(1)
    assert finite[0]
    bad = np.nonzero(~finite)[0]
    assert list(bad) == u.build_nonfinite_rows(n)
    assert len(bad) == len(range(13, n, 97)) - len(set(range(13, n, 97)) & set(u.build_stray_rows(n)))
    if n >= 511:
        assert 0.005 * n <= len(bad) <= 0.012 * n                          # about 1 %
    if n >= 4095:
        assert np.isnan(a[bad, :3]).any() and np.isposinf(a[bad, :3]).any() and np.isneginf(a[bad, :3]).any()
    strays = u.build_stray_rows(n)
    assert len(strays) == (3 if n >= 63 else 0) and len(set(strays)) == len(strays)
    box = np.ones(n, bool)
    box[bad] = False
    box[strays] = False
    assert (a[box, :3] >= 0).all() and (a[box, :3] < u.BUILD_EXTENT).all()
    if strays:
        assert (a[strays, :3] == u.BUILD_STRAYS).all()
        # every stray is 10^3 extents out along its own axis: +x, -x and +y, -z
        assert (np.abs(u.BUILD_STRAYS).max(1) / u.BUILD_EXTENT[np.abs(u.BUILD_STRAYS / u.BUILD_EXTENT).argmax(1)] == 1000).all()
    if n >= 73216:
        # the third stray lies in statistics row 130: in the tail group of rows 128 ... of a 143- or 144-row build
        rows = u.pack_rows(n)
        assert (strays[2] // 256) % rows == 130


def test_build_sizes_sit_on_the_edges_the_pack_kernel_has():
    """pack.hip: one workgroup per 512 points; trimming from 128 rows (:137); a tail group of fewer than 16 rows is skipped
    (grid_params_device.hpp).  65 535 points are 128 rows already -- 65 024 / 65 025 is where 127 becomes 128."""
    rows = {n: u.pack_rows(n) for n in BUILD_SIZES}
    assert rows[511] == rows[512] == 1 and rows[513] == 2
    assert rows[65024] == 127 and rows[65025] == rows[65535] == rows[65536] == 128
    assert rows[73216] == 143 and rows[73216] - 128 == 15 and rows[73728] == 144 and rows[73728] - 128 == 16


def test_build_queries_are_a_third_each_and_a_few_are_not_finite():
    q = u.build_queries()
    assert q.shape == (1000, 3) and q.dtype == np.float32
    bad = ~np.isfinite(q).all(1)
    assert list(np.nonzero(bad)[0]) == [5, 500, 999]
    ok = q[~bad]
    inside = ((ok >= 0) & (ok < u.BUILD_EXTENT)).all(1)
    twice = ((ok >= -0.5 * u.BUILD_EXTENT) & (ok < 1.5 * u.BUILD_EXTENT)).all(1)
    far = (np.abs(ok) >= 29).all(1)
    assert inside.sum() >= 334 - 3 and (twice & ~inside).sum() >= 250 and 330 <= far.sum() <= 333
    assert (twice | far).all() and np.abs(ok).max() < 100                  # far, but nowhere near the strays


@pytest.mark.parametrize("n", [3, 65, 4096])
def test_build_expectations_contain_the_cases_that_matter(n):
    i1, d1, i8, d8, cnt = u.build_expected(n)
    q = u.build_queries()
    bad = ~np.isfinite(q).all(1)
    assert (i1[bad] == -1).all() and np.isinf(d1[bad]).all() and (cnt[bad] == 0).all() and (i8[bad] == -1).all()
    assert (i1[~bad] >= 0).all()
    valid = int(np.isfinite(u.build_cloud(n)[:, :3]).all(1).sum())
    assert ((i8[~bad] >= 0).sum(1) == min(8, valid)).all()                 # short rows below 8 valid points
    if n >= 4096:
        assert (cnt > 0).sum() > 200 and (cnt == 0).sum() > 300            # the radius finds something, and nothing far away


def test_knn_scene_holds_duplicates_piles_clumps_and_a_sparse_scatter():
    ref, fam, q, kind = u.knn_scene()
    assert len(ref) == sum(u.KNN_PARTS.values()) == 12040 and len(q) == u.KNN_NQ == 1501
    # the kernel cuts the FINITE queries into runs (knn.hip:537, 557): that count, and the whole count the issue names, are
    # divided by no run length but 1
    assert int(np.isfinite(q).all(1).sum()) == u.KNN_NQ_FINITE == 1481
    assert [r for r in u.KNN_RUNS if u.KNN_NQ_FINITE % r == 0] == [1] and [r for r in u.KNN_RUNS if u.KNN_NQ % r == 0] == [1]
    finite = np.isfinite(ref).all(1)
    assert (~finite).sum() == 20 and (fam[~finite] == 4).all()
    # exact duplicates: every lattice site three times, every pile 320 times
    _, counts = np.unique(ref[finite], axis=0, return_counts=True)
    assert (counts == 3).sum() == 1000 and (counts == u.KNN_PILE).sum() == 6 and (counts == 1).sum() == 4800 + 2300
    assert u.KNN_PILE >= max(u.KNN_KS)
    # the queries: references themselves, runs of equal queries on the piles, jittered copies, outside the grid, non-finite
    assert [(kind == k).sum() for k in range(5)] == [520, 120, 480, 361, 20]
    assert (~np.isfinite(q).all(1)).sum() == 20 and (kind[~np.isfinite(q).all(1)] == 4).all()
    lo, hi = ref[finite].min(0), ref[finite].max(0)
    assert ((q[kind == 3] < lo) | (q[kind == 3] > hi)).any(1).all()
    _, qcounts = np.unique(q[kind == 1], axis=0, return_counts=True)
    assert list(qcounts) == [20] * 6


def test_knn_expectations_have_zero_kth_distances_ties_and_a_refused_bound():
    ref, fam, q, kind = u.knn_scene()
    for k in (8, 300):
        idx, d2 = u.knn_expected(k)
        assert idx.shape == (1501, k)
        assert (idx[kind == 4] == -1).all() and (idx[kind != 4] >= 0).all()
        assert (d2[kind == 1, k - 1] == 0).all()                           # a pile holds more than k copies: K-th distance 0
        fin = kind != 4
        tied_at_k = bits_equal_neighbours(d2[fin])
        assert tied_at_k.sum() > 100                                       # rows with equal distances in a row: ties by index
    # the sparse scatter at k = 8: the nearest OTHER query, hence the predecessor in any order, is further away than 0.45 of
    # the K-th distance -- the bound of knn.hip (sep <= 0.45 r) is refused there
    idx8, d28 = u.knn_expected(8)
    own_sparse = np.array([i for i in np.nonzero(kind == 0)[0] if fam[idx8[i, 0]] == 3])
    assert len(own_sparse) == 120 and (d28[own_sparse, 0] == 0).all()
    qf = q[kind != 4].astype(np.float64)
    refused = 0
    for i in own_sparse:
        d = np.sqrt(((qf - q[i].astype(np.float64)) ** 2).sum(1))
        sep = np.partition(d, 1)[1]                                        # (the smallest is the query itself)
        refused += sep > 0.45 * np.sqrt(d28[i, 7])
    assert refused >= 108                                                  # nine in ten
    # and it can be taken elsewhere: 200 queries are clump members, millimetres from each other, with a K-th distance at
    # k = 300 of 3 mm and more
    i300, d300 = u.knn_expected(300)
    clump_q = [i for i in np.nonzero(kind == 0)[0] if fam[i300[i, 0]] == 2]
    assert len(clump_q) == 200 and (np.sqrt(d300[clump_q, 299]) > 0.003).all()


@pytest.mark.parametrize("k", [1, 8, 300])
def test_knn_decoy_rows_differ_from_the_rows_under_test_everywhere(k):
    """the decoy search leaves, in every row of a finite query, something else than the search after it must write"""
    q, dq = u.knn_queries(False), u.knn_queries(True)
    assert q.shape == dq.shape and (np.isfinite(q).all(1) == np.isfinite(dq).all(1)[::-1]).all()
    assert u.rows_in_common(*u.knn_expected(k, False), *u.knn_expected(k, True)) == 0
    assert u.rows_in_common(*u.knn_expected(k, False), *u.knn_expected(k, False)) == u.KNN_NQ_FINITE   # (the helper counts)


def test_small_and_self_knn_decoys_differ_everywhere():
    ref, q = u.knn_small_scene()
    assert u.rows_in_common(*oracle.knn_exhaustive(ref, q, 51), *oracle.knn_exhaustive(ref, u.decoy_of(q), 51)) == 0
    a = u.self_knn_scene()
    b = u.decoy_of(a)
    ia, da = u.knn_oracle(a, a, 50)
    ib, db = u.knn_oracle(b, b, 50)
    assert u.rows_in_common(ia, da, ib, db) == 0
    ma, mb = oracle.sor(a, 50, 1.5)[0], oracle.sor(b, 50, 1.5)[0]
    assert ((u.bits(ma) == u.bits(mb)) & np.isfinite(a).all(1) & np.isfinite(b).all(1)).sum() == 0


def bits_equal_neighbours(d2):
    """rows in which two consecutive distances carry the same bits"""
    b = u.bits(d2).reshape(d2.shape)
    return (b[:, 1:] == b[:, :-1]).any(1)


def test_small_knn_scene_has_fewer_points_than_k():
    ref, q = u.knn_small_scene()
    assert np.isfinite(ref).all(1).sum() == 37 and len(q) == 90 and 90 % 16 != 0
    idx, d2 = oracle.knn_exhaustive(ref, q, 51)
    ok = np.isfinite(q).all(1)
    assert ((idx[ok] >= 0).sum(1) == 37).all() and (idx[ok][:, 37:] == -1).all() and np.isinf(d2[ok][:, 37:]).all()
    assert (idx[~ok] == -1).all()


def test_self_knn_scene_has_duplicates_and_a_non_finite_point():
    a = u.self_knn_scene()
    assert a.shape == (6000, 3) and (~np.isfinite(a).all(1)).sum() == 1
    _, counts = np.unique(a[np.isfinite(a).all(1)], axis=0, return_counts=True)
    assert (counts == 2).sum() >= 29


def test_placement_counts_make_every_clause_of_the_remap_live():
    """the arithmetic of grid.hip:1021 (clamp), :1041 (flat kernel: 128 queries a workgroup) and :1076 (lane kernel: 256, half the
    run) restated: effective runs of 1, 2 and 3 occur, and wherever a kernel remaps its workgroup count is no multiple of 8 x run
    and leaves a tail"""
    runs = {nq: {u.placement_effective_run(nq, o) for o in u.XCD_RUNS} for nq in u.PLACEMENT_NQ}
    assert runs[2500] == {1} and runs[4700] == {1, 2} and runs[6700] == {1, 2, 3} and runs[10300] == {1, 2, 3, 5}
    seen = set()
    for nq in u.PLACEMENT_NQ:
        for form in u.NN1_FORMS:
            for o in u.XCD_RUNS:
                wg, run = u.placement_launch(nq, form, o)
                if run > 1:
                    assert wg % (8 * run) != 0 and wg > 8 * run, (nq, form, o)   # remapped workgroups AND a tail
                    seen.add((form, run, wg % (8 * run)))
    assert {(f, r) for f, r, _ in seen} == {(1, 2), (1, 3), (1, 5), (0, 2), (0, 3)}
    assert (1, 5, 1) in seen                                               # a tail of exactly one workgroup
    # the remap as the kernels apply it (grid.hip:280) is a bijection of the workgroup numbers at every launch used here
    for nq in u.PLACEMENT_NQ:
        for form in u.NN1_FORMS:
            for o in u.XCD_RUNS:
                wg, run = u.placement_launch(nq, form, o)
                per, bid = 8 * run, np.arange(wg)
                full = wg // per * per
                base = bid // per * per
                inn = bid - base
                mapped = np.where((run > 1) & (bid < full), base + (inn & 7) * run + (inn >> 3), bid)
                assert sorted(mapped) == list(range(wg))


@pytest.mark.parametrize("nq", u.PLACEMENT_NQ)
def test_placement_decoy_keys_differ_from_the_keys_under_test_everywhere(nq):
    """a query the remap loses keeps the decoy's key: that key must be wrong for every finite query"""
    q, dq = u.placement_queries(nq, False), u.placement_queries(nq, True)
    assert q.shape == dq.shape == (nq, 3)
    assert u.rows_in_common(*u.placement_expected(nq, False), *u.placement_expected(nq, True)) == 0
    # and a finite query never sits where the decoy had a non-finite one, whose preset "nothing found" would be stale too --
    # except that the search under test must then find something: -1 against an index is a difference as well
    assert (u.placement_expected(nq, False)[0][np.isfinite(q).all(1)] >= 0).all()


def test_placement_scene_has_a_pile_clumps_and_tied_answers():
    ref, q = u.placement_scene()
    assert ref.shape == (20000, 3) and len(q) == max(u.PLACEMENT_NQ)
    assert (ref == np.float32(0.5)).all(1).sum() == 5900                   # one cell holds thousands of equal points
    for nq in (2500, 10300):
        idx, d2 = u.placement_expected(nq)
        bad = ~np.isfinite(q[:nq]).all(1)
        assert bad.sum() >= 7 and (idx[bad] == -1).all() and (idx[~bad] >= 0).all()
        on_pile = (ref[idx[~bad]] == np.float32(0.5)).all(1)
        assert on_pile.sum() > 50                                          # answers decided by the lowest index among 5900 equals
        assert (d2[~bad] == 0).sum() > nq // 12                            # queries that ARE references


def test_icp_scenes_sit_on_both_sides_of_the_sums_workgroup_and_the_sorted_threshold():
    assert [(m + 2047) // 2048 for m in u.ICP_SOURCE_SIZES] == [1, 2, 2, 2, 3]
    assert [m >= 4096 for m in u.ICP_SOURCE_SIZES] == [False, False, False, True, True]
    assert (u.ICP_ROW_CAP_POINTS + 2047) // 2048 == 481 and (u.ICP_ROW_CAP_POINTS - 1 + 2047) // 2048 == 480
    tgt, src = u.icp_scene(2049)
    assert tgt.shape == (20000, 3) and src.shape == (2049, 3) and src.dtype == np.float32
    assert 0.001 < np.abs(src - tgt[:2049]).max() < 2.0                    # moved (2 degrees about z, centimetres along), not gone


def test_rebuild_and_tie_scenes():
    first, second, q = u.rebuild_clouds()
    assert len(first) == 5000 and len(second) == 20000 and not np.isfinite(second).all()
    assert np.nanmin(second, 0).min() > first.max()                        # two different clouds: an answer from the old one shows
    ref, tq = u.tie_scene()
    assert len(ref) == 900 and len(ref) <= 4096                            # small_call: at most 4096 exhaustively searched points
    idx, d2 = oracle.knn_exhaustive(ref, tq, 3)
    assert (d2 == 0).all()                                                 # every query's nearest reference exists three times


# ---- the comparison helpers notice what they are there to notice -------------------------------------------------------------
def _tied_answer():
    ref, tq = u.tie_scene()
    idx, d2 = oracle.knn_exhaustive(ref, tq, 3)
    return idx.copy(), d2.copy()


def test_helpers_accept_the_oracle_itself():
    idx, d2 = _tied_answer()
    u.assert_same_rows(idx.copy(), d2.copy(), idx, d2)
    u.assert_same_counts(np.arange(5), np.arange(5))


def test_helpers_fail_on_an_index_swapped_between_two_tied_neighbours():
    idx, d2 = _tied_answer()
    got = idx.copy()
    assert d2[17, 0] == d2[17, 1] and got[17, 0] != got[17, 1]
    got[17, [0, 1]] = got[17, [1, 0]]
    with pytest.raises(AssertionError, match="indices differ"):
        u.assert_same_rows(got, d2.copy(), idx, d2)


def test_helpers_fail_on_one_flipped_d2_bit():
    idx, d2 = u.placement_expected(2500)
    got = d2.copy()
    row = int(np.nonzero(np.isfinite(d2) & (d2 > 0))[0][3])
    got.view(np.uint32)[row] ^= 1
    assert abs(float(got[row]) - float(d2[row])) < 1e-9                    # one ulp: no tolerance would see it
    with pytest.raises(AssertionError, match="d2 bits differ"):
        u.assert_same_rows(idx.copy(), got, idx, d2)
    # and on the sign of a zero, which == does not see
    zero = int(np.nonzero(d2 == 0)[0][0])
    got = d2.copy()
    got[zero] = -0.0
    assert (got == d2).all() or np.isnan(d2).any()
    with pytest.raises(AssertionError, match="d2 bits differ"):
        u.assert_same_rows(idx.copy(), got, idx, d2)


def test_helpers_fail_on_a_row_left_at_its_fill_value():
    idx, d2 = u.placement_expected(2500)
    gi, gd = u.filled(idx.shape)
    assert (gi == u.FILL_IDX).all() and (u.bits(gd) == u.FILL_D2_BITS).all() and np.isnan(gd).all()
    gi[:], gd[:] = idx, d2
    gi[1234] = u.FILL_IDX
    with pytest.raises(AssertionError, match="never written"):
        u.assert_same_rows(gi, gd, idx, d2)
    gi[1234] = idx[1234]
    gd.view(np.uint32)[77] = u.FILL_D2_BITS
    with pytest.raises(AssertionError, match="never written"):
        u.assert_same_rows(gi, gd, idx, d2)
    with pytest.raises(AssertionError, match="counts differ"):
        u.assert_same_counts(np.array([1, 2, 3]), np.array([1, 2, 4]))
