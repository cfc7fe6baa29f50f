"""include/pcc_nn.h promises of the 26 options of pcc_index_set_option that none of them changes a result bit of a search
(PCC_OPT_ICP_SORTED is the documented exception).  Each option selects between hand-written kernel routes; this file holds the
options no other test sets to anything but their default to that promise, on small clouds built for the edges each has.  Every
comparison is with the oracle's exhaustive scan -- or, route against route, with the same handle's default route -- and bit for
bit: indices equal, float32 values equal as uint32.  Scenes and helpers: tests/option_parity_util.py, pinned by
tests/test_option_parity_cpu.py.

A kernel that skips a query leaves, in the handle's result buffers, what the previous call on the handle wrote there -- and the
caller's arrays are filled from those buffers whatever the kernel did.  Where one handle is searched under several settings
every search therefore follows a decoy search of the same shape over other queries (option_parity_util.decoy_of), both checked:
a stale row is then a wrong row.  (The fill values the output arrays start with only show an entry the library never
delivered to the caller.)

No test can see which route ran: the library chooses it by host conditions that nothing reports back.  The conditions are
quoted beside the sizes derived from them -- api.hip:353 (fused grid derivation), pack.hip:137 and grid.hip:53 (trimming from
128 statistics rows), grid.hip:1021 (the XCD run's clamp), icp.hip:360 (the sorted working order from 4096 points) and :423
(the fused solve).

Where every option is set to a non-default value by a test that compares results:

 1 GRID_PPC              here: test_trim_and_density_settings_build_the_same_grid_either_way
 2 GRID_TRIM             here: test_trim_and_density_settings_build_the_same_grid_either_way
 3 FAR_MODE              test_nn1_gpu.py (far queries, both modes)
 4 ICP_WARM              here: test_icp_fused_solve_working_order_and_warm_start; test_search_gpu.py
 5 ICP_DEVICE_LOOP       test_search_gpu.py: test_icp_align_options_do_not_change_a_bit
 6 EC_CELLS              test_search_gpu.py: test_euclidean_clusters_known_partition
 7 SORT_MP_MIN           test_nn1_kernels_gpu.py: test_three_level_sort_forms_build_the_same_index
 8 SORT_MP_MIN_Q         test_nn1_kernels_gpu.py: test_three_level_sort_forms_build_the_same_index
 9 NN1_KERNEL            here: test_k1_placement_options; test_nn1_kernels_gpu.py
10 FLANN_SPLIT           test_nn1_gpu.py (the replayed split rules)
11 NN1_DENSE_MIN         here: test_k1_placement_options
12 KNN_KERNEL            test_search_gpu.py: test_knn_selection_kernel_and_merge_kernel_agree_with_the_oracle
13 KNN_CACHE_K           test_search_gpu.py: test_kept_self_knn_rows_serve_normals_and_region_growing
14 NN1_OPEN_FLAT         test_nn1_kernels_gpu.py: test_nn1_kernel_forms_match_the_oracle
15 SORT_STAGE1           test_nn1_kernels_gpu.py: test_three_level_sort_forms_build_the_same_index
16 ICP_SORTED            here: test_icp_fused_solve_working_order_and_warm_start; test_fullsize_gpu.py
17 OVERLAP_PREP          test_nn1_gpu.py, test_fullsize_gpu.py
18 GRID_AXES             test_grid_axes_gpu.py
19 XCD_RUN               here: test_k1_placement_options
20 FUSE_PARAMS           here: bit 1 test_build_routes_give_one_index and the tests after it, bit 2 the ICP tests
21 HOST_PIPE             here: test_build_routes_give_one_index, test_rebuilds_on_one_handle...; test_nn1_gpu.py
22 SCAN_CHAINED          test_search_gpu.py: test_voxel_grid_sizes_around_the_scan_forms
23 KNN_RUN               here: test_knn_run_lengths and the two tests after it
24 RIFT_LAYOUT           test_rift_gpu.py, test_rift_batch_gpu.py
25 SIFT_LAYOUT           test_sift_gpu.py
26 RIFT_BATCH_BRUTE_MAX  test_rift_batch_gpu.py"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import option_parity_util as u  # noqa: E402

import oracle  # noqa: E402
from pointcloudcomparator_amd import capi, synth  # noqa: E402

pytestmark = pytest.mark.gpu

NOMEM, EMPTY = -4, -2  # enum pcc_status


def _check_searches(ix, n, what):
    """k = 1, k = 8 and a radius count of the 1000 build queries on `ix` against the oracle over build_cloud(n)"""
    q = u.build_queries()
    i1, d1, i8, d8, cnt = u.build_expected(n)
    gi, gd = u.filled((len(q),))
    ix.nn1(q, out_idx=gi, out_d2=gd)
    u.assert_same_rows(gi, gd, i1, d1, (what, "nn1"))
    ki, kd = ix.knn(q, 8)
    u.assert_same_rows(ki, kd, i8, d8, (what, "knn 8"))
    u.assert_same_counts(ix.radius_count(q, u.BUILD_RADIUS), cnt, (what, "radius count"))


# ---- A: build routes -----------------------------------------------------------------------------------------------------------
# api.hip:353  fused = (fuse_params & 1) || (host_pipe && n <= SMALL_FUSED_POINTS (8192)): with FUSE_PARAMS = 0 the launch of
# k_grid_params runs from 8193 points on, and below only with HOST_PIPE = 0.  One pack workgroup takes 512 points and writes one
# statistics row: 511 / 512 / 513 are one and two rows; trimming acts from 128 rows (pack.hip:137, grid.hip:53), i.e. from 65 025
# points -- 65 024 is the last size without it, 65 535 and 65 536 both have it; the trimmed box takes the rows in groups of 64 and
# skips a tail group of fewer than 16: 73 216 points are 143 rows (a tail of 15, skipped), 73 728 are 144 (a tail of 16, counted),
# and the third stray lies in row 130.  4095 / 4096: where PCC_ENGINE_AUTO changes engine -- the grid is forced in every case.
BUILD_SIZES = (1, 2, 3, 63, 64, 65, 511, 512, 513, 4095, 4096, 8192, 8193, 65024, 65025, 65535, 65536, 73216, 73728)


@pytest.mark.parametrize("n", BUILD_SIZES)
def test_build_routes_give_one_index(gpu, n):
    """FUSE_PARAMS bit 1 x HOST_PIPE x {host array, device tensor}: eight routes to the index of one cloud -- an anisotropic box
    with non-finite rows, three strays at 10^3 extents and NaN in the fourth float of every other 16-byte record.  All count the
    same valid points and lay the same number of cells; k = 1, k = 8 and radius counts carry the oracle's bits after each."""
    import torch
    cloud = u.build_cloud(n)
    valid = int(np.isfinite(cloud[:, :3]).all(1).sum())
    seen = {}
    for mem, pts in (("host", cloud), ("device", torch.from_numpy(cloud.copy()).cuda())):
        with capi.Index(pts, engine=capi.ENGINE_GRID) as ix:
            for fuse in (0, 1):
                for pipe in (1, 0):
                    ix.set_option(capi.OPT_FUSE_PARAMS, fuse)
                    ix.set_option(capi.OPT_HOST_PIPE, pipe)
                    ix.set_input(pts)
                    st = ix.stats()
                    seen[(mem, fuse, pipe)] = (st[2], st[3])
                    _check_searches(ix, n, (n, mem, "fuse", fuse, "pipe", pipe))
    assert len(seen) == 8 and set(seen.values()) == {(valid, seen[("host", 0, 1)][1])}, seen


@pytest.mark.parametrize("n", (4096, 65024, 65535, 65536, 73728))
def test_trim_and_density_settings_build_the_same_grid_either_way(gpu, n):
    """GRID_TRIM x GRID_PPC x FUSE_PARAMS bit 1: the fused derivation and k_grid_params lay the same number of cells under every
    setting, and every grid answers with the oracle's bits.  HOST_PIPE is 0 throughout: with 1, api.hip:353 fuses every cloud of up
    to 8192 points and the 4096-point case would compare the fused form with itself.  That the scene exercises the trim at all:
    with 128 statistics rows or more (65 025 points) GRID_TRIM = 3 drops the strays and lays other cells than GRID_TRIM = 0;
    below, the option does nothing.
    (65 535 points are 128 rows: trimmed, like 65 536.  The last untrimmed size is 65 024.)"""
    cloud = u.build_cloud(n)
    cells = {}
    with capi.Index(cloud, engine=capi.ENGINE_GRID) as ix:
        ix.set_option(capi.OPT_HOST_PIPE, 0)
        for trim in (0, 3, 8):
            for ppc in (0.05, 0.75, 64.0):
                for fuse in (0, 1):
                    ix.set_option(capi.OPT_GRID_TRIM, trim)
                    ix.set_option(capi.OPT_GRID_PPC, ppc)
                    ix.set_option(capi.OPT_FUSE_PARAMS, fuse)
                    ix.set_input(cloud)
                    cells[(trim, ppc, fuse)] = ix.stats()[3]
                    _check_searches(ix, n, (n, "trim", trim, "ppc", ppc, "fuse", fuse))
    for trim, ppc, _ in cells:
        assert cells[(trim, ppc, 0)] == cells[(trim, ppc, 1)], (trim, ppc, cells)
    trimmed = u.pack_rows(n) >= 128
    assert (cells[(3, 0.75, 0)] != cells[(0, 0.75, 0)]) == trimmed, (n, cells)
    assert len({cells[(0, ppc, 0)] for ppc in (0.05, 0.75, 64.0)}) == 3    # (and the density option is not ignored either)


def test_rebuilds_on_one_handle_alternate_between_the_two_derivations(gpu):
    """six pcc_index_set_input calls on ONE handle, 8000 and 70 000 points in turn, FUSE_PARAMS (and once HOST_PIPE) flipped
    between them: the ticket word the fused form counts its workgroups in must be back at zero for every later build, whichever
    form ran in between -- a k = 1 search after each build against the oracle"""
    q = u.build_queries()
    small, large = u.build_cloud(8000), u.build_cloud(70000)
    want = {8000: oracle.nn1_exhaustive(small, q), 70000: oracle.nn1_exhaustive(large, q)}
    # (points, FUSE_PARAMS, HOST_PIPE) -> the form api.hip:353 takes
    sequence = [(8000, 0, 1),     # fused: the small-cloud rule
                (70000, 0, 1),    # k_grid_params
                (8000, 1, 1),     # fused
                (70000, 1, 1),    # fused, 137 workgroups
                (8000, 0, 0),     # k_grid_params for a small cloud
                (70000, 1, 0)]    # fused
    with capi.Index(small, engine=capi.ENGINE_GRID) as ix:
        for step, (n, fuse, pipe) in enumerate(sequence):
            ix.set_option(capi.OPT_FUSE_PARAMS, fuse)
            ix.set_option(capi.OPT_HOST_PIPE, pipe)
            ix.set_input(small if n == 8000 else large)
            gi, gd = u.filled((len(q),))
            ix.nn1(q, out_idx=gi, out_d2=gd)
            u.assert_same_rows(gi, gd, *want[n], ("build", step, n, fuse, pipe))
            assert ix.stats()[2] == int(np.isfinite(u.build_cloud(n)[:, :3]).all(1).sum())


# ---- B: KNN_RUN -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", u.KNN_KS)
def test_knn_run_lengths(gpu, k):
    """PCC_OPT_KNN_RUN: every query after the first of its run starts from a bound (the predecessor's K-th distance plus their
    separation, taken only while the separation is at most 0.45 of that distance) and falls through to the full path when the
    bound misses.  Runs of 1 (no bound at all), 2, 7, 16 and 64.  The kernel cuts the cell-sorted order of the FINITE queries into
    runs (knn.hip:537, 557): 1481 of the 1501 queries, a prime, so the last run is short under every length but 1; the 20
    non-finite queries never enter a run, their rows are preset.  Piles (K-th distance 0), duplicates, clumps (the bound is taken),
    a sparse scatter (it is refused) and queries outside the grid: the oracle's rows, whatever the run.  Every search follows a
    decoy search of the same shape, so a query the run arithmetic dropped would keep a row of other queries."""
    ref = u.knn_scene()[0]
    with capi.Index(ref, engine=capi.ENGINE_GRID) as ix:
        for run in u.KNN_RUNS:
            ix.set_option(capi.OPT_KNN_RUN, run)
            for decoy in (True, False):
                idx, d2 = ix.knn(u.knn_queries(decoy), k)
                u.assert_same_rows(idx, d2, *u.knn_expected(k, decoy), ("k", k, "run", run, "decoy" if decoy else "queries"))


def test_knn_runs_over_a_cloud_smaller_than_k(gpu):
    """40 points, 37 of them finite, k = 51: no row is ever full, so no query hands a bound to the next one of its run"""
    ref, q = u.knn_small_scene()
    with capi.Index(ref, engine=capi.ENGINE_GRID) as ix:
        for run in u.KNN_RUNS:
            ix.set_option(capi.OPT_KNN_RUN, run)
            for qq in (u.decoy_of(q), q):                                  # (the decoy first: see the file's docstring)
                idx, d2 = ix.knn(qq, 51)
                u.assert_same_rows(idx, d2, *oracle.knn_exhaustive(ref, qq, 51), ("run", run))
                assert (idx[np.isfinite(qq).all(1)][:, 37:] == -1).all()


def test_knn_runs_behind_sor_and_normals(gpu):
    """the consumers of the self k-NN rows, pcc_sor and pcc_normals(50), under KNN_RUN 1 and 64: identical bits between the two,
    and each the oracle's -- pcl::StatisticalOutlierRemoval restated, and NormalEstimation over the same handle's rows (NaN
    rows are NaN on both sides; between the two runs the NaNs' bits are compared as well).  Before each, the same calls over a
    decoy cloud (the points reversed and moved): the rows the handle keeps from the run before are then another cloud's."""
    a = u.self_knn_scene()
    res = {}
    with capi.Index(a, engine=capi.ENGINE_GRID) as ix:
        for run in (1, 64):
            ix.set_option(capi.OPT_KNN_RUN, run)
            for cloud in (u.decoy_of(a), a):
                omd, oinl, othr, okept = oracle.sor(cloud, 50, 1.5)
                ix.set_input(cloud)
                md, inl, thr, kept = ix.sor(50, 1.5)
                nm = ix.normals(50)
                rows, _ = ix.knn(cloud, 50)
                res[run] = (md, inl, thr, kept, nm, rows)
                assert (u.bits(md) == u.bits(omd)).all() and thr == othr and (inl == oinl).all() and kept == okept, run
                want = oracle.normals(cloud, 50, neighbours=rows)
                same = (u.bits(nm) == u.bits(want)).reshape(nm.shape) | (np.isnan(nm) & np.isnan(want))
                assert same.all(), (run, np.argwhere(~same)[:5])
    one, many = res[1], res[64]
    assert (u.bits(one[0]) == u.bits(many[0])).all() and (one[1] == many[1]).all() and one[2:4] == many[2:4]
    assert (u.bits(one[4]) == u.bits(many[4])).all() and (one[5] == many[5]).all()


# ---- C: where the k = 1 kernels put their workgroups ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", u.PLACEMENT_NQ)
def test_k1_placement_options(gpu, nq):
    """PCC_OPT_XCD_RUN x PCC_OPT_NN1_KERNEL x PCC_OPT_NN1_DENSE_MIN.  k_grid_nn1 and k_grid_nn1_flat2 renumber their workgroups
    in groups of 8 x run and leave the workgroups beyond the last full group alone; a renumbering that is no bijection loses
    queries and searches others twice.  The query counts (option_parity_util.PLACEMENT_NQ says which clause each makes live)
    give runs of 1, 2, 3 and 5 after the host's clamp and workgroup counts that are no multiple of 8 x run.  Every key must be
    written by the search under test: the keys live in a buffer of the handle that no call clears, so each search follows a
    decoy search of the same count whose answer differs in every row -- a query the remap lost keeps the decoy's key and fails
    the comparison.  The reference has one cell of thousands of equal points (dense waves) and clumps on a coarse lattice
    (sparse ones)."""
    ref = u.placement_scene()[0]
    with capi.Index(ref, engine=capi.ENGINE_GRID) as ix:
        for form in u.NN1_FORMS:
            for run in u.XCD_RUNS:
                for dense in u.DENSE_MINS:
                    ix.set_option(capi.OPT_NN1_KERNEL, form)
                    ix.set_option(capi.OPT_XCD_RUN, run)
                    ix.set_option(capi.OPT_NN1_DENSE_MIN, dense)
                    for decoy in (True, False):
                        gi, gd = u.filled((nq,))
                        ix.nn1(u.placement_queries(nq, decoy), out_idx=gi, out_d2=gd)
                        u.assert_same_rows(gi, gd, *u.placement_expected(nq, decoy),
                                           ("kernel", form, "run", run, "dense", dense, "decoy" if decoy else "queries"))


# ---- D: ICP ----------------------------------------------------------------------------------------------------------------------------
def _align(ix, src, **kw):
    T, fit, it, conv = ix.icp_align(src, **kw)
    return T.view(np.uint32).copy(), int(np.float64(fit).view(np.uint64)), it, conv


def _same_run(a, b):
    return (a[0] == b[0]).all() and a[1:] == b[1:]


@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("m", u.ICP_SOURCE_SIZES)
def test_icp_fused_solve_working_order_and_warm_start(gpu, m, fixed):
    """FUSE_PARAMS bit 2 (the last k_icp_sums workgroup solves the pass, icp.hip:423) x ICP_SORTED x ICP_WARM.  k_icp_sums takes
    2048 points per workgroup: 2048 is one workgroup -- the first to arrive is the last -- 2049 to 4096 two, 6000 three; the
    cell-ordered working set exists from 4096 points (icp.hip:360): below, ICP_SORTED changes nothing and all eight runs carry
    the same bits.  Within one ICP_SORTED value all four runs carry the same
    bits of T, fitness, iteration count and verdict; across it the order of the double sums differs, so each is compared with
    the oracle's loop as test_icp_align_options_do_not_change_a_bit does (its atol = 5e-5, equal iteration count)."""
    tgt, src = u.icp_scene(m)
    runs = {}
    with capi.Index(tgt, engine=capi.ENGINE_GRID) as ix:
        for order in (1, 0):
            for fuse in (0, 2):
                for warm in (1, 0):
                    ix.set_option(capi.OPT_ICP_SORTED, order)
                    ix.set_option(capi.OPT_FUSE_PARAMS, fuse)
                    ix.set_option(capi.OPT_ICP_WARM, warm)
                    runs[(order, fuse, warm)] = _align(ix, src, max_iter=12, fixed=fixed)
    oT, ofit, oit, _, _ = oracle.icp(src, tgt, max_iter=12, fixed=fixed)
    for order in (1, 0):
        first = runs[(order, 0, 1)]
        assert first[2] > 1
        for key, r in runs.items():
            if key[0] == order:
                assert _same_run(r, first), (key, r[2:], first[2:])
        if m < 4096:
            assert _same_run(first, runs[(1 - order, 0, 1)]), "ICP_SORTED acts below 4096 points"
        assert first[2] == oit, (order, first[2], oit)
        assert np.allclose(first[0].view(np.float32), oT, atol=5e-5), (order, np.abs(first[0].view(np.float32) - oT).max())


def test_icp_fused_solve_after_a_loop_that_stopped_on_the_device(gpu):
    """three aligns on one handle under FUSE_PARAMS = 2: a normal one, one of two source points -- fewer than 3 correspondences,
    the loop stops on the device with passes still enqueued -- and the first again, which must repeat its bits: neither the
    ticket word nor the loop state may carry anything over"""
    tgt, src = u.icp_scene(6000)
    with capi.Index(tgt, engine=capi.ENGINE_GRID) as ix:
        ix.set_option(capi.OPT_FUSE_PARAMS, 2)
        first = _align(ix, src, max_iter=8)
        T, fit, it, conv = ix.icp_align(src[:2], max_iter=8)
        assert not conv and it == 0 and np.array_equal(T, np.eye(4, dtype=np.float32))
        third = _align(ix, src, max_iter=8)
        ix.set_option(capi.OPT_FUSE_PARAMS, 0)
        plain = _align(ix, src, max_iter=8)
    assert first[2] > 1 and _same_run(third, first) and _same_run(plain, first)


def test_icp_fused_solve_at_the_row_cap(gpu):
    """983 041 source points are 481 rows of sums, capped at ICP_MAX_BLOCKS = 480: the most rows the solve ever stages, 65 280
    bytes of LDS, which the fused form needs beside k_icp_sums' own.  Three fixed passes on device-resident clouds, FUSE_PARAMS
    0 against 2: the same bits.  (The one large cloud of this file: the edge exists at no smaller size.)"""
    import torch
    tgt = torch.from_numpy(synth.corridor_cloud(20000, synth.SEED_A)).cuda()
    src = synth.corridor_cloud(u.ICP_ROW_CAP_POINTS, synth.SEED_B) + np.float32([0.01, -0.02, 0.005])
    src = torch.from_numpy(np.ascontiguousarray(src, dtype=np.float32)).cuda()
    runs = {}
    with capi.Index(tgt, engine=capi.ENGINE_GRID) as ix:
        for fuse in (0, 2, 0):
            ix.set_option(capi.OPT_FUSE_PARAMS, fuse)
            run = _align(ix, src, max_iter=3, fixed=True)
            assert _same_run(runs.setdefault(fuse, run), run)
    assert runs[0][2] == 3 and runs[0][3] and _same_run(runs[2], runs[0]), (runs[0][2:], runs[2][2:])


# ---- E: a build that runs out of memory --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse", [0, 1])
def test_a_failed_build_leaves_the_handle_usable(gpu, fuse):
    """pcc_debug_fail_alloc (the hook tests/test_comm_gpu.py uses) refuses the nth device allocation of a pcc_index_set_input
    with 20 000 points on a handle that holds another, smaller cloud: for nth = 1, 2, ... until the build gets through.  A
    failed build returns PCC_ERR_NOMEM, the handle then answers PCC_ERR_EMPTY instead of searching buffers of two clouds, and
    the next build on it -- with the fused derivation's ticket word wherever the failure left it -- matches the oracle.
    Host-side allocation failures only: no kernel is made to fail."""
    first, second, q = u.rebuild_clouds()
    oi, od = oracle.nn1_exhaustive(second, q)
    failed, built = 0, False
    for nth in range(1, 41):
        with capi.Index(first, engine=capi.ENGINE_GRID) as ix:
            ix.set_option(capi.OPT_FUSE_PARAMS, fuse)
            error = None
            try:
                capi.LIB.pcc_debug_fail_alloc(nth)
                try:
                    ix.set_input(second)
                except capi.PccError as e:
                    error = e
            finally:
                capi.LIB.pcc_debug_fail_alloc(0)
            if error is not None:
                failed += 1
                assert error.status == NOMEM and "injected" in str(error), (nth, str(error))
                with pytest.raises(capi.PccError) as e:
                    ix.nn1(q)
                assert e.value.status == EMPTY, (nth, str(e.value))
                ix.set_input(second)
            gi, gd = u.filled((len(q),))
            ix.nn1(q, out_idx=gi, out_d2=gd)
            u.assert_same_rows(gi, gd, oi, od, ("nth", nth, "failed" if error is not None else "built"))
            if error is None:
                built = True
                break
    assert built and failed >= 1, (failed, built)


# ---- F: the tie counters after a small call ------------------------------------------------------------------------------------------------
def test_small_call_in_lowest_index_order_reports_no_ties_of_an_earlier_search(gpu):
    """pcc_index_stats [5] and [6] speak of the last search.  A PCC_TIES_FLANN search over a small host cloud full of
    duplicates flags its tied queries; the lowest-index search after it (the one-launch small call: host queries, at most 4096
    exhaustively searched points, HOST_PIPE = 1) flags nothing and must not report the earlier count."""
    ref, q = u.tie_scene()
    oi, od = oracle.nn1_exhaustive(ref, q)
    with capi.Index(ref) as ix:
        assert ix.engine == capi.ENGINE_BRUTE and ix.get_option(capi.OPT_HOST_PIPE) == 1
        ix.set_tie_order(capi.TIES_FLANN)
        fi, fd = ix.nn1(q)
        assert ix.stats()[5] == len(q)                                     # every query's nearest reference exists three times
        assert (u.bits(fd) == u.bits(od)).all() and (ref[fi] == ref[oi]).all()
        ix.set_tie_order(capi.TIES_LOWEST_INDEX)
        gi, gd = u.filled((len(q),))
        ix.nn1(q, out_idx=gi, out_d2=gd)
        u.assert_same_rows(gi, gd, oi, od, "lowest index")
        st = ix.stats()
        assert st[5] == 0 and st[6] == 0, st
