"""Levels 1 and 2 of the three-level cell sort (cellsort_mp.hip) and its widest plan, on clouds of 16 000 to 30 000 points.

tests/test_cellsort_fine_gpu.py holds the sort's last level to the oracle; its grids have fewer than 262 144 cells, so level 1
sorts into ONE bucket and level 2 sees one level-1 bucket per slice.  Here PCC_OPT_GRID_PPC makes the grid sparse -- up to the
clamp of 2^26 cells -- and PCC_OPT_SORT_MP_MIN / _Q = 1000 sends the small clouds through the sort: several to 256 level-1
buckets (k_mp_hist1, the scatter cursors, k_mp_scatter1_staged's scan over 256 tile counts), slices of level 2 that span more
level-1 buckets than their LDS window (k_mp_level2's branch straight to memory, which the counting and the placing form take
for different elements), F2 = 4096 at the clamp, a level-1 slice that ends inside a load group.  cellsort_levels_util.py has
the scenes and says which host condition (mp_plan, grid_nc_cap) puts each on its route; test_cellsort_levels_cpu.py pins that
every scene still shows its edge.  The route itself cannot be observed.

Every comparison is bit for bit (indices equal, float32 values equal as uint32): with the exhaustive engine, with the same
handle's two-level sort, with the oracle.  Two calls in a row on a handle never ask the same rows of the same queries: a row
that a search skips keeps what the call before left in the handle's buffers (option_parity_util.decoy_of)."""
import numpy as np
import pytest

import oracle
import cellsort_levels_util as u
import voxel_util
from option_parity_util import FILL_IDX, assert_same_counts, assert_same_rows, bits, filled, knn_oracle
from voxel_ref import voxel_grid_ref

pytestmark = pytest.mark.gpu

MP_MIN = 1000                                    # PCC_OPT_SORT_MP_MIN / _Q: every cloud here takes the three-level sort


def _knn_into(ix, q, k):
    """ix.knn into sentinel-filled arrays"""
    from pointcloudcomparator_amd import capi
    ptr, n, stride, mem = capi._points(q)
    idx, d2 = filled((n, k))
    capi._check(capi.LIB.pcc_knn(ix._h, ptr, n, stride, mem, k, idx.ctypes.data, d2.ctypes.data))
    return idx, d2


def _radius_count_into(ix, q, radius):
    from pointcloudcomparator_amd import capi
    ptr, n, stride, mem = capi._points(q)
    cnt = np.full(n, FILL_IDX, np.int32)
    capi._check(capi.LIB.pcc_radius_count_max(ix._h, ptr, n, stride, mem, float(radius), 0, cnt.ctypes.data))
    return cnt


def _four_calls(ix, q_in, r_in, sample, radius):
    """k = 1 of the queries, k = 1 of the references, k = 8 and a radius count of the sample, all into filled arrays"""
    i1, d1 = filled((len(q_in),))
    ix.nn1(q_in, i1, d1)
    i2, d2 = filled((len(r_in),))
    ix.nn1(r_in, i2, d2)
    return (i1, d1), (i2, d2), _knn_into(ix, sample, 8), _radius_count_into(ix, sample, radius)


def _three_level(ix, largest):
    """from here on the handle sorts every cloud of MP_MIN points or more in three levels; until here it sorted them in two"""
    from pointcloudcomparator_amd import capi
    assert ix.get_option(capi.OPT_SORT_MP_MIN) > largest and ix.get_option(capi.OPT_SORT_MP_MIN_Q) > largest
    ix.set_option(capi.OPT_SORT_MP_MIN, MP_MIN)
    ix.set_option(capi.OPT_SORT_MP_MIN_Q, MP_MIN)


def _assert_same_sor(got, want, what):
    md, inl, thr, kept = got
    omd, oinl, othr, okept = want
    assert (bits(md) == bits(omd)).all(), (what, "mean distances differ", np.flatnonzero(bits(md) != bits(omd))[:5])
    assert thr == othr and kept == okept and (inl == oinl).all(), what


@pytest.mark.parametrize("name", u.SCENES)
def test_three_level_sort_upper_levels(gpu, name):
    from pointcloudcomparator_amd import capi
    sc, m = u.scene(name), u.model(name)
    assert sc.shows(m), (name, "the cloud does not show what the case is about")
    wide = u.SCENES.index(name) % 2 == 1
    r_in, q_in = u.strided(sc.ref, wide), u.strided(sc.qry, not wide)
    sample = u.sample_of(sc.qry)
    with capi.Index(r_in, engine=capi.ENGINE_BRUTE) as bx:
        want_q, want_r = bx.nn1(q_in), bx.nn1(r_in)
    stage1 = {}
    with capi.Index(r_in, engine=capi.ENGINE_GRID) as ix:
        ix.set_option(capi.OPT_GRID_PPC, sc.ppc)
        ix.set_option(capi.OPT_GRID_TRIM, 0)
        ix.set_input(r_in)                               # 1. the two-level sort (cellsort.hip: F clamped at 24 576, 2731 buckets at the clamp)
        two = _four_calls(ix, q_in, r_in, sample, sc.radius)
        assert ix.stats()[3] == m.ncells, (name, "the model's grid is not the handle's", ix.stats()[3], m.ncells)
        sor_two = ix.sor(8, 1.0)
        part_two = ix.sor_partial(1, len(r_in) - 1, 8)[0]
        _three_level(ix, len(r_in))                      # 2. the three-level sort, of the references and of every query cloud
        ix.set_input(r_in)
        three = _four_calls(ix, q_in, r_in, sample, sc.radius)
        assert ix.stats()[3] == m.ncells
        # the indexed cloud asks about itself: the WHOLE cloud takes the order of the index (grid.hip grid_sort_queries: no sort, so
        # this holds the three-level build's cell_refs to account); all but its first point are a query cloud that the pack kernel
        # left no cells for: the pair scatter k_mp_scatter1<uint2> works them out from the points
        sor_three = ix.sor(8, 1.0)
        part_three = ix.sor_partial(1, len(r_in) - 1, 8)[0]
        if name in u.STAGE1_SCENES:                      # 3. level 1's scatter: plain, in sorted tiles for points, for pairs too
            for v in (0, 1, 2):
                ix.set_option(capi.OPT_SORT_STAGE1, v)
                ix.set_input(r_in)
                i1, d1 = filled((len(q_in),))
                ix.nn1(q_in, i1, d1)
                i2, d2 = filled((len(r_in),))
                ix.nn1(r_in, i2, d2)
                stage1[v] = ((i1, d1), (i2, d2), ix.sor_partial(1, len(r_in) - 1, 8)[0])
    assert_same_rows(*three[0], *want_q, (name, "k = 1 of the queries against the exhaustive engine"))
    # a reference that a level loses, doubles or files under the wrong cell is not found at distance 0 in its own cell; among
    # equal points the index is the exhaustive engine's
    assert_same_rows(*three[1], *want_r, (name, "k = 1 of the references against the exhaustive engine"))
    for k, what in enumerate(("k = 1 of the queries", "k = 1 of the references", "k = 8 of the sample")):
        assert_same_rows(*three[k], *two[k], (name, what + " against the two-level sort"))
    assert_same_counts(three[3], two[3], (name, "radius count against the two-level sort"))
    assert_same_rows(*three[2], *knn_oracle(sc.ref, sample, 8), (name, "k = 8 against the oracle"))
    assert_same_counts(three[3], oracle.radius_count_exhaustive(sc.ref, sample, sc.radius), (name, "radius count against the oracle"))
    for v, (rows_q, rows_r, part) in stage1.items():
        assert_same_rows(*rows_q, *want_q, (name, "SORT_STAGE1", v, "k = 1 of the queries"))
        assert_same_rows(*rows_r, *want_r, (name, "SORT_STAGE1", v, "k = 1 of the references"))
        assert (bits(part) == bits(part_three)).all(), (name, "SORT_STAGE1", v, "mean distances of a part of the cloud")
    want_sor = oracle.sor(sc.ref, 8, 1.0)
    _assert_same_sor(sor_three, want_sor, (name, "SOR against the oracle"))
    _assert_same_sor(sor_three, sor_two, (name, "SOR against the two-level sort"))
    assert (bits(part_three) == bits(want_sor[0][1:])).all(), (name, "mean distances of a part of the cloud against the oracle")
    assert (bits(part_three) == bits(part_two)).all(), (name, "mean distances of a part of the cloud against the two-level sort")


@pytest.mark.parametrize("leaf", u.VOXEL_LEAVES)
def test_voxel_grid_through_the_three_level_sort(gpu, leaf):
    """voxel.hip:133 sorts by voxel with the lattice's cell count as the cap: 2^20 voxels (B1 = 5) and 511 x 512 x 256 (B1 = 256, the
    lattice's last voxel occupied).  A dyadic cloud: the reference's bytes."""
    from pointcloudcomparator_amd import capi
    rec = u.voxel_cloud()
    rows, _ = voxel_grid_ref(rec, leaf, True)
    with capi.Index(np.arange(192, dtype=np.float32).reshape(64, 3)) as ix:
        default = voxel_util.call(ix, rec, leaf)
        _three_level(ix, len(rec))
        three = voxel_util.call(ix, rec, leaf)
        bare = voxel_util.call(ix, rec, leaf, has_rgb=False, in_stride=12, out_stride=12)
    voxel_util.assert_equals_reference(three, rows, 32, True, False, (leaf, "three-level"))
    voxel_util.assert_equals_reference(default, rows, 32, True, False, (leaf, "default sizes"))
    assert three[1] == default[1] and (three[2] == default[2]).all(), (leaf, "three-level against default sizes")
    voxel_util.assert_equals_reference(bare, voxel_grid_ref(rec, leaf, False)[0], 12, False, False, (leaf, "three-level, 12-byte rows"))


@pytest.mark.parametrize("form", [3, 1])
def test_euclidean_clusters_through_the_three_level_sort(gpu, form):
    """cluster.hip:762 sorts the indexed cloud by the cells of the clique-cell grid, here 400^3 = 64M of them (B1 = 245); PCC_OPT_EC_CELLS
    3 = union-find over the cells, 1 = one parent per point"""
    from pointcloudcomparator_amd import capi
    pts = u.cluster_cloud()
    ol, on, osz = oracle.euclidean_clusters(pts, u.CLUSTER_TOLERANCE, u.CLUSTER_MIN, u.CLUSTER_MAX)
    assert on >= 50
    with capi.Index(pts) as ix:
        ix.set_option(capi.OPT_EC_CELLS, form)
        default = ix.euclidean_clusters(u.CLUSTER_TOLERANCE, u.CLUSTER_MIN, u.CLUSTER_MAX)
        _three_level(ix, len(pts))
        ix.set_input(pts)
        three = ix.euclidean_clusters(u.CLUSTER_TOLERANCE, u.CLUSTER_MIN, u.CLUSTER_MAX)
    for (labels, ncl, sizes), what in ((three, "three-level"), (default, "default sizes")):
        assert ncl == on, (form, what, ncl, on)
        assert (sizes == osz).all(), (form, what)
        assert (labels == ol).all(), (form, what, np.flatnonzero(labels != ol)[:5])
