"""What the scenes of tests/test_cellsort_levels_gpu.py must show, held without a GPU: every scene's predicate over the model of
tools/bucket_sizes.py (a scene that stops reaching its edge fails here, not silently on the GPU), the plan arithmetic against
values worked out by hand at its three boundaries, the slice model on a hand-made order, and that the model reads every
constant from the sources."""
import numpy as np
import pytest

import cellsort_levels_util as u
from cellsort_levels_util import bs


def test_every_constant_is_read_from_the_sources():
    names = ("MP_F2", "MP_B2", "MP_MAX_B1", "MP_MAX_G", "MP_WIN", "MP_SLICE2", "MP_STAGE_BYTES", "GRID_MAX_CELLS")
    assert set(bs.CONSTANTS) == set(names)
    assert all(isinstance(bs.CONSTANTS[k], int) and bs.CONSTANTS[k] > 0 for k in names)
    assert bs.GRID_MAX_CELLS == 1 << 26 and bs.SLICES == (bs.MP_STAGE_BYTES // 16, bs.MP_STAGE_BYTES // 8, bs.MP_SLICE2)
    with pytest.raises(LookupError):
        bs._constants("constexpr unsigned int MP_F2 = 2048;", ("MP_B2",))


def test_sort_plan_at_its_boundaries():
    """hand-computed from cellsort_mp.hip mp_plan with MP_F2 = 2048, MP_B2 = 128, MP_MAX_B1 = 256 (F1 = 262 144 = 2^18)"""
    assert (bs.MP_F2, bs.MP_B2, bs.MP_MAX_B1, bs.MP_MAX_G) == (2048, 128, 256, 512)
    # cap 262 143: (262 143 + 262 144) / 262 144 = 1 bucket; one more cell and entry [cap] needs a second
    assert bs.sort_plan(20000, 262143) == (2048, 262144, 1, 2, 10000)
    assert bs.sort_plan(20000, 262144) == (2048, 262144, 2, 2, 10000)
    # cap 2^26 - 1: 2048 * 128 * 256 = 2^26 is not below cap + 1, F2 stays, (2^26 - 1 + 2^18) / 2^18 = 256;
    # cap 2^26: F2 doubles, F1 = 2^19, (2^26 + 2^19) / 2^19 = 129
    assert bs.sort_plan(20000, (1 << 26) - 1) == (2048, 262144, 256, 2, 10000)
    assert bs.sort_plan(20000, (1 << 26) - 262144) == (2048, 262144, 256, 2, 10000)
    assert bs.sort_plan(20000, (1 << 26) - 262145) == (2048, 262144, 255, 2, 10000)
    assert bs.sort_plan(20000, 1 << 26) == (4096, 524288, 129, 2, 10000)
    # n 16 384: (16 384 + 16 383) / 16 384 = 1 workgroup; 16 385: 2 workgroups of ceil(16 385 / 2) = 8193
    assert bs.sort_plan(16384, 1 << 20)[3:] == (1, 16384)
    assert bs.sort_plan(16385, 1 << 20)[3:] == (2, 8193)
    assert bs.sort_plan(0, 4096)[3:] == (1, 0)
    assert bs.sort_plan(10_000_000, 1 << 25)[3:] == (512, 19532)       # the workgroup count stops at MP_MAX_G
    # the cap (grid.hip grid_nc_cap): 2 n / ppc + 4096, truncated, clamped
    assert bs.nc_cap(20000, 0.05) == 804096 and bs.nc_cap(20000, 0.004) == 10004096
    assert bs.nc_cap(20000, 0.00059) == 1 << 26 and bs.nc_cap(32_000_000) == 1 << 26 and bs.nc_cap(25_000_000) < 1 << 26


def test_slice_windows_on_a_hand_made_order():
    assert bs.MP_WIN == 8
    #        slice 0: buckets 0 0 3 7 | slice 1: 7 8 15 16 | slice 2: 16 40 (a short last slice)
    b1 = np.array([0, 0, 3, 7, 7, 8, 15, 16, 16, 40])
    distinct, beyond = bs.slice_windows(b1, 4)
    assert distinct.tolist() == [3, 4, 2]
    assert beyond.tolist() == [0, 2, 1]          # 15 - 7 = 8 and 16 - 7 = 9 lie beyond; 40 - 16 too; 7 - 0 does not
    distinct, beyond = bs.slice_windows(b1, 16)
    assert distinct.tolist() == [7] and beyond.tolist() == [5]
    distinct, beyond = bs.slice_windows(np.zeros(9, int), 4)
    assert distinct.tolist() == [1, 1, 1] and beyond.tolist() == [0, 0, 0]


@pytest.mark.parametrize("name", u.SCENES)
def test_scene_shows_what_it_is_about(name):
    sc, m = u.scene(name), u.model(name)
    seen = (name, tuple(m.plan), m.cap, m.ncells, m.occupied, m.highest, m.max_jump, m.beyond, m.beyond_q)
    assert sc.shows(m), ("the scene does not show what it is about", seen)
    assert 16000 <= len(sc.ref) <= 30000 and 16000 <= len(sc.qry) <= 30000
    assert m.ncells <= m.cap and m.plan.B1 > 1
    for p in (sc.ref, sc.qry):
        assert not p.flags.writeable and p.dtype == np.float32
        finite = np.isfinite(p).all(1)
        assert (len(p) - 13) // u.NONFINITE_EVERY - 2 <= (~finite).sum() <= (len(p) - 13) // u.NONFINITE_EVERY + 1
        assert (p[finite].min(0) == sc.ref[np.isfinite(sc.ref).all(1)].min(0)).all()      # both clouds span the same box:
        assert (p[finite].max(0) == sc.ref[np.isfinite(sc.ref).all(1)].max(0)).all()      # its corners are among their points
    # a radius count looks at no more than about 30 cells an axis
    assert 2.0 * sc.radius / float(m.grid[0]) <= 30.0, seen


def test_full_and_wide_are_one_cloud_under_two_plans():
    assert u.scene("full").ref is not u.scene("wide").ref and (u.scene("full").ref.view(np.uint32) == u.scene("wide").ref.view(np.uint32)).all()
    assert u.model("full").plan.F2 * 2 == u.model("wide").plan.F2


def test_the_sheet_is_the_candidate_that_reaches_highest():
    highest = {t: u.sheet_highest(t) for t in u.SHEET_CANDIDATES}
    assert max(highest, key=highest.get) == u.SHEET_THICKNESS and highest[u.SHEET_THICKNESS] >= 160, highest


def test_voxel_and_cluster_scenes_reach_their_plans():
    rec = u.voxel_cloud()
    assert 19000 <= len(rec) <= 21000 and not np.isfinite(rec[:, :3]).all()
    coarse, fine = (int(u.voxel_lattice(rec, leaf).prod()) for leaf in u.VOXEL_LEAVES)
    assert 262144 < coarse <= 2 << 20 and 1 < bs.sort_plan(len(rec), coarse).B1 <= 16
    assert bs.GRID_MAX_CELLS - 262144 < fine <= bs.GRID_MAX_CELLS and bs.sort_plan(len(rec), fine)[:3] == (bs.MP_F2, bs.MP_F2 * bs.MP_B2, bs.MP_MAX_B1)
    # the lattice's last voxel holds a point: the last level-1 bucket is the one with entry [ncells - 1] and [ncells]
    assert (rec[-1, :3] == rec[np.isfinite(rec[:, :3]).all(1), :3].max(0)).all()
    # every coordinate a multiple of 2^-10 below 2: float64 sums of any voxel are exact
    xyz = rec[np.isfinite(rec[:, :3]).all(1), :3].astype(np.float64) * 1024
    assert (xyz == np.round(xyz)).all() and np.abs(xyz).max() <= 1024
    pts = u.cluster_cloud()
    cells = u.cluster_grid_cells(pts, u.CLUSTER_TOLERANCE)
    assert len(pts) == 20000 and 4 << 20 < cells <= 1 << 26 and bs.sort_plan(len(pts), cells).B1 > 64, cells   # (cluster.hip: cells <= 2^26)
