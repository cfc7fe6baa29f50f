"""Scenes of tests/test_cellsort_levels_gpu.py: small clouds on SPARSE grids, which put the three-level cell sort
(cellsort_mp.hip) on the plans and branches of its levels 1 and 2 that otherwise only clouds of millions of points reach.
tests/test_cellsort_levels_cpu.py pins, without a GPU, what every scene must show.

The route a sort takes cannot be observed; it follows from host conditions, which tools/bucket_sizes.py restates:
  grid.hip grid_nc_cap         cap = min(2 n / ppc + 4096, GRID_MAX_CELLS = 2^26)
  cellsort_mp.hip mp_plan      F2 = MP_F2 = 2048, doubled while F2 * MP_B2 * MP_MAX_B1 < cap + 1;  B1 = ceil((cap + 1) / (F2 * MP_B2))
                               (cap < 262 144: B1 = 1;  cap in [2^26 - 262 144, 2^26): B1 = 256;  cap = 2^26: F2 = 4096, B1 = 129)
                               G1 = ceil(n / 16 384) workgroups in level 1, slice1 = ceil(n / G1)
  cellsort_mp.hip k_mp_level2  a slice (8192 elements counting, 2048 points or 4096 pairs placing) keeps LDS counters for the
                               MP_WIN = 8 level-1 buckets from that of its first element on; an element of a later bucket is
                               counted and placed through global memory
Every scene is a reference cloud and a query cloud over the same box, both with its two corners, shuffled, a non-finite row
every 97, frozen.  A scene's predicate takes model(name) and says what the scene is about."""
import functools
import sys
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import bucket_sizes as bs  # noqa: E402

BOX = np.array([0.5, 0.25, 1.0], np.float32)   # x second, y shortest, z longest: layers along z
NONFINITE_EVERY = 97
SAMPLE = 2000                                    # queries that k = 8 and the radius count are asked for
PPC_FEW = 0.05                                   # cap 804 096 at 20 000 points: B1 = 4
PPC_EDGE = 0.004                                 # cap 10 004 096: B1 = 39


def ppc_full(n):
    """the occupancy that puts the cap of n points in the middle of [2^26 - 262 144, 2^26): F2 = 2048, B1 = 256"""
    return 2.0 * n / (bs.GRID_MAX_CELLS - 131072 - 4096)


def ppc_wide(n):
    """a little sparser: 2 n / ppc + 4096 > 2^26, the cap is the clamp, F2 = 4096, B1 = 129"""
    return 0.99 * 2.0 * n / (bs.GRID_MAX_CELLS - 4096)


# the sheet's thickness: of these the one whose grid puts a point in the highest level-1 bucket -- the thinnest that still has two
# cells across, so that the per-dimension round-up doubles the cell count and uses nearly all of the cap's headroom
SHEET_CANDIDATES = (0.0001, 0.00011, 0.00012, 0.000125, 0.00013, 0.00015, 0.0002, 0.0003, 0.0005, 0.001)
SHEET_THICKNESS = 0.000125
S_PTS, S_ORD, S_CNT = bs.SLICES                  # a level-2 slice: placing points, placing pairs, counting


def _cloud(n, seed, box=BOX, lo=(0, 0, 0), hi=(1, 1, 1)):
    """n uniform points in the part [lo, hi] of the box, the box's two corners among them"""
    rng = np.random.default_rng([0x1E7E1, seed])
    lo, hi = np.array(lo, np.float32), np.array(hi, np.float32)
    p = (lo + rng.random((n, 3), dtype=np.float32) * (hi - lo)) * box
    p[0], p[1] = 0, box
    return p


def _finish(p, seed, box=BOX):
    """shuffled, then a non-finite row every 97 (never a corner of the box), frozen"""
    rng = np.random.default_rng([0x1E7E2, seed])
    p = np.ascontiguousarray(p[rng.permutation(len(p))], dtype=np.float32)
    keep = (p == 0).all(1) | (p == box).all(1)
    for j, i in enumerate(range(13, len(p), NONFINITE_EVERY)):
        if not keep[i]:
            p[i, j % 3] = (np.nan, np.inf, -np.inf)[j % 3]
    p.setflags(write=False)
    return p


def _slabs(n, seed, box=BOX):
    """two slabs, z below 0.3 and above 0.7 of the box, nothing between them"""
    return np.concatenate([_cloud(n // 2, seed, box, hi=(1, 1, 0.3)), _cloud(n - n // 2, seed + 1, box, lo=(0, 0, 0.7))[::-1]])


def sheet_box(thickness):
    return np.array([BOX[0], thickness, BOX[2]], np.float32)


def sheet_highest(thickness):
    """the highest level-1 bucket that a reference of the sheet scene occupies at that thickness"""
    box = sheet_box(thickness)
    ref = _finish(_cloud(20000, 15, box), 0, box)
    return int(level1_highest(ref, ppc_full(20000)))


def level1_highest(ref, ppc):
    return bs.level1_buckets(ref, bs.grid_of(ref, ppc))[-1]


def _radius(ref, ppc):
    """the radius of the counts: the ball's box stays within 27 cells an axis, and 0.02 on the coarser grids"""
    return float(np.float32(min(0.02, 13.0 * float(bs.grid_of(ref, ppc)[0]))))


Scene = types.SimpleNamespace


@functools.lru_cache(maxsize=None)
def scene(name):
    """ref, qry (read-only float32 (n, 3)), ppc, radius, shows(model) -> bool"""
    kind, _, arg = name.partition(":")
    box = BOX
    if kind == "few":
        ref, qry, ppc = _cloud(20000, 1), _cloud(20000, 2), PPC_FEW
        shows = lambda m: 1 < m.plan.B1 <= 16 and m.plan.F2 == bs.MP_F2 and m.occupied >= 2 and m.occupied_q >= 2 and \
            not any(m.beyond.values()) and not any(m.beyond_q.values())
    elif kind == "edge":
        ref, qry, ppc = _cloud(20000, 3), _cloud(20000, 4), PPC_EDGE
        # the counting form sees elements beyond its window that the placing forms do not: the cursors must agree all the same
        shows = lambda m: m.beyond[S_CNT] > 0 and m.beyond[S_PTS] == 0 and m.beyond[S_ORD] == 0 and \
            m.beyond_q[S_CNT] > 0 and m.beyond_q[S_PTS] == 0 and m.beyond_q[S_ORD] == 0
    elif kind in ("full", "wide"):                # one cloud under two plans
        ref, qry, ppc = _cloud(20000, 5), _cloud(20000, 6), ppc_full(20000) if kind == "full" else ppc_wide(20000)
        if kind == "full":
            shows = lambda m: m.plan.B1 == bs.MP_MAX_B1 and m.plan.F2 == bs.MP_F2 and bs.GRID_MAX_CELLS - 262144 < m.cap < bs.GRID_MAX_CELLS and \
                all(m.beyond.values()) and all(m.beyond_q.values())
        else:
            shows = lambda m: m.cap == bs.GRID_MAX_CELLS and m.plan.F2 == 2 * bs.MP_F2 and m.plan.B1 == 129 and m.occupied > bs.MP_WIN and \
                m.beyond[S_CNT] > 0 and m.beyond_q[S_CNT] > 0
    elif kind == "gap":
        ref, qry, ppc = _slabs(20000, 7), _slabs(20000, 9), ppc_full(20000)
        # a slice that straddles the gap: one step of more than MP_WIN level-1 buckets between two neighbours in the order
        shows = lambda m: m.plan.B1 == bs.MP_MAX_B1 and m.plan.F2 == bs.MP_F2 and m.max_jump > 5 * bs.MP_WIN and m.max_jump_q > 5 * bs.MP_WIN
    elif kind == "pile":
        at, clump_at = BOX * np.float32(0.5), BOX * np.array([0.4, 0.6, 0.1533], np.float32)

        def build(seed):
            rng = np.random.default_rng([0x1E7E3, seed])
            clump = clump_at + (rng.random((17500, 3), dtype=np.float32) - np.float32(0.5)) * np.array([0.2, 0.1, 0.0015], np.float32)
            return np.concatenate([_slabs(6000, seed), np.repeat(at[None], 3000, 0), clump])
        ref, qry, ppc = build(11), build(13), ppc_full(26500)

        def shows(m):
            ok = m.plan.B1 == bs.MP_MAX_B1
            for pts, counts, b1, beyond in ((m.pts, m.counts, m.b1, m.beyond), (m.pts_q, m.counts_q, m.b1_q, m.beyond_q)):
                b = int(bs.cells_of(at[None], m.grid)[0]) // m.plan.F1
                heavy = int(np.argmax(counts))
                near = counts[heavy + 1:heavy + 1 + bs.MP_WIN]
                copies = int((pts == at).all(1).sum())                  # (3000 less the rows made non-finite)
                ok = ok and copies > 2900 and counts[b] == copies       # the pile's cell is all its level-1 bucket holds
                ok = ok and counts[heavy] >= 2 * S_CNT and near.min() > 0 and near.sum() < S_PTS   # a whole counting slice inside, then eight that fill none
                for s in bs.SLICES:                                     # slices inside one bucket and slices beyond their window
                    distinct, bey = bs.slice_windows(b1, s)
                    ok = ok and (distinct == 1).any() and beyond[s] > 0 and (bey > 0).any()
            return ok
    elif kind == "sheet":
        box = sheet_box(SHEET_THICKNESS)
        ref, qry, ppc = _cloud(20000, 15, box), _cloud(20000, 16, box), ppc_full(20000)
        shows = lambda m: m.plan.B1 == bs.MP_MAX_B1 and m.plan.F2 == bs.MP_F2 and m.highest >= 160 and m.highest_q >= 160
    elif kind == "g1":                            # 16 384: one level-1 workgroup; 16 385: two, of 8193 and 8192 points -- the first
        n = int(arg)                              # slice ends inside a load group of four
        ref, qry, ppc = _cloud(n, 17), _cloud(n, 18), ppc_full(n)
        want = {16384: (1, 16384), 16385: (2, 8193)}[n]
        shows = lambda m: m.plan.B1 > 64 and (m.plan.G1, m.plan.slice1) == want and (m.plan_q.G1, m.plan_q.slice1) == want and m.occupied > 64
    else:
        raise KeyError(name)
    seed = sum(map(ord, "full" if kind == "wide" else name))
    ref, qry = _finish(ref, seed, box), _finish(qry, seed + 1, box)
    return Scene(name=name, ref=ref, qry=qry, ppc=ppc, radius=_radius(ref, ppc), shows=shows)


SCENES = ["few", "edge", "full", "wide", "gap", "pile", "sheet", "g1:16384", "g1:16385"]
STAGE1_SCENES = ["full", "pile"]                 # the scenes every PCC_OPT_SORT_STAGE1 value is run on


@functools.lru_cache(maxsize=None)
def model(name):
    """what tools/bucket_sizes.py says of the scene: the reference cloud's grid and cap, the plans of the two sorts, and per
    cloud (the queries' with _q) the points of every level-1 bucket, how many are occupied and the highest of them, the
    largest step between neighbours of the grouped order, and the elements beyond the window per slice length"""
    sc = scene(name)
    g = bs.grid_of(sc.ref, sc.ppc)
    m = types.SimpleNamespace(grid=g, cap=g[5], ncells=int(g[2].prod()), plan=bs.sort_plan(len(sc.ref), g[5]), plan_q=bs.sort_plan(len(sc.qry), g[5]))
    for tag, pts in (("", sc.ref), ("_q", sc.qry)):
        b1 = bs.level1_buckets(pts, g)
        setattr(m, "pts" + tag, pts)
        counts = np.bincount(b1, minlength=m.plan.B1)
        setattr(m, "b1" + tag, b1)
        setattr(m, "counts" + tag, counts)
        setattr(m, "occupied" + tag, int((counts > 0).sum()))
        setattr(m, "highest" + tag, int(b1[-1]))
        setattr(m, "max_jump" + tag, int(np.diff(b1).max()))
        setattr(m, "beyond" + tag, {s: int(bs.slice_windows(b1, s)[1].sum()) for s in bs.SLICES})
    assert len(m.counts) == m.plan.B1, "a cell beyond the cap"
    return m


def strided(p, wide):
    """12-byte records, or 32-byte ones (x, y, z and five words no search may read)"""
    if not wide:
        return np.ascontiguousarray(p[:, :3])
    out = np.full((len(p), 8), np.nan, np.float32)
    out[:, :3] = p[:, :3]
    return out


def sample_of(qry):
    """the fixed sample of the queries: 12-byte rows, the first and the last query among them"""
    return np.ascontiguousarray(qry[np.linspace(0, len(qry) - 1, min(SAMPLE, len(qry))).astype(int)])


# ---- the two callers with a grid of their own -----------------------------------------------------------------------------
# pcc_voxel_grid (voxel.hip) sorts by voxel and gives the sort the lattice's TRUE cell count as its cap, so the last level-1
# bucket is occupied and holds entry [ncells]; pcc_euclidean_clusters (cluster.hip grid_clusters) sorts the indexed cloud by the
# cells of its clique-cell grid, edge 0.57 tolerance, when that grid has at most 2^26 cells.
VOXEL_LEAVES = (2.0 ** -6, 2.0 ** -8)            # lattices of 128 x 128 x 64 (B1 = 5) and 511 x 512 x 256 voxels (B1 = 256)
VOXEL_LO, VOXEL_HI = (-1024, -1024, -512), (1019, 1023, 511)   # in units of 2^-10


@functools.lru_cache(maxsize=None)
def voxel_cloud():
    """20 002 32-byte records (x, y, z, 1, rgb) in the manner of tests/voxel_util.py: dyadic coordinates, multiples of 2^-10 -- many
    on voxel faces, both signs --, so every float64 sum is exact and tests/voxel_ref.py is the specified result.  14 000 scattered,
    2 000 spots of three within 3 * 2^-10 of each other (voxels of more than one point at the finer leaf too), the two corners that
    fix the lattice, a non-finite row every 97."""
    from voxel_util import records
    rng = np.random.default_rng(0x1E7E4)
    lo, hi = np.array(VOXEL_LO), np.array(VOXEL_HI)
    scattered = rng.integers(lo, hi + 1, (14000, 3))
    spots = np.minimum(np.repeat(rng.integers(lo, hi + 1, (2000, 3)), 3, axis=0) + rng.integers(0, 4, (6000, 3)), hi)
    units = np.concatenate([scattered, spots])[rng.permutation(20000)]
    xyz = (np.concatenate([lo[None], units, hi[None]]).astype(np.float64) * 2.0 ** -10).astype(np.float32)
    rec = records(xyz, rng)
    rec[13:-1:NONFINITE_EVERY, 1] = np.nan
    rec.setflags(write=False)
    return rec


def voxel_lattice(rec, leaf):
    """voxels along x, y, z of PCL's lattice (voxel_plan.hpp: floor(max * inverse_leaf) - floor(min * inverse_leaf) + 1, in float)"""
    p = rec[np.isfinite(rec[:, :3]).all(1), :3]
    inv = np.float32(1.0) / np.float32(leaf)
    return (np.floor(p.max(0) * inv) - np.floor(p.min(0) * inv) + 1).astype(np.int64)


CLUSTER_TOLERANCE = 0.0044                       # clique cells of edge 0.0025: 400^3 = 64M of them over the unit box
CLUSTER_MIN, CLUSTER_MAX = 20, 25000


@functools.lru_cache(maxsize=None)
def cluster_cloud():
    """20 000 points in the unit box: 60 tight blobs of 100 to 400 points (sigma 0.0008: every blob one cluster at the tolerance),
    uniform scatter for the rest (nearly all alone, below the minimum size), the box's corners, a non-finite row every 97"""
    rng = np.random.default_rng(0x1E7E5)
    sizes = rng.integers(100, 401, 60)
    centres = 0.05 + 0.9 * rng.random((60, 3))
    blobs = np.concatenate([c + rng.normal(0, 0.0008, (k, 3)) for c, k in zip(centres, sizes)])
    p = np.concatenate([blobs, rng.random((20000 - len(blobs), 3))]).astype(np.float32)
    p = p[rng.permutation(len(p))]
    p[0], p[1] = 0, 1
    p[13::NONFINITE_EVERY, 2] = np.nan
    p = np.ascontiguousarray(p)
    p.setflags(write=False)
    return p


def cluster_grid_cells(pts, tolerance):
    """cells of the clique-cell grid (cluster.hip grid_clusters: edge 0.57f * tolerance in float, ext / h + 2 cells an axis)"""
    p = pts[np.isfinite(pts).all(1)]
    h = np.float32(tolerance) * np.float32(0.57)
    ext = p.max(0).astype(np.float64) - p.min(0).astype(np.float64)
    return int(np.prod(np.minimum(ext / np.float64(h) + 2.0, 2.0e9).astype(np.int64)))
