"""The last level of the three-level cell sort (cellsort_mp.hip, k_mp_fine): buckets of at most LIGHT elements are sorted by
one wave each, four to a workgroup; up to four times as many by a whole workgroup from one read; the others as before.  Small clouds reach that LEVEL through
PCC_OPT_SORT_MP_MIN / _Q = 1000 -- its last level only: every grid here has fewer than 262 144 cells, so level 1 sorts into one
bucket and level 2 sees one level-1 bucket per slice (tests/test_cellsort_levels_gpu.py has the upper levels); PCC_OPT_GRID_PPC shapes the cells and PCC_OPT_GRID_TRIM = 0 lays the grid over the true
bounding box, which is what tools/bucket_sizes.py models: every case states what its buckets hold from that model and checks
the model's cell count against the handle's.

Every case sorts a reference cloud (16-byte points travel) and a query cloud (order words), one with 12-byte and one with
32-byte records, both with non-finite rows, and checks bit for bit (indices equal, float32 values equal as uint32):
k = 1 against the exhaustive engine, k = 1 / k = 8 / a radius count against the same handle's two-level sort, and k = 8 and
the radius count of a sample of the queries against the oracle."""
import functools
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle
from option_parity_util import assert_same_counts, assert_same_rows, filled, knn_oracle

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
from bucket_sizes import F2, bucket_sizes, cells_of, grid_of  # noqa: E402

pytestmark = pytest.mark.gpu

_SRC = (ROOT / "pointcloudcomparator_amd" / "csrc" / "cellsort_mp.hip").read_text()
LIGHT_PTS = int(re.search(r"#define PCC_MP_LIGHT_PTS (\d+)", _SRC).group(1))   # reference clouds
LIGHT_ORD = int(re.search(r"#define PCC_MP_LIGHT_ORD (\d+)", _SRC).group(1))   # query clouds
STAGE_PTS = int(re.search(r"#define PCC_MP_STAGE_PTS (\d+)", _SRC).group(1))   # the whole-workgroup form's LDS stage
STAGE_ORD = int(re.search(r"#define PCC_MP_STAGE_ORD (\d+)", _SRC).group(1))
BOX = np.array([0.5, 0.25, 1.0], np.float32)   # x second, y shortest, z longest: layers along z
NONFINITE_EVERY = 97
SAMPLE = 300                                     # queries the oracle answers for k = 8 and the radius count


def _box(n, seed, lo=(0, 0, 0), hi=(1, 1, 1)):
    rng = np.random.default_rng([0xCE11, seed])
    lo, hi = np.array(lo, np.float32), np.array(hi, np.float32)
    p = (lo + rng.random((n, 3), dtype=np.float32) * (hi - lo)) * BOX
    p[0], p[1] = 0, BOX      # the bounding box is the box itself, whatever else a case adds
    return p


def _finish(p, seed):
    """shuffled, then a non-finite row every 97 (never the box corners, which sit anywhere after the shuffle: the box is
    taken again from the finite rows by whoever models the grid)"""
    rng = np.random.default_rng([0xCE12, seed])
    p = np.ascontiguousarray(p[rng.permutation(len(p))], dtype=np.float32)
    keep = (p == 0).all(1) | (p == BOX).all(1)
    for j, i in enumerate(range(13, len(p), NONFINITE_EVERY)):
        if not keep[i]:
            p[i, j % 3] = (np.nan, np.inf, -np.inf)[j % 3]
    p.setflags(write=False)
    return p


def _mix(p, extra, seed):
    """extra rows dealt into p at random places"""
    rng = np.random.default_rng([0xCE13, seed])
    out = np.ascontiguousarray(np.concatenate([p, np.asarray(extra, np.float32)])[rng.permutation(len(p) + len(extra))])
    out.setflags(write=False)
    return out


SPARE = 400


def _clump_in(p, at, grid_for, want, spread, seed):
    """p plus a clump around `at` sized so that the bucket of `at` holds exactly `want` finite points in grid_for(cloud).
    What the clump does not take of SPARE more points goes to a corner far away: the cloud's size, and with it its own
    grid, does not move with the clump's."""
    rng = np.random.default_rng([0xCE14, seed])
    offs = (rng.random((want + SPARE, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(spread)
    far = BOX * np.array([0.9, 0.9, 0.05], np.float32)
    m = want - SPARE // 2
    for _ in range(8):
        cloud = _mix(p, np.concatenate([np.float32(at) + offs[:m], far + offs[m:]]), seed)
        g = grid_for(cloud)
        have = int(bucket_sizes(cloud, g)[int(cells_of(np.float32(at)[None], g)[0]) // F2])
        if have == want:
            return cloud
        m += want - have
    raise AssertionError(("no clump size gives the bucket", want, have))


@functools.lru_cache(maxsize=None)
def scene(name):
    """(references, queries, ppc, radius, what the model must show: a function of (bucket sizes of refs, of queries, ncells))"""
    kind, _, arg = name.partition(":")
    if kind == "corridor":          # 1 500 / 20 000 / 60 000 points: about 1, 13 and 40 occupied buckets
        from pointcloudcomparator_amd import synth
        n = int(arg)
        ref = _finish(synth.corridor_cloud(n, synth.SEED_A), 1)
        qry = _finish(synth.corridor_cloud(n, synth.SEED_B), 2)
        lo, hi = {1500: (1, 2), 20000: (10, 16), 60000: (30, 50)}[n]
        return ref, qry, 0.75, 0.08, lambda br, bq, nc: lo <= (br > 0).sum() <= hi
    if kind == "boundary":          # LIGHT - 1, LIGHT, LIGHT + 1 in one bucket whose neighbours in the group of four are light
        d = int(arg)
        at = np.array([0.31, 0.11, 0.52], np.float32)
        ref = _clump_in(_finish(_box(20000, 3), 3), at, lambda c: grid_of(c, 0.4), LIGHT_PTS + d, 0.004, 4)
        g = grid_of(ref, 0.4)
        qry = _clump_in(_finish(_box(20000, 5), 5), at, lambda c: g, LIGHT_ORD + d, 0.004, 6)
        b = int(cells_of(at[None], g)[0]) // F2

        def shows(br, bq, nc):
            mates_r, mates_q = np.delete(br[b - b % 4:b - b % 4 + 4], b % 4), np.delete(bq[b - b % 4:b - b % 4 + 4], b % 4)
            return br[b] == LIGHT_PTS + d and bq[b] == LIGHT_ORD + d and 0 < mates_r.min() and mates_r.max() < LIGHT_PTS and \
                0 < mates_q.min() and mates_q.max() < LIGHT_ORD
        return ref, qry, 0.4, 0.03, shows
    if kind == "gap":               # two slabs, nothing between them: whole groups of empty buckets, and groups that are partly empty;
        # at this size the grid has 54 x 2048 cells: bucket 54, third of its group, holds nothing but entry [ncells]
        two = lambda s: np.concatenate([_box(11000, s, hi=(1, 1, 0.3)), _box(11000, s + 1, lo=(0, 0, 0.7))])
        ref, qry = _finish(two(7), 8), _finish(two(9), 10)

        def shows(br, bq, nc):
            four = np.pad(br, (0, -len(br) % 4)).reshape(-1, 4)
            some = ((four > 0).any(1) & (four == 0).any(1)).sum()
            last = nc // F2                     # the bucket of entry [ncells]; its group ends mid-group
            return ((four == 0).all(1)).sum() >= 2 and some >= 1 and last % 4 != 3 and nc % F2 == 0 and br.max() <= LIGHT_PTS
        return ref, qry, 0.2, 0.03, shows
    if kind == "pile":              # duplicates: a bucket whose points are all one point, in the gap where nothing else is -- the most
        # a wave sorts, more than the two-read form stages, the most a workgroup sorts from one read (four waves' worth), one more
        m_r, m_q = {"light": (LIGHT_PTS, LIGHT_ORD), "stage": (STAGE_PTS + 1, STAGE_ORD + 1), "once": (4 * LIGHT_PTS, 4 * LIGHT_ORD),
                    "twice": (4 * LIGHT_PTS + 1, 4 * LIGHT_ORD + 1)}[arg]
        at = np.array([0.2, 0.1, 0.5], np.float32)
        two = lambda s: np.concatenate([_box(8000, s, hi=(1, 1, 0.3)), _box(8000, s + 1, lo=(0, 0, 0.7))])
        ref = _mix(_finish(two(11), 12), np.repeat(at[None], m_r, 0), 12)
        qry = _mix(_finish(two(13), 14), np.repeat(at[None], m_q, 0), 14)
        g = grid_of(ref, 0.2)
        b = int(cells_of(at[None], g)[0]) // F2
        return ref, qry, 0.2, 0.03, lambda br, bq, nc: br[b] == m_r and bq[b] == m_q
    raise KeyError(name)


def model(name):
    ref, qry, ppc, _, shows = scene(name)
    g = grid_of(ref, ppc)
    return g, bucket_sizes(ref, g), bucket_sizes(qry, g), shows


def strided(p, wide):
    """12-byte records, or 32-byte ones (x, y, z and five words no search may read)"""
    if not wide:
        return np.ascontiguousarray(p[:, :3])
    out = np.full((len(p), 8), np.nan, np.float32)
    out[:, :3] = p[:, :3]
    return out


CASES = ["corridor:1500", "corridor:20000", "corridor:60000", "boundary:-1", "boundary:0", "boundary:1", "gap:", "pile:light", "pile:stage", "pile:once", "pile:twice"]


@pytest.mark.parametrize("name", CASES)
def test_three_level_sort_last_level(gpu, name):
    from pointcloudcomparator_amd import capi
    ref, qry, ppc, radius, _ = scene(name)
    g, br, bq, shows = model(name)
    ncells = int(g[2].prod())
    assert shows(br, bq, ncells), (name, "the cloud does not show what the case is about", br, bq, ncells)
    wide = CASES.index(name) % 2 == 1
    r_in, q_in = strided(ref, wide), strided(qry, not wide)
    with capi.Index(r_in, engine=capi.ENGINE_BRUTE) as bx:
        want1 = bx.nn1(q_in)
    with capi.Index(r_in, engine=capi.ENGINE_GRID) as ix:
        ix.set_option(capi.OPT_GRID_PPC, ppc)
        ix.set_option(capi.OPT_GRID_TRIM, 0)
        ix.set_input(r_in)                               # the default two-level sort (both clouds are far below its limit)
        two = (ix.nn1(q_in), ix.knn(q_in, 8), ix.radius_count(q_in, radius))
        assert ix.stats()[3] == ncells, (name, "the model's grid is not the handle's", ix.stats()[3], ncells)
        ix.set_option(capi.OPT_SORT_MP_MIN, 1000)
        ix.set_option(capi.OPT_SORT_MP_MIN_Q, 1000)
        ix.set_input(r_in)
        i1, d1 = filled((len(qry),))
        ix.nn1(q_in, i1, d1)
        assert ix.stats()[1] == 0 and ix.stats()[3] == ncells
        three = ((i1, d1), ix.knn(q_in, 8), ix.radius_count(q_in, radius))
    assert_same_rows(*three[0], *want1, (name, "k = 1 against the exhaustive engine"))
    assert_same_rows(*three[0], *two[0], (name, "k = 1 against the two-level sort"))
    assert_same_rows(*three[1], *two[1], (name, "k = 8 against the two-level sort"))
    assert_same_counts(three[2], two[2], (name, "radius count against the two-level sort"))
    sample = np.linspace(0, len(qry) - 1, SAMPLE).astype(int)
    assert_same_rows(three[1][0][sample], three[1][1][sample], *knn_oracle(ref, qry[sample], 8), (name, "k = 8 against the oracle"))
    assert_same_counts(three[2][sample], oracle.radius_count_exhaustive(ref, qry[sample], radius), (name, "radius count against the oracle"))
