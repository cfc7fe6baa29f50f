"""Scenes and comparison helpers of tests/test_option_parity_gpu.py (pinned without a GPU by tests/test_option_parity_cpu.py).

Every scene is built from a fixed seed and cached, the oracle's answers with it: the GPU tests compare many routes with one
reference and never change it.  Every comparison is bit for bit: indices equal, float32 values equal as uint32."""
from __future__ import annotations

import functools

import numpy as np

import oracle

# what an output array holds before a search writes it: an index no search gives (-1 is "nothing found") and a NaN with a
# payload no arithmetic produces
FILL_IDX = np.int32(-7)
FILL_D2_BITS = np.uint32(0x7FC0BEEF)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def to_numpy(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def filled(shape):
    """(indices, squared distances) of `shape`, every entry at its fill value"""
    d2 = np.empty(shape, np.float32)
    d2.view(np.uint32)[...] = FILL_D2_BITS
    return np.full(shape, FILL_IDX, np.int32), d2


def _first(mask):
    return [tuple(int(v) for v in ix) for ix in np.argwhere(mask)[:5]]


def assert_same_rows(got_idx, got_d2, want_idx, want_d2, what=""):
    """indices and squared distances of a k = 1 or k-NN search against the expected ones: no entry left at its fill value (the
    library delivered every entry to the caller -- NOT that a kernel wrote it: see decoy_of), every index equal, every
    distance equal as uint32"""
    got_idx, got_d2 = to_numpy(got_idx), to_numpy(got_d2)
    assert got_idx.shape == want_idx.shape and got_d2.shape == want_d2.shape, (what, got_idx.shape, want_idx.shape)
    unwritten = (got_idx == FILL_IDX) | (bits(got_d2).reshape(got_d2.shape) == FILL_D2_BITS)
    assert not unwritten.any(), (what, "entries never written", _first(unwritten))
    bad = bits(got_d2).reshape(got_d2.shape) != bits(want_d2).reshape(want_d2.shape)
    assert not bad.any(), (what, "d2 bits differ", _first(bad))
    bad = got_idx != want_idx
    assert not bad.any(), (what, "indices differ", _first(bad))


def assert_same_counts(got, want, what=""):
    got = to_numpy(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), (what, "counts differ", _first(bad))


# A search writes its keys into buffers of the HANDLE (out_packed, the k-NN staging rows), which no call clears, and the caller's
# arrays are then filled from all of them: a query that a kernel skips keeps what the previous call on the handle left there.
# With the same queries in the previous call that is the right answer.  So every search under test follows a DECOY search of
# the same shape over other queries -- the same ones reversed and moved by a centimetre -- whose answer differs in every row.
DECOY_SHIFT = np.array([0.0137, -0.0071, 0.0053], np.float32)


def decoy_of(q):
    return _frozen(np.ascontiguousarray(q[::-1] + DECOY_SHIFT))


def rows_in_common(idx_a, d2_a, idx_b, d2_b):
    """rows (of found neighbours) that two answers share entry for entry: what a stale row could hide behind"""
    n = len(idx_a)
    same = (idx_a.reshape(n, -1) == idx_b.reshape(n, -1)).all(1) & (bits(d2_a).reshape(n, -1) == bits(d2_b).reshape(n, -1)).all(1)
    return int((same & (idx_a.reshape(n, -1)[:, 0] >= 0)).sum())


def knn_oracle(ref, q, k):
    """oracle.knn_exhaustive, the queries dealt out to a few threads (one C call per slice, every row the same call's answer)"""
    if len(ref) * len(q) < 4_000_000:
        return oracle.knn_exhaustive(ref, q, k)
    from concurrent.futures import ThreadPoolExecutor
    cuts = np.linspace(0, len(q), 17).astype(int)
    with ThreadPoolExecutor(max_workers=8) as pool:
        parts = list(pool.map(lambda se: oracle.knn_exhaustive(ref, q[se[0]:se[1]], k), zip(cuts[:-1], cuts[1:])))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---- A: build routes ---------------------------------------------------------------------------------------------------
BUILD_EXTENT = np.array([1.0, 0.3, 0.01], np.float32)
BUILD_STRAYS = np.array([[1000.0, 0.1, 0.005], [-1000.0, 300.0, 0.0], [0.5, 0.15, -10.0]], np.float32)  # 10^3 x the extent
BUILD_STRAY_MIN_N = 63          # smaller clouds are all box (three strays of a 3-point cloud would be the cloud)
BUILD_NONFINITE_EVERY = 97      # rows 13, 110, 207, ...: about 1 %
BUILD_RADIUS = 0.02
PACK_POINTS_PER_ROW = 512       # one pack workgroup takes 512 points (pack.hip: grid_for(n, 256, 2))


def pack_rows(n):
    """rows of per-workgroup statistics the build's pack kernel writes for n points (pack.hip launch_pack)"""
    return min(max((n + PACK_POINTS_PER_ROW - 1) // PACK_POINTS_PER_ROW, 1), 1024)


def build_stray_rows(n):
    """where the three strays sit: the last one in statistics row 130 of clouds that have one -- a row of the tail group
    (rows 128 ...) that the trimmed box skips when it is shorter than 16 rows"""
    if n < BUILD_STRAY_MIN_N:
        return []
    return [n // 7, n // 2, 130 * 256 + 5 if n > 40000 else n - 2]


def build_nonfinite_rows(n):
    return [i for i in range(13, n, BUILD_NONFINITE_EVERY) if i not in build_stray_rows(n)]


@functools.lru_cache(maxsize=None)
def build_cloud(n):
    """(n, 4) float32, 16-byte stride: an anisotropic box 1 x 0.3 x 0.01, about 1 % non-finite rows, three strays at 10^3
    times the extent, NaN in the fourth float of every other row (a search must never read it).  Row 0 is finite."""
    rng = np.random.default_rng([0xA11, n])
    a = np.zeros((n, 4), np.float32)
    a[:, :3] = rng.random((n, 3), dtype=np.float32) * BUILD_EXTENT
    a[::2, 3] = np.nan
    for j, i in enumerate(build_nonfinite_rows(n)):
        a[i, j % 3] = (np.nan, np.inf, -np.inf)[j % 3]
    for i, s in zip(build_stray_rows(n), BUILD_STRAYS):
        a[i, :3] = s
    return _frozen(a)


@functools.lru_cache(maxsize=None)
def build_queries():
    """1000 queries: a third inside the box, a third in a box twice its size about the same centre, a third far away (30 to 60
    units off, beyond every grid but not as far as the strays); rows 5, 500 and 999 are non-finite"""
    rng = np.random.default_rng(0xA12)
    inside = rng.random((334, 3)) * BUILD_EXTENT
    around = (rng.random((333, 3)) * 2.0 - 0.5) * BUILD_EXTENT
    far = rng.random((333, 3)) * BUILD_EXTENT + rng.choice([-1.0, 1.0], (333, 3)) * (30.0 + 30.0 * rng.random((333, 3)))
    q = np.concatenate([inside, around, far]).astype(np.float32)
    q = q[rng.permutation(len(q))]
    q[5, 0] = np.nan
    q[500, 2] = np.inf
    q[999, 1] = np.nan
    return _frozen(np.ascontiguousarray(q))


@functools.lru_cache(maxsize=None)
def build_expected(n):
    """the oracle over build_cloud(n) and build_queries(): (nn1 idx, nn1 d2, knn8 idx, knn8 d2, radius counts)"""
    ref, q = build_cloud(n), build_queries()
    i1, d1 = oracle.nn1_exhaustive(ref, q)
    i8, d8 = knn_oracle(ref, q, 8)
    cnt = oracle.radius_count_exhaustive(ref, q, BUILD_RADIUS)
    return _frozen(i1, d1, i8, d8, cnt)


# ---- B: k-NN runs ------------------------------------------------------------------------------------------------------
KNN_RUNS = (1, 2, 7, 16, 64)
KNN_KS = (1, 8, 51, 129, 300)
KNN_NQ = 1501                      # 19 x 79: no run length above 1 divides it
KNN_NQ_FINITE = 1481               # prime.  THIS is what the selection kernel cuts into runs (knn.hip:537, 557: the sorted order
                                   # holds the finite queries only), so it is the count no run length may divide
KNN_PILE = 320                     # copies per pile: more than the largest k, so the K-th distance of a pile member is 0
KNN_PARTS = {"lattice": 3000, "piles": 6 * KNN_PILE, "clumps": 4800, "sparse": 2300, "nonfinite": 20}


@functools.lru_cache(maxsize=None)
def knn_scene():
    """(references (12040, 3), family of every reference, queries (1501, 3), kind of every query).
    References: a 10 x 10 x 10 lattice of pitch 0.05, every site three times (exact duplicates); six piles of 320 copies of one
    point; eight clumps of 600 points within millimetres; a sparse scatter over a box 6 units wide between and around them;
    20 non-finite rows.  Shuffled.  Queries: 640 references themselves (120 of the sparse scatter; 20 copies of every pile among them:
    separation 0 after a K-th distance of 0), 480 jittered copies, 361 points outside the grid, 20 non-finite rows (these never
    enter the cell-sorted order the runs are cut from: 1481 queries do)."""
    rng = np.random.default_rng(0xB01)
    g = np.arange(10, dtype=np.float32) * np.float32(0.05)
    lattice = np.repeat(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3), 3, axis=0)
    pile_at = (rng.random((6, 3)) * 0.4 + np.array([1.0, 0.0, 0.0])).astype(np.float32)
    piles = np.repeat(pile_at, KNN_PILE, axis=0)
    centres = rng.random((8, 3)) * 1.5 + np.array([0.0, 1.0, 0.0])
    clumps = (centres[:, None, :] + rng.normal(0, 0.002, (8, 600, 3))).reshape(-1, 3).astype(np.float32)
    sparse = (rng.random((KNN_PARTS["sparse"], 3)) * 6.0 - 2.0).astype(np.float32)
    bad = rng.random((KNN_PARTS["nonfinite"], 3)).astype(np.float32)
    bad[np.arange(len(bad)), np.arange(len(bad)) % 3] = np.nan
    ref = np.concatenate([lattice, piles, clumps, sparse, bad])
    fam = np.concatenate([np.full(len(x), k) for k, x in enumerate([lattice, piles, clumps, sparse, bad])])
    assert [int((fam == k).sum()) for k in range(5)] == list(KNN_PARTS.values())
    perm = rng.permutation(len(ref))
    ref, fam = np.ascontiguousarray(ref[perm]), fam[perm]
    own = np.concatenate([np.nonzero(fam == 0)[0][:200], np.nonzero(fam == 2)[0][:200], np.nonzero(fam == 3)[0][:120]])
    pile_q = np.repeat(pile_at, 20, axis=0)                                     # 120: six runs of identical queries
    jit = ref[rng.choice(np.nonzero(fam < 4)[0], 480, replace=False)] + rng.normal(0, 0.003, (480, 3)).astype(np.float32)
    outside = (rng.random((361, 3)) * 3.0 + rng.choice([-1.0, 1.0], (361, 3)) * 20.0).astype(np.float32)
    nanq = rng.random((20, 3)).astype(np.float32)
    nanq[np.arange(20), np.arange(20) % 3] = np.tile(np.array([np.nan, np.inf, -np.inf], np.float32), 7)[:20]
    q = np.concatenate([ref[own], pile_q, jit, outside, nanq]).astype(np.float32)
    kind = np.concatenate([np.full(len(own), 0), np.full(len(pile_q), 1), np.full(480, 2), np.full(361, 3), np.full(20, 4)])
    # (shuffled: the library sorts the queries by cell, which brings the equal ones of a pile back together)
    perm = rng.permutation(len(q))
    q, kind = np.ascontiguousarray(q[perm]), kind[perm]
    assert len(q) == KNN_NQ and int(np.isfinite(q).all(1).sum()) == KNN_NQ_FINITE
    return _frozen(ref, fam, q, kind)


@functools.lru_cache(maxsize=None)
def knn_queries(decoy=False):
    q = knn_scene()[2]
    return decoy_of(q) if decoy else q


@functools.lru_cache(maxsize=None)
def knn_expected(k, decoy=False):
    return _frozen(*knn_oracle(knn_scene()[0], knn_queries(decoy), k))


@functools.lru_cache(maxsize=None)
def knn_small_scene():
    """40 references, 3 of them non-finite, and 90 queries around them: k = 51 finds fewer than K everywhere"""
    rng = np.random.default_rng(0xB02)
    ref = rng.random((40, 3), dtype=np.float32)
    ref[[7, 19, 33], [0, 1, 2]] = np.nan
    q = (rng.random((90, 3)) * 1.4 - 0.2).astype(np.float32)
    q[:30] = ref[rng.integers(0, 40, 30)]
    q[44, 1] = np.nan
    return _frozen(ref, np.ascontiguousarray(q))


@functools.lru_cache(maxsize=None)
def self_knn_scene():
    """6000 points whose self k-NN rows feed pcc_sor and pcc_normals: surfaces (bound path taken), clumps, a few duplicates"""
    rng = np.random.default_rng(0xB03)
    sheet = rng.random((3000, 3)) * np.array([1.0, 1.0, 0.002])
    blobs = (rng.random((10, 3))[:, None, :] + rng.normal(0, 0.01, (10, 250, 3))).reshape(-1, 3)
    loose = rng.random((500, 3)) * 3.0 - 1.0
    a = np.concatenate([sheet, blobs, loose]).astype(np.float32)
    a[100:130] = a[200:230]            # exact duplicates
    a[41, 0] = np.nan
    return _frozen(np.ascontiguousarray(a[rng.permutation(len(a))]))


# ---- C: placement of the k = 1 search ------------------------------------------------------------------------------------
XCD_RUNS = (1, 2, 3, 256, 4096)
NN1_FORMS = (0, 1)
DENSE_MINS = (1, 4, 1000000)
# Query counts.  grid.hip:1021 clamps the run to r = max(1, min(PCC_OPT_XCD_RUN, ceil(nq / 128) / 16)).  The flat kernel
# (PCC_OPT_NN1_KERNEL = 1) launches F = ceil(nq / 128) workgroups and remaps with run r; the lane-per-query kernel (= 0) launches
# L = ceil(nq / 256) workgroups and remaps with run (r + 1) / 2.  A run of 1 skips the remap; a run R > 1 remaps the workgroups
# below floor(W / 8R) * 8R and leaves the rest (the tail clause) where they are.
PLACEMENT_NQ = (
    2500,    # F = 20, clamp 1: every option value runs r = 1 -- the remap is skipped in both kernels
    4700,    # F = 37, clamp 2: r = 2 from option 2 on -- flat: 8R = 16, 32 remapped, a tail of 5; lane kernel: run 1, no remap
    6700,    # F = 53, clamp 3: r = 3 from option 3 on -- flat: 8R = 24, 48 remapped, tail 5 (r = 2: 16, 48 remapped, tail 5);
             #         lane kernel: L = 27, run 2, 8R = 16, 16 remapped, tail 11
    10300,   # F = 81, clamp 5: r = 5 for 256 and 4096 -- flat: 8R = 40, 80 remapped, a tail of ONE workgroup (r = 2: 80 + 1,
             #         r = 3: 72 + 9); lane kernel: L = 41, run 3 (r = 5), 8R = 24, 24 remapped, tail 17; run 2 (r = 3): 32 + 9
)


def placement_effective_run(nq, option):
    return max(1, min(option, ((nq + 127) // 128) // 16))


def placement_launch(nq, form, option):
    """(workgroups, run of the remap) of the k = 1 kernel for nq queries: grid.hip:1041 and :1076"""
    r = placement_effective_run(nq, option)
    return ((nq + 127) // 128, r) if form else ((nq + 255) // 256, (r + 1) // 2)


@functools.lru_cache(maxsize=None)
def placement_scene():
    """(references (20000, 3), queries (10300, 3)): the "pile" and "clumps" families of tests/test_nn1_kernels_gpu.py -- one cell
    holding thousands of equal points, and tight clumps on a coarse lattice -- so that waves over dense and over sparse cells both
    occur; the queries cover the box and its surroundings, some are references, a few non-finite.  A test takes a prefix."""
    rng = np.random.default_rng(0xC01)
    pile = np.full((6000, 3), 0.5, np.float32)
    pile[:100] = rng.random((100, 3), dtype=np.float32)
    clumps = (rng.integers(0, 6, (14000, 3)) * np.float32(0.2) + rng.normal(0, 0.004, (14000, 3))).astype(np.float32)
    ref = np.concatenate([pile, clumps])
    ref = np.ascontiguousarray(ref[rng.permutation(len(ref))])
    q = (rng.random((max(PLACEMENT_NQ), 3)) * 1.2 - 0.1).astype(np.float32)
    q[::11] = ref[rng.integers(0, len(ref), len(q[::11]))]
    q[::331, 1] = np.nan
    return _frozen(ref, np.ascontiguousarray(q))


@functools.lru_cache(maxsize=None)
def placement_queries(nq, decoy=False):
    q = placement_scene()[1][:nq]
    return decoy_of(q) if decoy else q


@functools.lru_cache(maxsize=None)
def placement_expected(nq, decoy=False):
    return _frozen(*oracle.nn1_exhaustive(placement_scene()[0], placement_queries(nq, decoy)))


# ---- D: ICP ---------------------------------------------------------------------------------------------------------------
ICP_SOURCE_SIZES = (2048, 2049, 4095, 4096, 6000)   # k_icp_sums takes 2048 points per workgroup; ICP_SORTED acts from 4096
ICP_ROW_CAP_POINTS = 983041                          # ceil(n / 2048) = 481 rows, capped at ICP_MAX_BLOCKS = 480


@functools.lru_cache(maxsize=None)
def icp_scene(m):
    """(target (20000, 3), source (m, 3)): the source is synth.rigid_offset of the target's first m points"""
    from pointcloudcomparator_amd import synth
    tgt = synth.corridor_cloud(20000, synth.SEED_A)
    src = np.ascontiguousarray(synth.rigid_offset(tgt[:m].copy(), jitter=0.002), dtype=np.float32)
    return _frozen(tgt, src)


# ---- E / F ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rebuild_clouds():
    """(held first (5000, 3), then built (20000, 3), queries (800, 3)) of the failed-build test; two different clouds"""
    rng = np.random.default_rng(0xE01)
    first = rng.random((5000, 3), dtype=np.float32)
    second = (rng.random((20000, 3)) * np.array([2.0, 1.0, 0.5]) + 3.0).astype(np.float32)
    second[::501, 2] = np.nan
    q = np.concatenate([second[:400] + np.float32(0.004), rng.random((400, 3), dtype=np.float32)]).astype(np.float32)
    return _frozen(first, second, np.ascontiguousarray(q))


@functools.lru_cache(maxsize=None)
def tie_scene():
    """(references (900, 3), queries (400, 3)): 300 points three times over, every query one of them -- each query's nearest
    reference exists three times at distance 0, the tie a PCC_TIES_FLANN search flags"""
    rng = np.random.default_rng(0xF01)
    base = rng.random((300, 3), dtype=np.float32)
    ref = np.ascontiguousarray(np.concatenate([base, base, base])[rng.permutation(900)])
    q = np.ascontiguousarray(base[rng.integers(0, 300, 400)])
    return _frozen(ref, q)
