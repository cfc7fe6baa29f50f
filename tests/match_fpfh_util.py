"""Shared by the pcc_match_fpfh_batch tests: the 33-wide descriptor generators, the seeded batch the GPU parity test runs and the
planted-tie and bin-32 constructions.  The oracle is match_dims_util.restate / d2_chain at dim = 33 (the NumPy restatement of the
search); the CPU test asserts on the same inputs that it is sensitive to what it has to pin."""
import numpy as np

import fpfh_util
import match_dims_util as mdu

DIM = 33
FAMILIES = ("fpfh-like", "quantised")
N1, N2 = mdu.N1, mdu.N2          # around the wave share (16), the smallest slice (256) and more of them; the query block (64)
STRIDES = (132, 144, 256)        # tight (the [n][33] array pcc_fpfh_descriptors writes), the packed width, a wide record


def fpfh_cloud(n, family, seed):
    """n records of 33 floats.  "fpfh-like": three groups of eleven non-negative bins, each group scaled to sum to about 100 as
    the percentages of a pcl::FPFHSignature33 do (a few bins of a group carry most of it).  "quantised": every bin a multiple of
    1/64 in [0, 1/4], the lattice of synth.descriptor_cloud one bin wider."""
    rng = np.random.default_rng([0xF9F4, seed])
    if family == "quantised":
        return np.round(rng.random((n, DIM), dtype=np.float32) * 16) / np.float32(64)
    assert family == "fpfh-like"
    w = rng.random((n, 3, 11), dtype=np.float32) ** np.float32(4)
    w = w / w.sum(-1, keepdims=True, dtype=np.float32) * np.float32(100)
    return np.ascontiguousarray(w.reshape(n, DIM), dtype=np.float32)


def fpfh_queries(des1, n, family, seed):
    """n query records made from des1: randomly chosen records of it plus small noise -- "fpfh-like": up to +-0.5 a bin, kept
    non-negative; "quantised": one step of 1/64 in 30 % of the bins (still on the lattice)."""
    rng = np.random.default_rng([0xF9F5, seed])
    if len(des1) == 0:
        return fpfh_cloud(n, family, seed + 1)
    base = des1[rng.integers(0, len(des1), n)]
    if family == "fpfh-like":
        noise = (rng.random((n, DIM), dtype=np.float32) - np.float32(0.5)) * rng.random((n, 1), dtype=np.float32)
        return np.ascontiguousarray(np.maximum(base + noise, np.float32(0)), dtype=np.float32)
    noise = (rng.random((n, DIM), dtype=np.float32) < 0.3) * np.float32(1.0 / 64)
    return np.ascontiguousarray(base + noise, dtype=np.float32)


def family_of(i, j):
    return FAMILIES[(i + j + 1) % 2]


def parity_pairs():
    """[(des1, des2)] of (n, 33) float32: every n1 x n2 of N1 x N2, the two families alternating; pairs of one (n1, family) share
    their des1 array, as the clusters of a comparison do"""
    firsts, pairs = {}, []
    for i, n1 in enumerate(N1):
        for j, n2 in enumerate(N2):
            fam = family_of(i, j)
            if (n1, fam) not in firsts:
                firsts[(n1, fam)] = fpfh_cloud(n1, fam, 4000 + i)
            a = firsts[(n1, fam)]
            pairs.append((a, fpfh_queries(a, n2, fam, 5000 + 10 * i + j)))
    return pairs


def with_stride(x, stride, memo=None):
    """the 33 bins of x as an array whose rows are `stride` bytes apart, the floats behind bin 32 of every row NaN"""
    return mdu.with_stride(x, DIM, "tight" if stride == 4 * DIM else stride, memo)


def bin32_pair():
    """(des1, des2, perm): 300 references equal in bins 0 ... 31 and distinct in bin 32 (0.01 apart); 130 queries, references
    perm[i] with noise below 0.004 in bin 32 only.  33 bins see the permutation, 32 bins see one point 430 times."""
    rng = np.random.default_rng(33)
    a = np.tile(fpfh_cloud(1, "fpfh-like", 9), (300, 1))
    a[:, 32] = (np.arange(300, dtype=np.float32) * np.float32(0.01))[rng.permutation(300)]
    perm = rng.permutation(300)[:130]
    b = a[perm].copy()
    b[:, 32] += (rng.random(130, dtype=np.float32) - np.float32(0.5)) * np.float32(0.008)
    return np.ascontiguousarray(a), np.ascontiguousarray(b), perm


def tie_pair(n=300):
    """match_dims_util.tie_pair rebuilt 33 wide, the moved bin being bin 32: des1 = n drawn records of the quantised lattice, then
    copies of records 0 .. 39 (duplicates, in another slice of 256 than their originals), then records 40 .. 79 moved by TWO
    lattice steps in bin 32; query i = record i moved by ONE step in bin 32.  Queries 0 .. 39 are (1/64)^2 from a record and its
    copy, queries 40 .. 79 (1/64)^2 from two different records, queries 80 .. 99 have one nearest record."""
    step = np.float32(1.0 / 64)
    c = fpfh_cloud(n, "quantised", 77)
    moved = c[40:80].copy()
    moved[:, 32] += 2 * step
    des1 = np.ascontiguousarray(np.concatenate([c, c[:40], moved]))
    des2 = c[:100].copy()
    des2[:, 32] += step
    return des1, np.ascontiguousarray(des2)


# ---- the end-to-end scene: cloud A and cloud A with a compact region removed ---------------------------------------------------------
SCENE = "volume300"
CUT_RADIUS = 0.05   # B = the points of A farther than this from A's corner of smallest coordinates


def scene_clouds():
    a = fpfh_util.scene(SCENE)
    corner = a.min(0)
    far = np.sqrt(((a.astype(np.float64) - corner) ** 2).sum(1)) > CUT_RADIUS
    return np.ascontiguousarray(a), np.ascontiguousarray(a[far])
