"""Shared by the pcc_match_knn_batch_dims tests: the NumPy restatement of the search (the test oracle) and the seeded batch the
GPU parity test runs.  The CPU test asserts on the same inputs that the restatement is sensitive to what it has to pin."""
import numpy as np

from pointcloudcomparator_amd import synth

F32_MAX = np.finfo(np.float32).max

# the parity batch: every padded width (4, 8, 16, 32), its edges and the padding; the wave share (16), the smallest slice
# (256) and more than one of them, more than one query block of 64
DIMS = (1, 2, 4, 5, 8, 16, 17, 31, 32)
N1 = (1, 15, 16, 17, 255, 257, 2049)
N2 = (1, 63, 64, 65, 130)
STRIDES = ("tight", 128, 256)


def d2_chain(a, b, dim):
    """(len(b), len(a)) float32: FLANN's L2_Simple over bins 0 .. dim-1 in index order, every operation rounded on its own:
    d = d0 * d0; d = d + d1 * d1; ..."""
    assert a.dtype == np.float32 and b.dtype == np.float32
    with np.errstate(all="ignore"):
        t = b[:, None, 0] - a[None, :, 0]
        d = t * t
        for k in range(1, dim):
            t = b[:, None, k] - a[None, :, k]
            d = d + t * t
    assert d.dtype == np.float32
    return d


def d2_fma(a, b, dim):
    """the same chain contracted to multiply-adds: d = fma(t, t, d) (t * t is exact in float64; one rounding to float32)"""
    t = (b[:, None, 0] - a[None, :, 0]).astype(np.float64)
    d = (t * t).astype(np.float32)
    for k in range(1, dim):
        t = (b[:, None, k] - a[None, :, k]).astype(np.float64)
        d = (t * t + d.astype(np.float64)).astype(np.float32)
    return d


def d2_pairwise(a, b, dim):
    """the same terms summed by NumPy's own (pairwise / unrolled) float32 sum along the contiguous axis"""
    t = np.ascontiguousarray(b[:, None, :dim] - a[None, :, :dim])
    return (t * t).sum(-1, dtype=np.float32)


def restate(a, b, dim, threshold):
    """what pcc_match_knn_batch_dims returns for the pair (des1 = a, des2 = b): (row, row_d2, tied) -- the dummy 0, then per
    query in order the LOWEST index among the nearest valid references when that distance is < threshold; tied = the queries
    whose minimum is shared by several references (whatever the threshold)."""
    row, row_d2 = [0], [np.float32(0)]
    if len(a) == 0 or len(b) == 0:
        return np.array(row, np.int32), np.array(row_d2, np.float32), 0
    d = d2_chain(a, b, dim)
    valid_a, valid_b = np.isfinite(a[:, :dim]).all(1), np.isfinite(b[:, :dim]).all(1)
    d[:, ~valid_a] = np.inf
    d[~valid_b, :] = np.inf
    d[~(d < F32_MAX)] = np.inf                                  # an overflowed distance is no neighbour
    best, arg = d.min(1), d.argmin(1)                           # (argmin: the first, i.e. lowest, index)
    found = best < F32_MAX
    tied = int((((d == best[:, None]).sum(1) > 1) & found).sum())
    keep = found & (best < np.float32(threshold))
    return (np.concatenate([row, arg[keep]]).astype(np.int32), np.concatenate([row_d2, best[keep]]).astype(np.float32), tied)


def family_of(i, j):
    return synth.DESCRIPTOR_FAMILIES[(i + j + 1) % 2]


def parity_pairs():
    """[(des1, des2)] of (n, 32) float32: every n1 x n2 of N1 x N2, the two descriptor families alternating; pairs of one
    (n1, family) share their des1 array, as the clusters of a comparison do"""
    firsts, pairs = {}, []
    for i, n1 in enumerate(N1):
        for j, n2 in enumerate(N2):
            fam = family_of(i, j)
            if (n1, fam) not in firsts:
                firsts[(n1, fam)] = synth.descriptor_cloud(n1, fam, 4000 + i)
            a = firsts[(n1, fam)]
            pairs.append((a, synth.descriptor_queries(a, n2, fam, 5000 + 10 * i + j)))
    return pairs


def with_stride(x, dim, stride, memo=None):
    """the first dim bins of x as an array whose rows are `stride` bytes apart ("tight": 4 * dim), the rest of every row NaN"""
    key = (id(x), dim, stride)
    if memo is not None and key in memo:
        return memo[key]
    if stride == "tight":
        out = np.ascontiguousarray(x[:, :dim])
    else:
        wide = np.full((len(x), stride // 4), np.nan, np.float32)
        wide[:, :dim] = x[:, :dim]
        out = wide[:, :dim]
        assert len(x) < 2 or out.strides[0] == stride
    if memo is not None:
        memo[key] = out
    return out


def tie_pair(n=300):
    """(des1, des2) on the quantised lattice with exact ties at dim 32.  The family as drawn has none there (17^32 lattice
    points: no two records of a cloud agree in all 32 bins), so they are planted: des1 = n drawn records, then copies of
    records 0 .. 39 (duplicates, in another slice of 256 than their originals), then records 40 .. 79 moved by TWO lattice
    steps in bin 31; query i = record i moved by ONE step in bin 31.  Queries 0 .. 39 are (1/64)^2 from a record and its copy,
    queries 40 .. 79 (1/64)^2 from two different records, queries 80 .. 99 have one nearest record."""
    step = np.float32(1.0 / 64)
    c = synth.descriptor_cloud(n, "quantised", 77)
    moved = c[40:80].copy()
    moved[:, 31] += 2 * step
    des1 = np.ascontiguousarray(np.concatenate([c, c[:40], moved]))
    des2 = c[:100].copy()
    des2[:, 31] += step
    return des1, np.ascontiguousarray(des2)
