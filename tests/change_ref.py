"""The contract of pcc_change_detection (include/pcc_nn.h) restated in NumPy float64: np.floor on the same double expressions,
membership with Python sets.  Imports nothing of the library.

    anchor(a, b, res)              the lattice's minimum corner a[3] (None: neither cloud has a finite point)
    voxels(points, anchor, res)    (finite mask, int64 voxel coordinates of the finite rows)
    change_detection(a, b, res, min_points_per_leaf=0)   the ascending int32 indices into b
"""
import numpy as np

EPS = float(np.finfo(np.float32).eps)  # FLT_EPSILON


def finite_rows(points):
    return np.isfinite(np.asarray(points)[:, :3]).all(axis=1)


def anchor(a, b, res):
    """p = the first finite point of a in index order, else of b; per axis, in double and in this order:
    mn = p - res/2, mx = p + res/2, side = 2*res - eps, over = (side - (mx - mn)) / 2, anchor = mn - over"""
    res = np.float64(res)
    for cloud in (a, b):
        ok = np.flatnonzero(finite_rows(cloud))
        if len(ok):
            p = np.asarray(cloud)[ok[0], :3].astype(np.float64)
            mn = p - res / 2
            mx = p + res / 2
            side = 2 * res - np.float64(EPS)
            over = (side - (mx - mn)) / 2
            return mn - over
    return None


def voxels(points, anc, res):
    ok = finite_rows(points)
    q = (np.asarray(points)[ok, :3].astype(np.float64) - anc) / np.float64(res)
    return ok, np.floor(q).astype(np.int64)


def change_detection(a, b, res, min_points_per_leaf=0):
    anc = anchor(a, b, res)
    if anc is None:
        return np.zeros(0, np.int32)
    _, ka = voxels(a, anc, res)
    ok_b, kb = voxels(b, anc, res)
    in_a = set(map(tuple, ka.tolist()))
    keys_b = list(map(tuple, kb.tolist()))
    count_b = {}
    for k in keys_b:
        count_b[k] = count_b.get(k, 0) + 1
    rows = np.flatnonzero(ok_b)
    out = [int(i) for i, k in zip(rows, keys_b) if k not in in_a and count_b[k] >= min_points_per_leaf]
    return np.asarray(out, np.int32)
