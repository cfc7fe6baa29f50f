"""pcl::VoxelGrid in plain NumPy with float64 sums: the reference pcc_voxel_grid's centroids are compared with.

The oracle (oracle.voxel_grid) adds a voxel's points in float, as PCL does, so its centroids carry a running sum's rounding
(count * 2^-24 * |coordinate|) and a kernel cannot be held to their bits.  Here x, y and z are summed in float64 and rounded to
float once -- what the kernel specifies -- and the lattice is PCL's float arithmetic, restated independently of the oracle.
On clouds whose coordinates are dyadic with few enough bits every float64 sum is exact in any order: there this reference is
the specified result to the bit."""
import numpy as np


def voxel_grid_ref(records, leaf, has_rgb):
    """records: (n, >= 3) float32 rows x, y, z[, 1, rgb word, ...] (has_rgb: >= 5 columns, the colour word's bits in column 4).
    Returns (rows, counts): rows (nv, 5 or 4) float32 in ascending voxel order -- x, y, z, 1.0 and, with has_rgb, the colour
    word's bits -- and the number of points of every voxel."""
    rec = np.asarray(records)
    assert rec.dtype == np.float32 and rec.ndim == 2 and rec.shape[1] >= (5 if has_rgb else 3)
    width = 5 if has_rgb else 4
    xyz = rec[:, :3]
    keep = np.isfinite(xyz).all(axis=1)
    p = np.ascontiguousarray(xyz[keep])
    if len(p) == 0:
        return np.zeros((0, width), np.float32), np.zeros(0, np.int64)
    inv = np.float32(1.0) / np.float32(leaf)
    fl = np.floor(p * inv)                                   # float32 product, float32 floor
    assert fl.dtype == np.float32
    min_b, max_b = np.floor(p.min(axis=0) * inv), np.floor(p.max(axis=0) * inv)
    assert np.isfinite(min_b).all() and np.isfinite(max_b).all()
    assert (np.abs(min_b) < 2.0 ** 31).all() and (np.abs(max_b) < 2.0 ** 31).all(), "a voxel coordinate beyond int32"
    min_i, max_i = min_b.astype(np.int64), max_b.astype(np.int64)
    dim = max_i - min_i + 1
    ijk = (fl - min_i.astype(np.float32)).astype(np.int64)   # int(floor(p * inv) - float(min_b)), the subtraction in float32
    assert (ijk >= 0).all() and (ijk < dim).all()
    key = ijk[:, 0] + ijk[:, 1] * dim[0] + ijk[:, 2] * dim[0] * dim[1]  # x fastest, z slowest
    order = np.argsort(key, kind="stable")
    skey = key[order]
    starts = np.flatnonzero(np.concatenate([[True], skey[1:] != skey[:-1]]))
    counts = np.diff(np.concatenate([starts, [len(skey)]])).astype(np.int64)
    sums = np.add.reduceat(p[order].astype(np.float64), starts, axis=0)
    rows = np.zeros((len(starts), width), np.float32)
    rows[:, :3] = (sums / counts[:, None].astype(np.float64)).astype(np.float32)  # rounded to float once
    rows[:, 3] = 1.0
    if has_rgb:
        word = np.ascontiguousarray(rec[keep, 4]).view(np.uint32)[order].astype(np.int64)
        fc = counts.astype(np.float32)
        packed = np.zeros(len(starts), np.int64)
        for shift in (16, 8, 0):                             # the top byte is ignored
            s = np.add.reduceat((word >> shift) & 0xFF, starts)
            packed |= (s.astype(np.float32) / fc).astype(np.int64) << shift  # int(float(sum) / float(count))
        rows[:, 4] = packed.astype(np.uint32).view(np.float32)
    return rows, counts


def ulp_distance(a, b):
    """number of float32 values between a and b, elementwise (finite inputs)"""
    def lin(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(lin(a) - lin(b))
