"""Scenes and the order-free restatement shared by tests/test_rgb_device_cpu.py and tests/test_rgb_device_gpu.py
(pcc_region_growing_rgb, csrc/region_rgb.hip)."""
import numpy as np


def cascade(rng):
    """6 clumps of 40 points in one colour, each a third the size of the one before and a third as far on: the 30 nearest
    neighbours of a point at a clump's edge lie in the denser clump next to it, which does not look back -- one-way edges"""
    pts = []
    for j in range(6):
        centre_x = sum(0.25 / 3 ** i for i in range(j))
        pts.append(np.array([centre_x, 0, 0]) + (rng.random((40, 3)) - 0.5) * 0.2 / 3 ** j)
    return np.concatenate(pts).astype(np.float32), np.full((240, 3), 100, np.uint8)


def fixpoint_scenes():
    """the six scenes of the order-free argument: (name, points, colours)"""
    rng = np.random.default_rng(3)
    pts = rng.random((3000, 3)).astype(np.float32)
    out = [("patches", pts, (rng.integers(0, 3, (3000, 3)) * 20).astype(np.uint8)),
           ("near", pts, (rng.integers(0, 3, (3000, 3)) * 4).astype(np.uint8)),
           ("noise", pts, rng.integers(0, 256, (3000, 3)).astype(np.uint8)),
           ("tiny", pts[:20], (rng.integers(0, 2, (20, 3)) * 50).astype(np.uint8))]
    cp, cc = cascade(rng)
    out.append(("cascade", cp, cc))
    out.append(("cascade_rev", np.ascontiguousarray(cp[::-1]), cc))
    return out


def valid_edges(rgb, ki, nn=30, point_colour=6.0):
    """(source, target) of every valid directed edge: target among the first min(nn, K) row entries of source, integer squared
    colour distance as float32 <= float32(point_colour) squared"""
    n, K = ki.shape
    P = min(nn, K)
    nb = ki[:, :P].reshape(-1)
    src = np.repeat(np.arange(n), P)
    keep = nb >= 0
    nb, src = nb[keep], src[keep]
    c = rgb.astype(np.int64)
    diff = ((c[src] - c[nb]) ** 2).sum(1)
    ok = diff.astype(np.float32) <= np.float32(point_colour) * np.float32(point_colour)
    return src[ok], nb[ok]


def order_free_segments(rgb, ki, nn=30, point_colour=6.0):
    """segment id per point = rank of the lowest index that reaches it along valid edges; also the number of Jacobi sweeps"""
    src, nb = valid_edges(rgb, ki, nn, point_colour)
    lab = np.arange(len(ki))
    sweeps = 0
    while True:
        new = lab.copy()
        np.minimum.at(new, nb, lab[src])
        sweeps += 1
        if (new == lab).all():
            break
        lab = new
    return np.searchsorted(np.unique(lab), lab).astype(np.int32), sweeps


def ordered_pair_count(seg, ki):
    """distinct ordered pairs (s, t != s) with a row entry leading from a point of s to a point of t, over all K entries"""
    n, K = ki.shape
    nb = ki.reshape(-1)
    src = np.repeat(np.arange(n), K)
    keep = nb >= 0
    s, t = seg[src[keep]].astype(np.int64), seg[nb[keep]].astype(np.int64)
    m = s != t
    return len(np.unique(s[m] * (int(seg.max()) + 1) + t[m]))
