"""An independent NumPy restatement of the VFH descriptor (reference src/comparator.cpp:482-516: processVHF = NormalEstimation
r = 0.03, VFHEstimation with setNormalizeBins(true), setNormalizeDistance(false), viewpoint origin) and of matchVHF
(:471-480), written from the published algorithm and NOT from csrc/vfh_math.hpp: NumPy's arccos and arctan2 through
fpfh_ref.pair_features, whole clouds at a time.

Parameterised by dtype: the centroids, the pair features and the viewpoint angle run in that dtype; the bin of a feature is
taken in double in both runs, as the C++ expressions promote.

Run as a script it prints the table of tests/test_vfh_cpu.py (EXPERIMENTS.md, "VFH descriptor")."""
from __future__ import annotations

import numpy as np

import fpfh_ref

NB, NVP = 45, 128
BINS = 4 * NB + NVP
COUNTERS = 3 * NB + NVP
D_PI = np.float32(1.0) / (np.float32(2.0) * np.float32(np.pi))  # d_pi_, a float in PCL


def _chain(a, T):
    """the sum of the rows of a, one after the other from 0 in dtype T (np.cumsum adds in order)"""
    if not len(a):
        return np.zeros(a.shape[1], T)
    return np.cumsum(a.astype(T), axis=0, dtype=T)[-1]


def centroids(p32, nrm, T):
    """(xyz centroid, normal centroid, cp, d_vp_p) in dtype T"""
    n = len(p32)
    fin = np.isfinite(nrm).all(1)
    cp = int(fin.sum())
    with np.errstate(all="ignore"):
        c = (_chain(p32, T) / T(n)).astype(T)
        nc = (_chain(nrm[fin], T) / T(cp)).astype(T)
        d = (T(0) - c).astype(T)
        d = (d / np.sqrt((d * d).sum(dtype=T))).astype(T)
    return c, nc, cp, d


def _clamped(h, bins):
    """floor'ed bin numbers in double -> 0 .. bins - 1; anything that is not >= 0, a NaN included, is bin 0"""
    with np.errstate(all="ignore"):
        return np.where(h >= 0, np.minimum(h, bins - 1), 0).astype(np.int64)


def votes(points, nrm, T):
    """every point against the centroids in dtype T.  dict: bins (n, 4) int64 -- f1, f2, f3 and viewpoint bin, ok (n,), f (n, 4),
    gap, swapped and dist (pair features, fpfh_ref.pair_features), alpha (n,) in double, cp"""
    p32 = np.ascontiguousarray(points, dtype=np.float32)
    n = len(p32)
    nrm = np.asarray(nrm)
    c, nc, cp, d = centroids(p32, nrm, T)
    P = np.vstack([p32.astype(T), c[None, :]])
    N = np.vstack([nrm.astype(T), nc[None, :]])
    pf = fpfh_ref.pair_features(P, N, np.full(n, n), np.arange(n), T)
    f = pf["f"].astype(np.float64)
    with np.errstate(all="ignore"):
        b1 = _clamped(np.floor(NB * ((f[:, 0] + np.pi) * np.float64(D_PI))), NB)
        b2 = _clamped(np.floor(NB * ((f[:, 1] + 1.0) * 0.5)), NB)
        b3 = _clamped(np.floor(NB * ((f[:, 2] + 1.0) * 0.5)), NB)
        cosv = (nrm.astype(T) * d[None, :]).sum(1, dtype=T)
        alpha = (cosv.astype(np.float64) + 1.0) * 0.5
        bv = _clamped(np.floor(alpha * NVP), NVP)
    return {"bins": np.stack([b1, b2, b3, bv], -1), "ok": pf["ok"], "f": pf["f"], "gap": pf["gap"], "swapped": pf["swapped"], "dist": pf["dist"], "alpha": alpha,
            "cp": cp, "centroid": c, "normal_centroid": nc, "d_vp_p": d}


def counters_of(bins, ok, keep=None):
    """the 263 counters from per-point bins (f1 .. f3 count where ok), over the points of `keep` (all)"""
    keep = np.ones(len(bins), bool) if keep is None else keep
    out = np.zeros(COUNTERS, np.int64)
    sel = keep & ok
    for k in range(3):
        out[k * NB:(k + 1) * NB] = np.bincount(bins[sel, k], minlength=NB)
    out[3 * NB:] = np.bincount(bins[keep, 3], minlength=NVP)
    return out


def near_edge(v, edge):
    """points whose vote the arithmetic could move.  edge = (f1, f2, f3, gap, alpha) bounds in the units of each: a feature
    within its bound of a 45-bin boundary -- f1's range is a circle, so its two ends are one more boundary; the ends of f2, f3
    and alpha clamp and are none --, the two angles of the swap decision within edge[3] of each other, or alpha within edge[4]
    of a 128-bin boundary.  A feature that is not a number is bin 0 in any arithmetic, and a gap that is not a number never
    swaps (a comparison with NaN is false): neither flags.  A point without a pair in this run is flagged unless it lies at
    the centroid exactly."""
    f = v["f"].astype(np.float64)
    out = np.zeros(len(f), bool)
    with np.errstate(all="ignore"):
        for k, (lo, width, bins, circular) in enumerate(((-np.pi, 2 * np.pi / NB, NB, True), (-1.0, 2.0 / NB, NB, False), (-1.0, 2.0 / NB, NB, False))):
            t = (f[:, k] - lo) / width
            r = np.round(t)
            inner = np.ones(len(f), bool) if circular else (r >= 1) & (r <= bins - 1)
            out |= inner & (np.abs(t - r) * width <= edge[k]) & v["ok"]
        gap = v["gap"].astype(np.float64)
        out |= (np.abs(gap) <= edge[3]) & v["ok"]
        t = v["alpha"] * NVP
        r = np.round(t)
        out |= (r >= 1) & (r <= NVP - 1) & (np.abs(t - r) / NVP <= edge[4])
    return out | (~v["ok"] & (v["dist"] != 0))


def bin_values(counters, n, T):
    """the 308 bins from the 263 counters in dtype T (float32: the increment added count times, one addition after the other;
    float64: the product)"""
    counters = np.asarray(counters, np.int64)
    incr = np.concatenate([np.full(3 * NB, T(100) / T(n - 1), T), np.full(NVP, T(np.float64(100.0) / np.float64(n)), T)])
    if T is np.float64:
        v = counters * incr
    else:
        v = np.zeros(COUNTERS, T)
        for k in range(int(counters.max()) if counters.size else 0):
            v = np.where(counters > k, v + incr, v).astype(T)
    return np.concatenate([v[:3 * NB], np.zeros(NB, T), v[3 * NB:]])


def descriptor(points, nrm, T=np.float64):
    """the 308 bins in dtype T over given normals (n >= 2)"""
    v = votes(points, nrm, T)
    return bin_values(counters_of(v["bins"], v["ok"]), len(points), T)


def match(h1, h2):
    """matchVHF of every pair: float32 difference, float64 square, the sum one term after the other, the root"""
    a, b = np.ascontiguousarray(h1, np.float32).reshape(-1, BINS), np.ascontiguousarray(h2, np.float32).reshape(-1, BINS)
    out = np.empty((len(a), len(b)), np.float64)
    with np.errstate(all="ignore"):
        for i in range(len(a)):
            for j in range(len(b)):
                d = (a[i] - b[j]).astype(np.float32)
                out[i, j] = np.sqrt(np.cumsum(d.astype(np.float64) ** 2, dtype=np.float64)[-1])
    return out


def deviation(points, nrm):
    """max |float32 run - float64 run| of f1 (as an angle), f2, f3, the swap gap and alpha over the points both runs call a pair
    and swap alike (alpha: over all points), values that are not numbers left out"""
    r32, r64 = votes(points, nrm, np.float32), votes(points, nrm, np.float64)
    both = r32["ok"] & r64["ok"] & (r32["swapped"] == r64["swapped"])
    d = np.abs(r32["f"].astype(np.float64) - r64["f"])[both][:, :3]
    d[:, 0] = fpfh_ref.circular(r32["f"][both, 0].astype(np.float64) - r64["f"][both, 0])
    g = np.abs(r32["gap"].astype(np.float64) - r64["gap"])[both]
    a = np.abs(r32["alpha"] - r64["alpha"])
    return np.array([np.nanmax(d[:, 0]), np.nanmax(d[:, 1]), np.nanmax(d[:, 2]), np.nanmax(g), np.nanmax(a)])


def value_deviation(counters, n):
    """max over the bins of |float32 repeated sum - float64 product| for these counts and this cloud size"""
    return float(np.abs(bin_values(counters, n, np.float32).astype(np.float64) - bin_values(counters, n, np.float64)).max())


if __name__ == "__main__":
    import oracle
    import vfh_util
    table = {}
    for name in vfh_util.SMALL:
        pts = vfh_util.scene(name)
        nr = oracle.normals_radius(np.ascontiguousarray(pts), 0.03)[:, :3]
        dev = deviation(pts, nr)
        table[name] = dev
        v = votes(pts, nr, np.float64)
        share = near_edge(v, 8.0 * dev).mean()
        print(f"{name}: n {len(pts)}, cp {v['cp']}, pairs {int(v['ok'].sum())}, flagged {100 * share:.2f} % at MARGIN 8, "
              f"value deviation {value_deviation(counters_of(v['bins'], v['ok']), len(pts)):.3g}")
    print("DEV_F32_VS_F64 = {" + ", ".join(f'"{k}": ({", ".join(f"{x:.3g}" for x in v)})' for k, v in table.items()) + "}")
