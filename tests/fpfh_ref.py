"""An independent NumPy restatement of the FPFH descriptor pipeline (reference src/comparator.cpp:824-875: processFPFH =
NormalEstimation r = 0.03, removeNaNNormals, FPFHEstimation r = 0.05 with 11 + 11 + 11 bins), written from the published
algorithm and NOT from csrc/fpfh_math.hpp: LAPACK for the normal, NumPy's arccos and arctan2, whole rows at a time.

Parameterised by dtype.  Row MEMBERSHIP and order come from the float32 squared distances in both cases (rift_ref._rows), so
float32 and float64 runs differ in arithmetic only, never in which points they look at.  The bin of a feature is taken in
double in both runs, as the C++ expressions promote.

Run as a script it prints the tables of tests/test_fpfh_cpu.py (EXPERIMENTS.md, "FPFH descriptors")."""
from __future__ import annotations

import numpy as np

from rift_ref import _rows

NB = 11
D_PI = np.float32(1.0) / (np.float32(2.0) * np.float32(np.pi))  # d_pi_, a float in PCL


def normals(p32, rows_n, T):
    """pcc_normals_radius semantics in dtype T: the smallest eigenvector of the row's single-pass covariance, turned to the origin"""
    p = np.where(np.isfinite(p32).all(1)[:, None], p32, 0).astype(T)
    out = np.full((len(p32), 3), np.nan, T)
    for i, j in enumerate(rows_n):
        if len(j) < 3:
            continue
        q = p[j]
        inv = T(1) / T(len(j))
        m = q.sum(0, dtype=T) * inv
        cov = ((q.T @ q).astype(T) * inv - np.outer(m, m)).astype(T)
        nv = np.linalg.eigh(cov)[1][:, 0].astype(T)
        out[i] = -nv if nv @ (-p[i]) < 0 else nv
    return out


def pair_features(p, nrm, a, b, T):
    """pcl::computePairFeatures of the pairs (a[k], b[k]) in dtype T: dict of f (m, 4), ok, swapped, gap = acos|a1| - acos|a2|"""
    pa, pb, na, nb = p[a].astype(T), p[b].astype(T), nrm[a].astype(T), nrm[b].astype(T)
    with np.errstate(all="ignore"):
        dp = pb - pa
        f4 = np.sqrt((dp * dp).sum(1, dtype=T))
        a1 = (na * dp).sum(1, dtype=T) / f4
        a2 = (nb * dp).sum(1, dtype=T) / f4
        gap = np.arccos(np.abs(a1)) - np.arccos(np.abs(a2))
        swapped = gap > 0
        n1 = np.where(swapped[:, None], nb, na)
        n2 = np.where(swapped[:, None], na, nb)
        dp = np.where(swapped[:, None], -dp, dp)
        f3 = np.where(swapped, -a2, a1)
        v = np.cross(dp, n1).astype(T)
        vn = np.sqrt((v * v).sum(1, dtype=T))
        ok = (f4 != 0) & (vn != 0)
        v = v / vn[:, None]
        w = np.cross(n1, v).astype(T)
        f2 = (v * n2).sum(1, dtype=T)
        f1 = np.arctan2((w * n2).sum(1, dtype=T), (n1 * n2).sum(1, dtype=T))
    f = np.stack([f1, f2, f3, f4], -1).astype(T)
    f[~ok] = 0
    return {"f": f, "ok": ok, "swapped": swapped & ok, "gap": gap.astype(T), "dist": f4}


def bins_of(f):
    """the three bins of every pair (m, 3), in double"""
    f = f.astype(np.float64)
    h1 = np.floor(NB * ((f[:, 0] + np.pi) * np.float64(D_PI)))
    h2 = np.floor(NB * ((f[:, 1] + 1.0) * 0.5))
    h3 = np.floor(NB * ((f[:, 2] + 1.0) * 0.5))
    return np.clip(np.stack([h1, h2, h3], -1), 0, NB - 1).astype(np.int64)


def near_edge(pf, edge):
    """pairs whose vote the arithmetic could move: a feature within edge[k] (feature units) of a bin boundary -- f1's range is a
    circle, so its two ends are one more boundary; the ends of f2 and f3 clamp and are none -- or the two angles of the
    swap decision within edge[3] of each other (a gap that is not a number counts as that)"""
    f = pf["f"].astype(np.float64)
    out = np.zeros(len(f), bool)
    for k, (lo, width, circular) in enumerate(((-np.pi, 2 * np.pi / NB, True), (-1.0, 2.0 / NB, False), (-1.0, 2.0 / NB, False))):
        t = (f[:, k] - lo) / width
        r = np.round(t)
        inner = np.ones(len(f), bool) if circular else (r >= 1) & (r <= NB - 1)
        out |= inner & (np.abs(t - r) * width <= edge[k])
    gap = pf["gap"].astype(np.float64)
    out |= ~(np.abs(gap) > edge[3])
    return (out | ~pf["ok"]) & (pf["dist"] != 0)  # (coincident points are no pair in any arithmetic)


def spfh_table(counts, row_len, T):
    """hist_incr = 100 / (row_len - 1) added count times (float32: one addition after the other; float64: the product)"""
    with np.errstate(all="ignore"):
        incr = (T(100) / (row_len.astype(T) - T(1))).astype(T)
    if T is np.float64:
        with np.errstate(all="ignore"):
            return np.where(counts > 0, counts * incr[:, None], 0.0)
    s = np.zeros(counts.shape, T)
    for k in range(int(counts.max()) if counts.size else 0):
        s = np.where(counts > k, s + incr[:, None], s).astype(T)
    return s


def weighting(spfh, rows_f, d2, in2, T):
    """weightPointSPFHSignature in dtype T over a given SPFH table (n, 33): every bin in row order, every feature's running sum
    entry-major, bin-minor; then float(100.0 / sum) per feature.  Returns (n, 33), rows outside cloud2 zero."""
    n = len(spfh)
    out = np.zeros((n, 3 * NB), T)
    table = spfh.astype(T)
    for i in np.nonzero(in2)[0]:
        j = rows_f[i]
        j = j[in2[j] & (d2[i, j] != 0)]
        if not len(j):
            continue
        with np.errstate(all="ignore"):
            vals = (table[j] * (T(1) / d2[i, j].astype(T))[:, None]).astype(T)
        h = np.cumsum(vals, axis=0, dtype=T)[-1]
        for f in range(3):
            s = np.cumsum(vals[:, f * NB:(f + 1) * NB].reshape(-1), dtype=T)[-1]
            fac = T(100.0 / np.float64(s)) if s != 0 else T(0)
            out[i, f * NB:(f + 1) * NB] = h[f * NB:(f + 1) * NB] * fac
    return out


def fpfh_pipeline(points, dtype=np.float64, normal_radius=0.03, fpfh_radius=0.05, normals_given=None, edge=None):
    """points (n, 3) float32.  Returns a dict: hist (m, 33) dtype, index (m,) int32, counts (n, 33) int64, row_len (n,) the
    cloud2 entries of every r = fpfh_radius row, in2, rows / d2 of that radius, spfh (n, 33) and -- with edge = four bounds --
    flagged (n,): points with a pair near_edge() names in their own row."""
    T = dtype
    p32 = np.ascontiguousarray(points, dtype=np.float32)
    n = len(p32)
    ok = np.isfinite(p32).all(1)
    p = np.where(ok[:, None], p32, 0)
    nrm = np.asarray(normals_given, dtype=T) if normals_given is not None else normals(p32, _rows(p32, ok, normal_radius)[0], T)
    in2 = ok & np.isfinite(nrm).all(1)
    rows_f, d2 = _rows(p32, ok, fpfh_radius)
    counts = np.zeros((n, 3 * NB), np.int64)
    row_len = np.zeros(n, np.int64)
    flagged = np.zeros(n, bool)
    for i in np.nonzero(in2)[0]:
        j = rows_f[i]
        j = j[in2[j]]
        row_len[i] = len(j)
        j = j[j != i]
        if not len(j):
            continue
        pf = pair_features(p, nrm, np.full(len(j), i), j, T)
        b = bins_of(pf["f"])[pf["ok"]]
        for k in range(3):
            counts[i, k * NB:(k + 1) * NB] = np.bincount(b[:, k], minlength=NB)
        if edge is not None:
            flagged[i] = near_edge(pf, edge).any()
    spfh = spfh_table(counts, row_len, T)
    hist = weighting(spfh, rows_f, d2, in2, T)
    index = np.nonzero(in2)[0].astype(np.int32)
    return {"hist": hist[index], "index": index, "counts": counts, "row_len": row_len, "in2": in2, "rows": rows_f, "d2": d2,
            "spfh": spfh, "flagged": flagged, "normals": nrm}


def circular(d):
    """|difference| of two angles"""
    d = np.abs(d) % (2 * np.pi)
    return np.minimum(d, 2 * np.pi - d)


def pair_deviation(p, nrm, a, b):
    """max |float32 run - float64 run| of f1 .. f4 and of the swap gap over the pairs both runs call a pair and swap alike"""
    r32, r64 = pair_features(p, nrm, a, b, np.float32), pair_features(p, nrm, a, b, np.float64)
    both = r32["ok"] & r64["ok"] & (r32["swapped"] == r64["swapped"])
    d = np.abs(r32["f"].astype(np.float64) - r64["f"])[both]
    d[:, 0] = circular(r32["f"][both, 0].astype(np.float64) - r64["f"][both, 0])
    g = np.abs(r32["gap"].astype(np.float64) - r64["gap"])[both]
    return np.append(d.max(0), g[np.isfinite(g)].max())


def scene_tables(pts, nrm, a, b, margin=8.0):
    """what tests/test_fpfh_cpu.py tabulates for one scene, all of it from the restatement alone, the normals given: the pair
    deviation (f1, f2, f3, f4, swap gap), the weighting deviation (float32 against float64 over the same SPFH table), the share
    of cloud2's points left out of the count comparison with edge = margin x the pair deviation, and the float64 run"""
    dev = pair_deviation(np.where(np.isfinite(pts), pts, 0), nrm, a, b)
    edge = margin * dev[[0, 1, 2, 4]]
    r = fpfh_pipeline(pts, np.float64, normals_given=nrm, edge=edge)
    t32 = spfh_table(r["counts"], r["row_len"], np.float32)
    w32 = weighting(t32, r["rows"], r["d2"], r["in2"], np.float32)
    w64 = weighting(t32, r["rows"], r["d2"], r["in2"], np.float64)
    return dev, float(np.abs(w32 - w64).max()), float(r["flagged"][r["in2"]].mean()), r


if __name__ == "__main__":
    import oracle
    import fpfh_util
    pair, weight = {}, {}
    for name in fpfh_util.SMALL:
        pts = fpfh_util.scene(name)
        nr = oracle.normals_radius(np.ascontiguousarray(pts), 0.03)[:, :3]
        a, b = fpfh_util.scene_pairs(pts, nr)
        dev, wdev, share, r = scene_tables(pts, nr, a, b)
        pair[name], weight[name] = dev, wdev
        rl = r["row_len"][r["in2"]]
        print(f"{name}: {len(a)} pairs, left out {100 * share:.2f} %, cloud2 {int(r['in2'].sum())} / {len(pts)}, rows median {np.median(rl):.0f} "
              f"min {rl.min()} max {rl.max()}")
    print("PAIR_F32_VS_F64 = {" + ", ".join(f'"{k}": ({", ".join(f"{x:.3g}" for x in v)})' for k, v in pair.items()) + "}")
    print("WEIGHT_F32_VS_F64 = {" + ", ".join(f'"{k}": {v:.3g}' for k, v in weight.items()) + "}")
