"""An independent NumPy restatement of the SHOT352 descriptor pipeline (reference src/comparator.cpp:941-986: NormalEstimation
r = 0.05, removeNaNNormals, SHOTEstimation r = 0.04), written from the statement of pcc_shot_descriptors in include/pcc_nn.h
and NOT from csrc/shot_math.hpp: LAPACK's eigh for the frame, NumPy's arccos and arctan2, all entries of all rows at a time.

Parameterised by dtype.  Row MEMBERSHIP and order come from the float32 squared distances in both cases (rift_ref._rows), and
sqrtf(d2) is the float root in both, as the statement has it; everything else -- differences, dots, sums, the interpolation -- runs
in the dtype, so the float32 and the float64 run differ in arithmetic only, never in which points they look at.

Run as a script it prints the tables of tests/test_shot_cpu.py (EXPERIMENTS.md, "SHOT descriptors")."""
from __future__ import annotations

import numpy as np

from fpfh_ref import normals  # pcc_normals_radius semantics in a dtype
from rift_ref import _rows

BINS = 352
GAP = 1e-3   # adjacent eigenvalue gap relative to the trace below which a frame is not compared (EXPERIMENTS.md says why)
MIN_NEIGHBOURS = 5


def _unit_angle(a, b):
    """the angle between two axes known up to sign"""
    c = np.cross(a.astype(np.float64), b.astype(np.float64))
    return float(np.arcsin(min(1.0, np.sqrt((c * c).sum()))))


def lrf(p32, rows, d2, in2, radius, T):
    """getLocalRF in dtype T for every point of cloud2.  Returns a dict over all n points: rf (n, 9) T (NaN: no frame), valid (n,),
    gap (n,) the smaller adjacent eigenvalue gap over the trace, axes (n, 2, 3) the unsigned x and z as eigh gives them, s (n, 2)
    the vote sums 2 plus - valid of x and z, dots: per point (valid, 2) the v . x and v . z of its valid entries in row order, cov (n, 6)
    the weighted covariance (xx, xy, xz, yy, yz, zz)"""
    n = len(p32)
    out = {"rf": np.full((n, 9), np.nan, T), "valid": np.zeros(n, np.int64), "gap": np.full(n, np.nan), "axes": np.full((n, 2, 3), np.nan, T),
           "s": np.zeros((n, 2), np.int64), "dots": [None] * n, "cov": np.full((n, 6), np.nan)}
    for i in np.nonzero(in2)[0]:
        j = rows[i]
        j = j[in2[j] & (d2[i, j] != 0)]
        valid = out["valid"][i] = len(j)
        if valid < MIN_NEIGHBOURS:
            continue
        v = (p32[j] - p32[i]).astype(T)                       # the difference in float, then promoted
        w = T(radius) - np.sqrt(d2[i, j]).astype(T)           # the root in float, then promoted
        cov = ((v * w[:, None]).T @ v).astype(T) / w.sum(dtype=T)
        out["cov"][i] = cov[[0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]
        ev, vec = np.linalg.eigh(cov)
        if not np.isfinite(ev).all():
            continue
        axes = np.stack([vec[:, 2], vec[:, 0]]).astype(T)     # x: the largest eigenvalue, z: the smallest
        out["gap"][i] = min(ev[1] - ev[0], ev[2] - ev[1]) / float(ev.sum())
        out["axes"][i] = axes
        dots = (v @ axes.T).astype(T)
        out["dots"][i] = dots
        signed = axes.copy()
        for a in range(2):
            s = out["s"][i, a] = 2 * int((dots[:, a] >= 0).sum()) - valid
            if s < 0 or (s == 0 and int((dots[valid // 2 - 2:valid // 2 + 3, a] > 0).sum()) < 3):
                signed[a] = -signed[a]
        x, z = signed
        out["rf"][i] = np.concatenate([x, np.cross(z, x).astype(T), z])
    return out


def lrf_flags(f, edge, gap=GAP):
    """points whose frame the arithmetic could turn or flip: an adjacent eigenvalue gap below `gap`, or a sign decision that rests on
    entries with |v . axis| < edge -- m such entries can move the vote sum s by 2 m, so |s| <= 2 m, or one of them among the five
    median entries when s == 0"""
    n = len(f["valid"])
    out = np.zeros(n, bool)
    for i in range(n):
        dots = f["dots"][i]
        if dots is None:
            continue
        if not f["gap"][i] >= gap:
            out[i] = True
            continue
        valid = int(f["valid"][i])
        for a in range(2):
            near = np.abs(dots[:, a].astype(np.float64)) < edge
            m, s = int(near.sum()), int(f["s"][i, a])
            if (m and abs(s) <= 2 * m) or (s == 0 and near[valid // 2 - 2:valid // 2 + 3].any()):
                out[i] = True
    return out


def lrf_deviation(f32, f64, gap=GAP):
    """(the largest axis angle, the largest |dot32 - dot64|) over the points both runs give axes and whose float64 gap is >= gap;
    the float32 axes are turned to the float64 axes' side first (an eigenvector has no sign)"""
    angle = dot = 0.0
    for i in range(len(f64["valid"])):
        if f64["dots"][i] is None or f32["dots"][i] is None or not f64["gap"][i] >= gap:
            continue
        for a in range(2):
            a64, a32 = f64["axes"][i, a].astype(np.float64), f32["axes"][i, a].astype(np.float64)
            angle = max(angle, _unit_angle(a32, a64))
            side = -1.0 if a32 @ a64 < 0 else 1.0
            dot = max(dot, float(np.abs(side * f32["dots"][i][:, a].astype(np.float64) - f64["dots"][i][:, a]).max()))
    return angle, dot


def descriptors(p32, nrm, rf, rows, d2, in2, radius, T):
    """computePointSHOT in dtype T with the frames rf (n, 9) and the normals nrm (n, 3) given: (n, 352) T, NaN rows where the row
    counts fewer than 5 entries of cloud2 or the frame is not finite (and outside cloud2)"""
    n = len(p32)
    out = np.full((n, BINS), np.nan, T)
    ii, jj = [], []
    for i in np.nonzero(in2)[0]:
        j = rows[i]
        j = j[in2[j]]
        if len(j) < MIN_NEIGHBOURS or not np.isfinite(rf[i]).all():
            continue
        out[i] = 0
        ii.append(np.full(len(j), i))
        jj.append(j)
    if not ii:
        return out
    ii, jj = np.concatenate(ii), np.concatenate(jj)
    R = T(radius)
    pi = T(np.pi)
    dist = np.sqrt(d2[ii, jj]).astype(T)
    keep = np.abs(dist) >= 1e-15
    ii, jj, dist = ii[keep], jj[keep], dist[keep]
    frame = np.asarray(rf, dtype=T)[ii]
    delta = p32[jj].astype(T) - p32[ii].astype(T)
    with np.errstate(all="ignore"):
        cosine = np.clip((np.asarray(nrm, dtype=T)[jj] * frame[:, 6:9]).sum(1, dtype=T), -1, 1).astype(T)
        bd = ((1 + cosine) * 10 / 2).astype(T)
        xf, yf, zf = ((delta * frame[:, 3 * k:3 * k + 3]).sum(1, dtype=T) for k in range(3))
        xf, yf, zf = (np.where(np.abs(c) < 1e-30, T(0), c).astype(T) for c in (xf, yf, zf))
        bit4 = (yf > 0) | ((yf == 0) & (xf < 0))
        bit3 = np.where((xf > 0) | ((xf == 0) & (yf > 0)), ~bit4, bit4)
        desc = (bit4.astype(np.int64) * 8 + bit3.astype(np.int64) * 4) * 2
        desc += np.where((xf * yf > 0) | (xf == 0), np.where(np.abs(xf) >= np.abs(yf), 0, 4), np.where(np.abs(xf) > np.abs(yf), 4, 0))
        desc += (zf > 0).astype(np.int64)
        desc += 2 * (dist > R / 2).astype(np.int64)
        step = np.floor(bd + T(0.5)).astype(np.int64)
        bd = (bd - step).astype(T)
        weight = (1 - np.abs(bd)).astype(T)
        votes = [(np.ones(len(ii), bool), desc * 11 + np.where(bd > 0, (step + 1) % 10, (step + 9) % 10), np.abs(bd))]
        # the husks
        outer = dist > R / 2
        rd = np.where(outer, (dist - R * 3 / 4) / (R / 2), (dist - R / 4) / (R / 2)).astype(T)
        alone = np.where(outer, dist > R * 3 / 4, dist < R / 4)
        weight += np.where(alone == outer, 1 - rd, 1 + rd).astype(T)   # (1 - rd: outermost, or inner voting outwards)
        votes.append((~alone, (desc + np.where(outer, -2, 2)) * 11 + step, np.abs(rd)))
        # the inclination
        inc = np.arccos(np.clip(zf / dist, -1, 1)).astype(T)
        upper = (inc > pi / 2) | ((np.abs(inc - pi / 2) < 1e-30) & (zf <= 0))
        idist = np.where(upper, (inc - pi * 3 / 4) / (pi / 2), (inc - pi / 4) / (pi / 2)).astype(T)
        alone = np.where(upper, inc > pi * 3 / 4, inc < pi / 4)
        weight += np.where(alone == upper, 1 - idist, 1 + idist).astype(T)
        votes.append((~alone, (desc + np.where(upper, 1, -1)) * 11 + step, np.abs(idist)))
        # the azimuth
        has = (xf != 0) | (yf != 0)
        az = np.arctan2(yf, xf).astype(T)
        ad = np.clip((az - (-pi * 7 / 8 + (pi / 4) * (desc >> 2).astype(T))) / (pi / 4), -0.5, 0.5).astype(T)
        weight += np.where(has, np.where(ad > 0, 1 - ad, 1 + ad), 0).astype(T)
        votes.append((has, ((desc + np.where(ad > 0, 4, 28)) % 32) * 11 + step, np.abs(ad)))
        votes.append((np.ones(len(ii), bool), desc * 11 + step, weight))
        for mask, b, val in votes:
            mask = mask & (b >= 0) & (b < BINS)
            np.add.at(out, (ii[mask], b[mask]), val[mask].astype(T))
        done = np.unique(ii)
        norm = np.sqrt((out[done].astype(np.float64) ** 2).sum(1))
        out[done] = (out[done] / norm.astype(T)[:, None]).astype(T)
    return out


def shot_pipeline(points, dtype=np.float64, normal_radius=0.05, shot_radius=0.04, normals_given=None, rf_given=None):
    """points (n, 3) float32.  Returns a dict: desc (m, 352) and rf (m, 9) in dtype, index (m,) int32, in2, row_len (n,) the cloud2
    entries of every row at shot_radius, lrf: what lrf() returns, rows / d2 of that radius, normals"""
    T = dtype
    p32 = np.ascontiguousarray(points, dtype=np.float32)
    ok = np.isfinite(p32).all(1)
    nrm = np.asarray(normals_given, dtype=T) if normals_given is not None else normals(p32, _rows(p32, ok, normal_radius)[0], T)
    in2 = ok & np.isfinite(nrm).all(1)
    p0 = np.where(ok[:, None], p32, 0)
    rows, d2 = _rows(p32, ok, shot_radius)
    f = lrf(p0, rows, d2, in2, shot_radius, T)
    rf = np.asarray(rf_given, dtype=T) if rf_given is not None else f["rf"]
    desc = descriptors(p0, nrm, rf, rows, d2, in2, shot_radius, T)
    index = np.nonzero(in2)[0].astype(np.int32)
    row_len = np.array([int(in2[r].sum()) if in2[i] else 0 for i, r in enumerate(rows)])
    return {"desc": desc[index], "rf": rf[index], "index": index, "in2": in2, "row_len": row_len, "lrf": f, "rows": rows, "d2": d2,
            "normals": nrm, "desc_all": desc, "rf_all": rf}


def scene_tables(pts, nrm, margin=8.0):
    """what tests/test_shot_cpu.py tabulates for one scene, all of it from the restatement alone, the normals given (float32):
    LRF_F32_VS_F64 (the largest axis angle), the dot deviation behind EDGE, DESC_F32_VS_F64 (the largest bin deviation with the
    float64 run's frames, rounded to float32, given to both runs), the share of cloud2 flagged, and the float64 run"""
    r64 = shot_pipeline(pts, np.float64, normals_given=nrm)
    r32 = shot_pipeline(pts, np.float32, normals_given=nrm)
    angle, dot = lrf_deviation(r32["lrf"], r64["lrf"])
    rf = r64["rf_all"].astype(np.float32)
    d64 = shot_pipeline(pts, np.float64, normals_given=nrm, rf_given=rf)["desc_all"]
    d32 = shot_pipeline(pts, np.float32, normals_given=nrm, rf_given=rf)["desc_all"]
    assert np.array_equal(np.isnan(d64), np.isnan(d32))
    fin = np.isfinite(d64)
    desc = float(np.abs(d32.astype(np.float64) - d64)[fin].max()) if fin.any() else 0.0
    flagged = lrf_flags(r64["lrf"], margin * dot)
    have = np.array([d is not None for d in r64["lrf"]["dots"]])
    return angle, dot, desc, float(flagged[have].mean()) if have.any() else 0.0, r64


if __name__ == "__main__":
    import oracle
    import shot_util
    angle, dot, desc = {}, {}, {}
    for name in shot_util.SMALL:
        pts = shot_util.scene(name)
        nr = oracle.normals_radius(np.ascontiguousarray(pts), 0.05)[:, :3]
        angle[name], dot[name], desc[name], share, r = scene_tables(pts, nr)
        rl = r["row_len"][r["in2"]]
        med = int(sum(1 for i in np.nonzero(r["in2"])[0] if r["lrf"]["dots"][i] is not None and (r["lrf"]["s"][i] == 0).any()))
        print(f"{name}: flagged {100 * share:.2f} %, cloud2 {int(r['in2'].sum())} / {len(pts)}, rows median {np.median(rl):.0f} min {rl.min()} "
              f"max {rl.max()}, median clause {med} points, NaN rows {int(np.isnan(r['desc']).all(1).sum())}")
    for label, t in (("LRF_F32_VS_F64", angle), ("LRF_DOT_F32_VS_F64", dot), ("DESC_F32_VS_F64", desc)):
        print(label + " = {" + ", ".join(f'"{k}": {v:.3g}' for k, v in t.items()) + "}")
