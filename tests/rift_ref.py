"""An independent NumPy restatement of the RIFT descriptor pipeline (reference src/comparator.cpp:590-684: processRIFT =
PointCloudXYZRGBtoXYZI, NormalEstimation r = 0.03, removeNaNNormals, IntensityGradientEstimation r = 0.03, RIFTEstimation
r = 0.05 with 4 x 8 bins, removal of non-finite descriptors), written from the published algorithms and NOT from
csrc/rift_math.hpp: LAPACK for the normal (eigh of the single-pass covariance) and for the 3 x 3 solve (lstsq, SVD), NumPy's arccos.

Parameterised by dtype.  Row MEMBERSHIP and order come from the float32 squared distances in both cases, so float32 and
float64 runs differ in arithmetic only, never in which points they look at."""
from __future__ import annotations

import numpy as np


def _rows(p32: np.ndarray, ok: np.ndarray, radius: float):
    """sorted radius rows of every point against every finite point: d2 < float32(r * r), ascending (d2, index)"""
    with np.errstate(invalid="ignore"):
        d = p32[:, None, :] - p32[None, :, :]
        d2 = d[..., 0] * d[..., 0]
        d2 = d2 + d[..., 1] * d[..., 1]
        d2 = d2 + d[..., 2] * d[..., 2]
    r2 = np.float32(radius * radius)
    out = []
    with np.errstate(invalid="ignore"):
        inside = (d2 < r2) & ok[None, :] & ok[:, None]
    for i in range(len(p32)):
        j = np.nonzero(inside[i])[0]
        out.append(j[np.lexsort((j, d2[i][j]))])
    return out, d2


def rift_pipeline(points, rgb, dtype=np.float64, normal_radius=0.03, gradient_radius=0.03, rift_radius=0.05, normals=None):
    """points (n, 3) float32, rgb (n, 3) uint8 (r, g, b).  Returns (hist (n_out, 32) dtype, index (n_out,) int32, info) with
    info = {'rows_normal': entries of every r = normal_radius row, 'cond': condition number of every gradient system}."""
    T = dtype
    p32 = np.ascontiguousarray(points, dtype=np.float32)
    n = len(p32)
    ok = np.isfinite(p32).all(1)
    p = np.where(ok[:, None], p32, 0).astype(T)
    c = rgb.astype(T)
    inten = (T(0.299) * c[:, 0] + T(0.587) * c[:, 1]) + T(0.114) * c[:, 2]
    rows_n, _ = _rows(p32, ok, normal_radius)
    # normals (pcc_normals_radius semantics: PCL's single-pass covariance E[xx] - E[x]E[x] of the row, in the run's dtype; its
    # smallest eigenvector, turned towards the origin).  `normals` replaces the stage by given (n, 3) normals.
    nrm = np.full((n, 3), np.nan, T)
    for i in range(n):
        if normals is not None:
            nrm[i] = np.asarray(normals[i], dtype=T)
            continue
        j = rows_n[i]
        if len(j) < 3:
            continue
        q = p[j]
        inv = T(1) / T(len(j))
        m = q.sum(0, dtype=T) * inv
        cov = ((q.T @ q).astype(T) * inv - np.outer(m, m)).astype(T)
        w, v = np.linalg.eigh(cov)
        nv = v[:, 0].astype(T)
        if nv @ (-p[i]) < 0:
            nv = -nv
        nrm[i] = nv
    in2 = np.isfinite(nrm).all(1)  # cloud2
    # intensity gradient over the rows of cloud2
    rows_g = rows_n if gradient_radius == normal_radius else _rows(p32, ok, gradient_radius)[0]
    grad = np.full((n, 3), np.nan, T)
    cond = np.zeros(n)
    for i in np.nonzero(in2)[0]:
        j = rows_g[i]
        j = j[in2[j]]
        if len(j) < 3:
            continue
        q = p[j] - (p[j].sum(0, dtype=T) / T(len(j)))
        di = inten[j] - inten[j].sum(dtype=T) / T(len(j))
        A = (q.T @ q).astype(T)
        b = (q.T @ di).astype(T)
        cond[i] = np.linalg.cond(A.astype(np.float64))
        x = np.linalg.lstsq(A, b, rcond=None)[0].astype(T)
        grad[i] = ((np.eye(3, dtype=T) - np.outer(nrm[i], nrm[i])) @ x).astype(T)
    # RIFT over the rows of cloud2
    rows_r, d2 = _rows(p32, ok, rift_radius)
    eps = T(np.finfo(np.float32).eps)
    hist, kept = [], []
    for i in np.nonzero(in2)[0]:
        j = rows_r[i]
        j = j[in2[j]]
        gv = grad[j]
        with np.errstate(all="ignore"):
            mag = np.sqrt((gv * gv).sum(1, dtype=T))
            e = p[j] - p[i]
            en = np.sqrt((e * e).sum(1, dtype=T))
            ang = np.arccos(((gv * (e / en[:, None])).sum(1, dtype=T) / mag).astype(T))
        ang = np.where(np.isfinite(ang), ang, T(0)).astype(T)
        d = T(4) * np.sqrt(d2[i, j].astype(T)) / (T(rift_radius) + eps)
        g = T(8) * ang / (T(np.float32(np.pi)) + eps)
        d_lo = np.maximum(np.ceil(d - 1), 0).astype(np.int64)
        d_hi = np.minimum(np.floor(d + 1), 3).astype(np.int64)
        g_lo = np.ceil(g - 1).astype(np.int64)
        g_hi = np.floor(g + 1).astype(np.int64)
        # every entry reaches at most 3 x 3 bins; flattened entry-major so that each bin adds its terms in row order
        m = len(j)
        bins = np.full((m, 9), 32, np.int64)  # 32 = nowhere
        term = np.zeros((m, 9), T)
        for a in range(3):
            for b_ in range(3):
                gi, di_ = g_lo + a, d_lo + b_
                use = (gi <= g_hi) & (di_ <= d_hi)
                with np.errstate(invalid="ignore"):
                    t = (T(1) - np.abs(d - di_.astype(T))) * (T(1) - np.abs(g - gi.astype(T))) * mag
                bins[:, a * 3 + b_] = np.where(use, ((gi + 8) % 8) * 4 + di_, 32)
                term[:, a * 3 + b_] = np.where(use, t, T(0))
        h = np.zeros(33, T)
        np.add.at(h, bins.reshape(-1), term.reshape(-1))
        h = h[:32]
        with np.errstate(all="ignore"):
            h = (h / np.sqrt((h * h).sum(dtype=T))).astype(T)
        if np.isfinite(h[0]):
            hist.append(h)
            kept.append(i)
    hist = np.array(hist, dtype=T).reshape(-1, 32)
    return hist, np.array(kept, dtype=np.int32), {"rows_normal": np.array([len(r) for r in rows_n]), "cond": cond}
