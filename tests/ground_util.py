"""The morphological ground filter restated in NumPy (brute force), and the scenes its tests use.

pcl::ProgressiveMorphologicalFilter and pcl::applyMorphologicalOperator (PCL 1.7) as include/pcc_nn.h specifies them: float32
arithmetic, every operation rounded on its own; boxes with both ends inclusive and their edges computed as x - half / x + half."""
import numpy as np

f32 = np.float32

# the reference's parameters (src/segmentation.cpp:330-387) and PCL's defaults for the rest
REFERENCE = dict(max_window_size=20, slope=1.0, initial_distance=0.5, max_distance=3.0, cell_size=1.0, base=2.0, exponential=True)
# the small terrain's
TERRAIN = dict(max_window_size=2, slope=1.0, initial_distance=0.05, max_distance=0.5, cell_size=0.1, base=2.0, exponential=True)


def pmf_windows(max_window_size=20, slope=1.0, initial_distance=0.5, max_distance=3.0, cell_size=1.0, base=2.0, exponential=True):
    """(windows, thresholds) as float32 arrays: the first loop of ProgressiveMorphologicalFilter::extract"""
    slope, initial_distance, max_distance, cell, base = f32(slope), f32(initial_distance), f32(max_distance), f32(cell_size), f32(base)
    ws, hs = [], []
    it, w = 0, f32(0.0)
    while w < f32(int(max_window_size)):
        if exponential:
            w = f32(float(cell) * (2.0 * float(base) ** it + 1.0))
        else:
            w = f32(float(cell) * (2.0 * (it + 1) * float(base) + 1.0))
        if it == 0:
            h = initial_distance
        else:
            h = f32(f32(f32(slope * f32(w - ws[-1])) * cell) + initial_distance)
        if h > max_distance:
            h = max_distance
        ws.append(w)
        hs.append(h)
        it += 1
        assert it <= 64
    return np.array(ws, dtype=f32), np.array(hs, dtype=f32)


def box_matrix(xyz, window, short_form=False):
    """B[i, j]: point j lies in the box of point i.  short_form: the |d| <= half form a correct kernel must NOT take."""
    p = np.asarray(xyz, dtype=f32)
    x, y = p[:, 0], p[:, 1]
    half = f32(window) / f32(2.0)
    fin = np.isfinite(p[:, :3]).all(axis=1)
    with np.errstate(invalid="ignore"):
        if short_form:
            B = (np.abs(x[None, :] - x[:, None]) <= half) & (np.abs(y[None, :] - y[:, None]) <= half)
        else:
            lo_x, hi_x, lo_y, hi_y = x - half, x + half, y - half, y + half
            B = ((lo_x[:, None] <= x[None, :]) & (x[None, :] <= hi_x[:, None]) &
                 (lo_y[:, None] <= y[None, :]) & (y[None, :] <= hi_y[:, None]))
    B &= fin[None, :] & fin[:, None]
    return B, fin


def _pass(B, fin, vals, take_max):
    fill = f32(-np.inf) if take_max else f32(np.inf)
    M = np.where(B, vals[None, :], fill)
    out = M.max(axis=1) if take_max else M.min(axis=1)
    return np.where(fin, out, vals).astype(f32)


def morph(xyz, window, op, short_form=False):
    """op: 'erode', 'dilate', 'open', 'close' -> (n,) float32"""
    p = np.asarray(xyz, dtype=f32)
    B, fin = box_matrix(p, window, short_form)
    z = p[:, 2].copy()
    if op == "erode":
        return _pass(B, fin, z, False)
    if op == "dilate":
        return _pass(B, fin, z, True)
    if op == "open":
        return _pass(B, fin, _pass(B, fin, z, False), True)
    assert op == "close"
    return _pass(B, fin, _pass(B, fin, z, True), False)


def pmf(xyz, **params):
    """(ground indices ascending, survivors after each window)"""
    p = np.asarray(xyz, dtype=f32)
    ws, hs = pmf_windows(**params)
    ground = np.arange(len(p))
    sizes = []
    for w, h in zip(ws, hs):
        if len(ground) == 0:
            sizes.append(0)
            continue
        sub = p[ground]
        o = morph(sub, w, "open")
        with np.errstate(invalid="ignore"):
            keep = ((sub[:, 2] - o).astype(f32) < h) & np.isfinite(sub[:, :3]).all(axis=1)
        ground = ground[keep]
        sizes.append(len(ground))
    if len(ws) == 0:
        ground = ground[np.isfinite(p[:, :3]).all(axis=1)]
    return ground.astype(np.int32), np.array(sizes, dtype=np.int64)


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def terrain(n=1500, seed=0, extent=4.0, cols=3):
    """a gentle slope with four raised boxes: xy uniform in [0, extent)^2"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, extent, size=(n, 2))
    z = 0.05 * xy[:, 0] + 0.03 * np.sin(3.0 * xy[:, 1]) + rng.normal(0.0, 0.004, n)
    s = extent / 4.0
    for cx, cy, half, height in ((0.8, 0.9, 0.15, 0.12), (2.9, 1.0, 0.3, 0.3), (1.2, 2.9, 0.5, 0.6), (2.8, 2.9, 0.8, 1.0)):
        inside = (np.abs(xy[:, 0] - cx * s) <= half * s) & (np.abs(xy[:, 1] - cy * s) <= half * s)
        z = np.where(inside, z + height, z)
    out = np.zeros((n, cols), dtype=f32)
    out[:, 0:2] = xy
    out[:, 2] = z
    return out


def lattice_points(nx=12, ny=9, step=0.25, seed=1):
    """points on a lattice of side `step`: a window of 2 * step hits box edges exactly"""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(nx) * step, np.arange(ny) * step)
    p = np.zeros((nx * ny, 3), dtype=f32)
    p[:, 0], p[:, 1] = gx.ravel(), gy.ravel()
    p[:, 2] = rng.normal(0.0, 1.0, nx * ny)
    return p[rng.permutation(len(p))]


def georeferenced(n=800, seed=2):
    """UTM-like coordinates: x around 512 000, y around 4 400 000 (float32 spacing 1/32 and 1/2)"""
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 3), dtype=f32)
    p[:, 0] = 512000.0 + rng.uniform(0.0, 30.0, n)
    p[:, 1] = 4400000.0 + rng.uniform(0.0, 30.0, n)
    p[:, 2] = 100.0 + 0.02 * (p[:, 0] - f32(512000.0)) + rng.normal(0.0, 0.05, n)
    tall = rng.random(n) < 0.2
    p[:, 2] = np.where(tall, p[:, 2] + rng.uniform(1.0, 6.0, n).astype(f32), p[:, 2])
    return p


def airborne_tile(n=38000, seed=5):
    """a synthetic airborne tile, about one point per square metre, with buildings and vegetation"""
    rng = np.random.default_rng(seed)
    side = float(np.sqrt(n))
    p = np.zeros((n, 3), dtype=f32)
    xy = rng.uniform(0.0, side, size=(n, 2))
    z = 0.02 * xy[:, 0] + 1.5 * np.sin(xy[:, 1] / 40.0) + rng.normal(0.0, 0.05, n)
    for _ in range(max(4, n // 2500)):
        cx, cy = rng.uniform(0.0, side, 2)
        hx, hy = rng.uniform(4.0, 15.0, 2)
        inside = (np.abs(xy[:, 0] - cx) <= hx) & (np.abs(xy[:, 1] - cy) <= hy)
        z = np.where(inside, z + rng.uniform(3.0, 12.0), z)
    veg = rng.random(n) < 0.1
    z = np.where(veg, z + rng.uniform(0.5, 8.0, n), z)
    p[:, 0:2], p[:, 2] = xy, z
    return p
