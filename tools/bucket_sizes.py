#!/usr/bin/env python3
"""The grid an index derives for a cloud (grid_params_device.hpp, untrimmed box) and what every last-level bucket of the
three-level cell sort (cellsort_mp.hip: F2 = 2048 consecutive cells) then holds -- numpy only: no GPU, no library.
usage: bucket_sizes.py [n = 10000000] [ppc = 0.75]     (synth.corridor_cloud(n, SEED_A), the C3 reference cloud)"""
import importlib.util, pathlib, sys
import numpy as np

F2 = 2048


def grid_of(pts, ppc=0.75):
    """(h, dims along the grid's axes, axis -> coordinate, origin) for the finite rows of pts (n, >= 3) float32"""
    p = np.asarray(pts, np.float32)[:, :3]
    p = p[np.isfinite(p).all(1)]
    lo, hi = p.min(0), p.max(0)
    ext = hi - lo
    keep = (ext > np.float32(1e-6) * ext.max()) & (ext > 0)
    cap = min(2.0 * len(pts) / ppc + 4096.0, 2.0 ** 31)  # (the library's own limit on the cell count lies far above these clouds)
    want = min(max(1.0, len(p) / ppc), float(int(cap)))
    h = (np.prod(ext[keep].astype(np.float64)) / want) ** (1.0 / keep.sum()) if keep.any() else 1.0
    order = np.argsort(ext, kind="stable")              # shortest, second, longest (ties in x, y, z order)
    ax = np.array([order[1], order[0], order[2]])       # rows run along the second shortest extent
    while True:
        hf = np.float32(h)
        inv = np.float32(1.0) / hf
        dims = np.minimum(np.floor(ext[ax].astype(np.float64) * np.float64(inv)) + 1.0, 1048576.0).astype(np.int64)
        if dims.prod() <= int(cap):
            return hf, inv, dims, ax, lo[ax]
        h *= 1.26


def cells_of(pts, grid):
    """linear cell of every finite row of pts in that grid (grid_device.hpp cell_id: float32, clamped)"""
    _, inv, dims, ax, org = grid
    p = np.asarray(pts, np.float32)[:, :3]
    p = p[np.isfinite(p).all(1)]
    t = np.minimum(np.maximum((p[:, ax] - org) * inv, np.float32(0)), (dims - 1).astype(np.float32)).astype(np.int64)
    return (t[:, 2] * dims[1] + t[:, 1]) * dims[0] + t[:, 0]


def bucket_sizes(pts, grid):
    """points in every last-level bucket that the grid has (the last one holds cell_start[ncells])"""
    return np.bincount(cells_of(pts, grid) // F2, minlength=int(grid[2].prod()) // F2 + 1)


if __name__ == "__main__":
    spec = importlib.util.spec_from_file_location("synth", pathlib.Path(__file__).resolve().parent.parent / "pointcloudcomparator_amd" / "synth.py")
    synth = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(synth)
    n, ppc = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000, float(sys.argv[2]) if len(sys.argv) > 2 else 0.75
    pts = np.concatenate([synth.corridor_cloud(min(4_000_000, n - o), synth.SEED_A, start=o) for o in range(0, n, 4_000_000)])
    g = grid_of(pts, ppc)
    every = bucket_sizes(pts, g)
    b = every[every > 0]
    print(f"n {n}  ppc {ppc}  h {g[0]:.5f}  dims {' x '.join(map(str, g[2]))} = {g[2].prod()} cells  non-empty buckets {len(b)}")
    print(f"points per bucket: median {int(np.median(b))}  p90 {int(np.percentile(b, 90))}  max {b.max()}")
    for cut in (768, 1024, 1536, 2048, 3072):
        four = np.pad(every, (0, -len(every) % 4)).reshape(-1, 4)
        light = four[(four <= cut).all(1)]
        print(f"  <= {cut}: {(b <= cut).sum()} buckets ({(b <= cut).mean() * 100:.0f} %) with {b[b <= cut].sum() / n * 100:.0f} % of the points; "
              f"groups of four all that light: {len(light)} of {len(four)} with {light.sum() / n * 100:.0f} % of the points")
