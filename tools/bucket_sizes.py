#!/usr/bin/env python3
"""The grid an index derives for a cloud (grid_params_device.hpp, untrimmed box; the cell cap of grid.hip grid_nc_cap), the plan
the three-level cell sort makes for it (cellsort_mp.hip mp_plan), what every last-level bucket then holds (F2 consecutive
cells) and what a level-2 slice sees of the level-1 buckets -- numpy only: no GPU, no library.  The sort's constants are read
from the sources.
usage: bucket_sizes.py [n = 10000000] [ppc = 0.75]     (synth.corridor_cloud(n, SEED_A), the C3 reference cloud)"""
import collections, importlib.util, pathlib, re, sys
import numpy as np

_CSRC = pathlib.Path(__file__).resolve().parent.parent / "pointcloudcomparator_amd" / "csrc"


def _constants(text, names):
    """the `constexpr <type> NAME = <integer or 1u << k>;` definitions of `names` in `text`"""
    out = {}
    for name in names:
        m = re.search(r"constexpr\s+(?:unsigned\s+)?int\s+" + name + r"\s*=\s*(\d+)u?\s*(?:<<\s*(\d+))?\s*;", text)
        if m is None:
            raise LookupError(name + " not found in the sources")
        out[name] = int(m.group(1)) << int(m.group(2) or 0)
    return out


CONSTANTS = {**_constants((_CSRC / "cellsort_mp.hip").read_text(),
                          ("MP_F2", "MP_B2", "MP_MAX_B1", "MP_MAX_G", "MP_WIN", "MP_SLICE2", "MP_STAGE_BYTES")),
             **_constants((_CSRC / "grid.hip").read_text(), ("GRID_MAX_CELLS",))}
MP_F2, MP_B2, MP_MAX_B1, MP_MAX_G = (CONSTANTS[k] for k in ("MP_F2", "MP_B2", "MP_MAX_B1", "MP_MAX_G"))
MP_WIN, MP_SLICE2, MP_STAGE_BYTES, GRID_MAX_CELLS = (CONSTANTS[k] for k in ("MP_WIN", "MP_SLICE2", "MP_STAGE_BYTES", "GRID_MAX_CELLS"))
F2 = MP_F2                       # cells of a last-level bucket under every plan but the widest (sort_plan)
# elements of a level-2 slice: the placing form of a reference cloud (16-byte points), of a query cloud (8-byte pairs), the
# counting form of both
SLICES = (MP_STAGE_BYTES // 16, MP_STAGE_BYTES // 8, MP_SLICE2)

SortPlan = collections.namedtuple("SortPlan", "F2 F1 B1 G1 slice1")


def nc_cap(n, ppc=0.75):
    """cells the grid of n points may use (grid.hip grid_nc_cap)"""
    return int(min(2.0 * n / ppc + 4096.0, float(GRID_MAX_CELLS)))


def sort_plan(n, cap):
    """cellsort_mp.hip mp_plan for n points (non-finite ones included) and a cell cap"""
    f2 = MP_F2
    while f2 * MP_B2 * MP_MAX_B1 < cap + 1:
        f2 *= 2
    f1 = f2 * MP_B2
    g1 = max(1, min((n + 16383) // 16384, MP_MAX_G))
    return SortPlan(f2, f1, (cap + f1) // f1, g1, (n + g1 - 1) // g1)


def grid_of(pts, ppc=0.75):
    """(h, 1 / h, dims along the grid's axes, axis -> coordinate, origin, cell cap) for the finite rows of pts (n, >= 3) float32"""
    p = np.asarray(pts, np.float32)[:, :3]
    p = p[np.isfinite(p).all(1)]
    lo, hi = p.min(0), p.max(0)
    ext = hi - lo
    keep = (ext > np.float32(1e-6) * ext.max()) & (ext > 0)
    cap = nc_cap(len(pts), ppc)
    want = min(max(1.0, len(p) / float(np.float32(ppc))), float(cap))   # (the cap takes ppc as a double, the device as a float)
    h = (np.prod(ext[keep].astype(np.float64)) / want) ** (1.0 / keep.sum()) if keep.any() else 1.0
    order = np.argsort(ext, kind="stable")              # shortest, second, longest (ties in x, y, z order)
    ax = np.array([order[1], order[0], order[2]])       # rows run along the second shortest extent
    while True:
        hf = np.float32(h)
        inv = np.float32(1.0) / hf
        dims = np.minimum(np.floor(ext[ax].astype(np.float64) * np.float64(inv)) + 1.0, 1048576.0).astype(np.int64)
        if dims.prod() <= cap:
            return hf, inv, dims, ax, lo[ax], cap
        h *= 1.26


def cells_of(pts, grid):
    """linear cell of every finite row of pts in that grid (grid_device.hpp cell_id: float32, clamped)"""
    _, inv, dims, ax, org = grid[:5]
    p = np.asarray(pts, np.float32)[:, :3]
    p = p[np.isfinite(p).all(1)]
    t = np.minimum(np.maximum((p[:, ax] - org) * inv, np.float32(0)), (dims - 1).astype(np.float32)).astype(np.int64)
    return (t[:, 2] * dims[1] + t[:, 1]) * dims[0] + t[:, 0]


def bucket_sizes(pts, grid):
    """points in every last-level bucket that the grid has (the last one holds cell_start[ncells])"""
    f2 = sort_plan(len(pts), grid[5]).F2
    return np.bincount(cells_of(pts, grid) // f2, minlength=int(grid[2].prod()) // f2 + 1)


def level1_buckets(pts, grid):
    """level-1 bucket of every finite row of pts, ascending: the order level 1 leaves them in, up to the order inside a bucket"""
    return np.sort(cells_of(pts, grid) // sort_plan(len(pts), grid[5]).F1)


def slice_windows(b1, slice_len):
    """what every level-2 slice of slice_len elements sees of b1, the level-1 bucket of every element in grouped ascending
    order: (distinct level-1 buckets in the slice, elements whose bucket lies MP_WIN or more behind that of the slice's
    first element: those beyond its LDS window).  Which elements a slice holds depends on the bucket counts alone."""
    b1 = np.asarray(b1, np.int64)
    starts = np.arange(0, len(b1), slice_len)
    first = np.repeat(b1[starts], np.diff(np.append(starts, len(b1))))
    beyond = np.add.reduceat((b1 - first >= MP_WIN).astype(np.int64), starts)
    new = np.ones(len(b1), np.int64)
    new[1:] = b1[1:] != b1[:-1]
    new[starts] = 1
    return np.add.reduceat(new, starts), beyond


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
