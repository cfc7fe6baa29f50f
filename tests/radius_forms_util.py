"""Scenes of tests/test_radius_forms_gpu.py: small clouds that put the radius search (knn.hip grid_radius and its kernels) on
every route its thresholds choose between, a model of those routes, and the exhaustive reference.
tests/test_radius_forms_cpu.py pins, without a GPU, what every scene must show.

The route a call takes cannot be observed; it follows from host conditions, restated here with the constants read from the sources:
  api.hip radius_fill_impl, knn.hip grid_radius    total >= RAD_WAVE_MEAN * nq: the wave-per-query fill (k_grid_radius_fill_wave), which
                                   delivers idx / d2 itself when the caller gives one; else one lane per query, memset, k_sort_rows, unpack
  k_grid_radius_fill_wave          row length <= 64 / <= 128 / <= ROW_LDS_MAX: emit<1> / <2> / <4> from LDS; longer: long_list, k_sort_rows
                                   bucket_sort_lds: a d2 bucket (BUCKET_N over [0, r2)) with more than BUCKET_FULL keys hands the row
                                   to the bitonic network
                                   the ball's box of cells: ny rows a layer, nrow rows in all; ny <= 8 and nrow <= 8 ny: the 8 x 8 form;
                                   chunks of RAD_ROWCAP rows; a chunk of up to RAD_FLAT_CAP candidates: span-end bit planes
  k_sort_rows                      64 / 128 / 256 / ROW_SORT_MAX: sort_row<1, 2, 4, 8>, beyond: sort_long_row
  radius_count_by_wave             (2 r / h + 1)^3 * n_valid / occupied cells >= RAD_COUNT_WAVE_MIN: the count goes by wave
  grid_radius                      gw = min(ceil(nq / 4), 8192) workgroups of 4 waves: a wave takes a second query -- the header it
                                   fetched a turn ahead -- only from 32 768 queries on (the `turns` scene)
The grid is that of tools/bucket_sizes.py (grid_params_device.hpp over the UNTRIMMED box: the GPU tests set PCC_OPT_GRID_TRIM = 0 and
hold the handle's cell count against the model's); cell_range and the chord clip of span_of are restated in float32.

Candidates of a chunk: `cand_box` counts the whole clipped box of cells, an upper bound; `cand` restates the chord clip the kernel
applies row by row (v_sqrt_f32 is good to an ulp, so it can differ by a cell where a chord ends on a cell face) and `cand_lo`
the same with the chord shortened by a thousandth, a lower bound.  What a scene claims rests on the bounds alone: a chunk is
beyond RAD_FLAT_CAP when it holds more HITS than that -- candidates inside the ball are never clipped away, and a ball of up to
RAD_ROWCAP rows is one chunk, so the row length says it --, it is within the cap when cand_box is, and it uses a bit plane when
cand_lo reaches it.

Every scene: read-only float32 clouds of a few thousand points (`crowd`: 20 000 references, 25 queries; `turns`: 81 references,
65 543 queries), seeded, with non-finite references and a non-finite query among them."""
import functools
import re
import sys
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import bucket_sizes as bs  # noqa: E402

_CSRC = ROOT / "pointcloudcomparator_amd" / "csrc"
f32 = np.float32


def _constant(text, name):
    """`constexpr <type> ..., NAME = <product of integers or 1u << k>, ...;` in `text`"""
    m = re.search(r"constexpr\s+(?:unsigned\s+)?int\s+(?:\w+\s*=[^,;]+,\s*)*" + name + r"\s*=\s*([^,;]+)[,;]", text)
    if m is None:
        raise LookupError(name + " not found in the sources")
    value = 1
    for term in m.group(1).split("*"):
        t = re.fullmatch(r"\s*(\d+)u?\s*(?:<<\s*(\d+))?\s*", term)
        if t is None:
            raise LookupError(name + " = " + m.group(1).strip() + " is no product of integers")
        value *= int(t.group(1)) << int(t.group(2) or 0)
    return value


def _row_steps(text):
    """the row lengths at which the fused fill's emit and k_sort_rows' sort_row change their register count (literals)"""
    emit = [int(v) for v in re.findall(r"if \(row_len <= (\d+)\) emit\(", text)]
    sort = [int(v) for v in re.findall(r"if \(len <= (\d+)\) sort_row<", text)]
    if len(emit) != 2 or len(sort) != 3:
        raise LookupError("the emit / sort_row ladders of knn.hip are not where they were")
    return tuple(sorted(set(emit + sort)))


_KNN, _INTERNAL = (_CSRC / "knn.hip").read_text(), (_CSRC / "pcc_internal.hpp").read_text()
CONSTANTS = {**{k: _constant(_KNN, k) for k in ("ROW_LDS_MAX", "ROW_SORT_MAX", "RAD_FLAT_CAP", "RAD_ROWCAP", "BUCKET_N", "BUCKET_FULL",
                                               "RAD_COUNT_WAVE_MIN")},
             "RAD_WAVE_MEAN": _constant(_INTERNAL, "RAD_WAVE_MEAN")}
ROW_LDS_MAX, ROW_SORT_MAX, RAD_FLAT_CAP, RAD_ROWCAP = (CONSTANTS[k] for k in ("ROW_LDS_MAX", "ROW_SORT_MAX", "RAD_FLAT_CAP", "RAD_ROWCAP"))
BUCKET_N, BUCKET_FULL, RAD_COUNT_WAVE_MIN, RAD_WAVE_MEAN = (CONSTANTS[k] for k in ("BUCKET_N", "BUCKET_FULL", "RAD_COUNT_WAVE_MIN", "RAD_WAVE_MEAN"))
ROW_STEPS = _row_steps(_KNN)
MAX_WAVES = 8192 * 4                             # grid_radius: gw = min(ceil(nq / 4), 8192) workgroups of 4 waves
# what the scenes below were aimed at, and the scenes to aim again when one of them moves
AIMED = {"ROW_LDS_MAX": (256, "ladder, ties: a rung on either side"), "ROW_SORT_MAX": (512, "ladder, ties: a rung on either side"),
         "RAD_FLAT_CAP": (8192, "crowd: both radii"), "RAD_ROWCAP": (121, "boxes: the radii 0.25 and 0.30"),
         "BUCKET_N": (128, "ties: the shells' buckets"), "BUCKET_FULL": (24, "ties: the rungs of 40 and 41"),
         "RAD_COUNT_WAVE_MIN": (200, "boxes: the radii 0.105 and 0.11"), "RAD_WAVE_MEAN": (24, "ladder: the far queries of ladder:long / :short")}
AIMED_ROW_STEPS = (64, 128, 256)                 # ladder, ties: a rung on either side of each


def radius2(radius):
    """the squared radius of every test: float32 of the double product (api.hip radius2)"""
    return f32(np.float64(radius) * np.float64(radius))


# ---- the reference ------------------------------------------------------------------------------------------------------------
def reference(ref, qry, radius):
    """CSR (offsets int64 [nq + 1], idx int32, d2 float32) of every reference with d2 < r2 for every query, rows ascending by
    (d2, index): exhaustive, float32, d = dx * dx; d = d + dy * dy; d = d + dz * dz with every operation rounded on its own (the bits of
    oracle.nn1_numpy and of the kernels).  A non-finite reference is no neighbour, a non-finite query finds nothing."""
    ref, qry = np.asarray(ref, f32)[:, :3], np.asarray(qry, f32)[:, :3]
    r2 = radius2(radius)
    vidx = np.flatnonzero(np.isfinite(ref).all(1)).astype(np.int32)
    r = ref[vidx]
    counts = np.zeros(len(qry), np.int64)
    idx_parts, d2_parts = [], []
    chunk = max(1, 4_000_000 // max(1, len(r)))
    for s in range(0, len(qry), chunk):
        q = qry[s:s + chunk]
        with np.errstate(invalid="ignore", over="ignore"):
            dx = q[:, None, 0] - r[None, :, 0]
            d = dx * dx
            dy = q[:, None, 1] - r[None, :, 1]
            d = d + dy * dy
            dz = q[:, None, 2] - r[None, :, 2]
            d = d + dz * dz
            hit = (d < r2) & np.isfinite(q).all(1)[:, None]
        rows, cols = np.nonzero(hit)
        dv = d[rows, cols]
        order = np.lexsort((vidx[cols], dv, rows))
        counts[s:s + chunk] = hit.sum(1)
        idx_parts.append(vidx[cols][order])
        d2_parts.append(dv[order])
    offsets = np.zeros(len(qry) + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    out = offsets, np.concatenate(idx_parts).astype(np.int32), np.concatenate(d2_parts).astype(f32)
    for a in out:
        a.setflags(write=False)
    return out


def rows_with_ties(offsets, d2):
    """queries with two neighbours at exactly the same distance (rows ascending)"""
    same = np.flatnonzero(d2[1:] == d2[:-1]) + 1
    row = np.searchsorted(offsets, same, side="right") - 1
    return np.unique(row[same > offsets[row]])


# ---- the route model ----------------------------------------------------------------------------------------------------------
def _cell_coord(v, org, inv, dim):
    return np.minimum(np.maximum((v - org) * inv, f32(0)), f32(dim - 1)).astype(np.int64)


def _cell_range(v, r, org, inv, dim):
    return _cell_coord(v - r, org, inv, dim), _cell_coord(v + r, org, inv, dim)


def grid_slack(grid):
    h, _, dims, _, org = grid[:5]
    far = f32(0)
    for a in range(3):
        far = max(far, abs(org[a]), abs(org[a] + f32(dims[a]) * h))
    return f32(4e-6) * far + f32(1e-6) * h


def occupied_cells(ref, grid):
    return len(np.unique(bs.cells_of(ref, grid)))


def count_expression(ref, grid, radius):
    """radius_count_by_wave's left side"""
    c = f32(2) * f32(radius) * grid[1] + f32(1)
    n_valid = int(np.isfinite(np.asarray(ref, f32)[:, :3]).all(1).sum())
    return float(c * c * c * (f32(n_valid) / f32(max(1, occupied_cells(ref, grid)))))


def model(ref, queries, radius, ppc=0.75, rows=None, per_query=True):
    """What the conditions above say of one call.  For the call: nq, total, wave_fill, count_expr, count_by_wave, turns (queries of
    the busiest wave), grid, ncells.  Per FINITE query (index array `finite`), unless per_query is off: ny, nrow, form8, chunks
    (candidates of every chunk, list of arrays: cand_box) and their maxima cand_box / cand / cand_lo, length (of the row, from the
    reference), bucket_max (keys in the row's fullest d2 bucket)."""
    ref, queries = np.asarray(ref, f32)[:, :3], np.asarray(queries, f32)[:, :3]
    offsets, idx, d2 = rows if rows is not None else reference(ref, queries, radius)
    g = bs.grid_of(ref, ppc)
    h, inv, dims, ax, org = g[:5]
    r, r2 = f32(radius), radius2(radius)
    m = types.SimpleNamespace(grid=g, ncells=int(dims.prod()), nq=len(queries), total=int(offsets[-1]), slack=grid_slack(g))
    m.wave_fill = m.total >= RAD_WAVE_MEAN * m.nq
    m.count_expr = count_expression(ref, g, radius)
    m.count_by_wave = m.count_expr >= RAD_COUNT_WAVE_MIN
    m.finite = np.flatnonzero(np.isfinite(queries).all(1))
    m.turns = -(-len(m.finite) // min(MAX_WAVES, 4 * ((m.nq + 3) // 4)))
    m.length = np.diff(offsets)[m.finite]
    row_of = np.repeat(np.arange(m.nq), np.diff(offsets))
    bucket = np.minimum(d2 * (f32(BUCKET_N) / r2), f32(BUCKET_N - 1)).astype(np.int64)
    m.bucket_max = np.bincount(row_of * BUCKET_N + bucket, minlength=m.nq * BUCKET_N).reshape(m.nq, BUCKET_N).max(1)[m.finite]
    if not per_query:
        return m
    cum = np.zeros((dims[2], dims[1], dims[0] + 1), np.int64)
    np.cumsum(np.bincount(bs.cells_of(ref, g), minlength=m.ncells).reshape(dims[2], dims[1], dims[0]), axis=2, out=cum[:, :, 1:])
    rr = r + m.slack
    inf = f32(np.inf)

    def gaps(v, c0, c1, dim, o):
        c = np.arange(c0, c1 + 1)
        lo = np.where(c == 0, -inf, o + c.astype(f32) * h)
        hi = np.where(c == dim - 1, inf, o + (c + 1).astype(f32) * h)
        return np.maximum(np.maximum(lo - v, v - hi) - m.slack, f32(0)).astype(f32)

    m.ny, m.nrow, m.chunks, m.cand_box, m.cand, m.cand_lo = [], [], [], [], [], []
    for q in queries[m.finite]:
        u = q[ax]
        (x0, x1), (y0, y1), (z0, z1) = (_cell_range(u[a], rr, org[a], inv, int(dims[a])) for a in range(3))
        ny, nz = int(y1 - y0 + 1), int(z1 - z0 + 1)
        starts = np.arange(0, ny * nz, RAD_ROWCAP)
        box = (cum[z0:z1 + 1, y0:y1 + 1, x1 + 1] - cum[z0:z1 + 1, y0:y1 + 1, x0]).ravel()     # rows in the kernel's order: z outer, y inner
        gy, gz = gaps(u[1], y0, y1, int(dims[1]), org[1]), gaps(u[2], z0, z1, int(dims[2]), org[2])
        g2 = (gz * gz)[:, None] + (gy * gy)[None, :]
        zz, yy = np.meshgrid(np.arange(z0, z1 + 1), np.arange(y0, y1 + 1), indexing="ij")
        clipped = []
        for shrink_g, shrink_c in ((f32(0.9999), f32(1.00001)), (f32(1.001), f32(0.999))):
            rem = rr * rr - g2 * shrink_g
            ok = rem >= 0
            xa, xb = _cell_range(u[0], np.sqrt(np.where(ok, rem, f32(0))).astype(f32) * shrink_c + m.slack, org[0], inv, int(dims[0]))
            xa, xb = np.maximum(xa, x0), np.minimum(xb, x1)
            ok &= xa <= xb
            clipped.append(np.where(ok, cum[zz, yy, np.where(ok, xb + 1, 0)] - cum[zz, yy, np.where(ok, xa, 0)], 0).ravel())
        m.ny.append(ny)
        m.nrow.append(ny * nz)
        m.chunks.append(np.add.reduceat(box, starts))
        m.cand_box.append(int(m.chunks[-1].max()))
        m.cand.append(int(np.add.reduceat(clipped[0], starts).max()))
        m.cand_lo.append(int(np.add.reduceat(clipped[1], starts).max()))
    for k in ("ny", "nrow", "cand_box", "cand", "cand_lo"):
        setattr(m, k, np.array(getattr(m, k), np.int64))
    m.form8 = (m.ny <= 8) & (m.nrow <= 8 * m.ny)
    return m


# ---- the scenes ---------------------------------------------------------------------------------------------------------------
LADDER = (0, 1, 2, 23, 24, 25, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
TIES_FULL = {40: (24, 10, 6), 41: (25, 10, 6)}   # rungs whose fullest bucket holds exactly BUCKET_FULL keys, and one more
R = 0.05                                         # the radius of the ladder and ties scenes; clusters lie within 0.8 R of their centre
SPACING = 1.0                                    # of the 3 x 3 x 3 lattice of cluster centres: 20 radii
SHELL_SCALE = 2.0 ** -11                         # the ties scene's integer lattice: offsets up to 81 units, every d2 exact in float32
# ladder: 21 centres + 1 non-finite query + far queries of empty rows.  The rungs hold 6027 references: 24 * 251 = 6024 is the last
# query count with total >= 24 nq; 252 is the first below but a multiple of 4 (the launch's waves: 4 * ceil(nq / 4)), so 253
LADDER_NQ = {"long": 251, "short": 253}
BOXES_RADII = (0.10, 0.105, 0.11, 0.16, 0.22, 0.25, 0.30, 0.45)
CROWD_PPC, CROWD_RADII = 64.0, (0.6, 0.34)
TURNS_NQ, TURNS_RADIUS = 2 * MAX_WAVES + 7, 0.6

Scene = types.SimpleNamespace


def _sites():
    k = np.arange(27)
    return np.stack([k % 3, k // 3 % 3, k // 9], 1).astype(np.float64) * SPACING


def _freeze(*arrays):
    out = []
    for a in arrays:
        a = np.ascontiguousarray(a, dtype=f32)
        a.setflags(write=False)
        out.append(a)
    return out


def _far_queries(rng, m):
    """m queries with nothing within reach: inside the lattice's box and up to 0.2 outside it, 0.2 and more from every site"""
    p = rng.random((8 * m + 64, 3)) * (2 * SPACING + 0.4) - 0.2
    far = np.sqrt(((p[:, None] - _sites()[None]) ** 2).sum(2)).min(1) > 0.2
    return p[far][:m]


def _clusters(rng, rungs, offsets_of):
    """references of the rungs' clusters (rung j at lattice site j), shuffled, three non-finite rows among them; and the centres"""
    sites = _sites()
    pts = [sites[j] + offsets_of(length) for j, length in enumerate(rungs)]
    pts.append(np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf]]))
    pts = np.concatenate(pts)
    return pts[rng.permutation(len(pts))], sites[:len(rungs)]


def _queries(rng, centres, n_total, n_tail=0):
    """the centres (query `rung_query[j]` is rung j's), one non-finite query and far queries, shuffled; the last n_tail are far ones"""
    head = np.concatenate([centres, [[0.5, np.nan, 0.5]], _far_queries(rng, n_total - len(centres) - 1)])
    perm = rng.permutation(len(head) - n_tail)
    rung_query = np.argsort(perm)[:len(centres)]
    return np.concatenate([head[:len(head) - n_tail][perm], head[len(head) - n_tail:]]), rung_query


@functools.lru_cache(maxsize=None)
def _shells():
    """three shells of the integer lattice (vectors of equal squared length n, up to 0.8 R / SHELL_SCALE long) with the most
    vectors, their n two d2 buckets and more apart: (n, vectors) ascending"""
    lim = int(0.8 * R / SHELL_SCALE)
    c = np.arange(-lim, lim + 1)
    v = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)
    n = (v * v).sum(1)
    keep = n <= lim * lim
    v, n = v[keep], n[keep]
    r3 = np.bincount(n)
    apart = int(2 * R * R / BUCKET_N / SHELL_SCALE ** 2) + 1
    chosen = []
    for cand in np.argsort(-r3, kind="stable"):
        if all(abs(int(cand) - o) >= apart for o in chosen):
            chosen.append(int(cand))
        if len(chosen) == 3:
            break
    return [(k, v[n == k]) for k in sorted(chosen)]


def ties_split(length):
    """references of a ties rung on the three shells, nearest first"""
    return TIES_FULL.get(length, (length - length // 3 - length // 4, length // 3, length // 4))


@functools.lru_cache(maxsize=None)
def scene(name):
    """ref, qry (read-only float32 (n, 3)), ppc, radii; ladder / ties: rungs and rung_query (the query at rung j's centre)"""
    kind, _, arg = name.partition(":")
    sc = Scene(name=name, ppc=0.75)
    if kind == "ladder":
        rng = np.random.default_rng(0x2AD1)

        def ball(length):                        # uniform in the ball of 0.8 R: no two distances alike
            d = rng.normal(size=(length, 3))
            return d / np.linalg.norm(d, axis=1, keepdims=True) * (0.8 * R * rng.random((length, 1)) ** (1 / 3))
        ref, centres = _clusters(rng, LADDER, ball)
        qry, sc.rung_query = _queries(rng, centres, LADDER_NQ["short"], n_tail=LADDER_NQ["short"] - LADDER_NQ["long"])
        qry = qry[:LADDER_NQ[arg]]               # (ladder:long is ladder:short less its last far queries)
        sc.rungs, sc.radii = LADDER, (R,)
    elif kind == "ties":
        rng = np.random.default_rng(0x71E5)
        sc.rungs = LADDER + tuple(TIES_FULL)

        def shells(length):
            return np.concatenate([v[rng.choice(len(v), k, replace=False)] for (_, v), k in zip(_shells(), ties_split(length))]) * SHELL_SCALE
        ref, centres = _clusters(rng, sc.rungs, shells)
        qry, sc.rung_query = _queries(rng, centres, len(sc.rungs) + 10)
        sc.radii = (R,)
    elif kind == "boxes":
        rng = np.random.default_rng(0xB0C5)
        ref = rng.random((6000, 3))
        ref[0], ref[1] = 0, 1
        ref[13::2000, 1] = (np.nan, np.inf, -np.inf)
        qry = np.concatenate([rng.random((280, 3)), rng.random((20, 3)) * 1.3 - 0.15, [[np.inf, 0.5, 0.5]]])
        qry = qry[rng.permutation(len(qry))]
        sc.radii = BOXES_RADII
    elif kind == "crowd":
        rng = np.random.default_rng(0xC20D)
        ref = rng.random((20000, 3))
        ref[0], ref[1] = 0, 1
        ref[13::7000, 2] = (np.nan, np.inf, -np.inf)
        ref = ref.astype(f32)
        h, _, dims, ax, org = bs.grid_of(ref, CROWD_PPC)[:5]
        # every query near the centre of a cell (a tenth of a cell off at most): the ball's box is the same whole number of cells
        # either way.  16 of the 27 inner cells, 8 of the outermost layer, where the ball leaves the grid
        inner = rng.permutation(27)[:16]
        cells = np.concatenate([np.stack([inner % 3, inner // 3 % 3, inner // 9], 1) + 2, rng.choice([0, int(dims.min()) - 1], (8, 3))])
        u = org.astype(np.float64) + (cells + 0.5 + rng.uniform(-0.1, 0.1, cells.shape)) * float(h)
        qry = np.empty_like(u)
        qry[:, ax] = u
        qry = np.concatenate([qry, [[0.5, 0.5, np.nan]]])[rng.permutation(25)]
        sc.ppc, sc.radii = CROWD_PPC, CROWD_RADII
    elif kind == "turns":
        rng = np.random.default_rng(0x7025)
        ref = rng.random((81, 3))
        ref[40, 0] = np.nan
        qry = rng.random((TURNS_NQ, 3))
        qry[12345, 2] = np.inf
        sc.radii = (TURNS_RADIUS,)
    else:
        raise KeyError(name)
    sc.ref, sc.qry = _freeze(ref, qry)
    return sc


SCENES = ("ladder:long", "ladder:short", "ties", "boxes", "crowd", "turns")
_RADII = {"ladder": (R,), "ties": (R,), "boxes": BOXES_RADII, "crowd": CROWD_RADII, "turns": (TURNS_RADIUS,)}
CASES = [(name, radius) for name in SCENES for radius in _RADII[name.partition(":")[0]]]   # (no scene is built at import)


@functools.lru_cache(maxsize=None)
def reference_of(name, radius):
    sc = scene(name)
    return reference(sc.ref, sc.qry, radius)


@functools.lru_cache(maxsize=None)
def model_of(name, radius):
    sc = scene(name)
    return model(sc.ref, sc.qry, radius, sc.ppc, rows=reference_of(name, radius), per_query=name != "turns")


# ---- the clouds of the normals tests (self rows through the keys route: normals.hip radius_csr) --------------------------------
NORMALS_LONG_RADIUS = 0.9
NORMALS_LONG_SEED = 17                           # the first seed whose cloud has no tied row (0 to 16 have one to seven)


def normals_long_cloud(seed=NORMALS_LONG_SEED):
    """640 points in the unit cube, one non-finite: self rows of 257 to 639 neighbours at NORMALS_LONG_RADIUS, most beyond 512"""
    rng = np.random.default_rng([0x90A1, seed])
    p = rng.random((640, 3))
    p[77, 1] = np.nan
    return _freeze(p)[0]
