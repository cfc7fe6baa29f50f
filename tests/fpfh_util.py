"""Scenes and file plumbing shared by tests/test_fpfh_cpu.py, tests/test_fpfh_gpu.py and tools/exp_fpfh.py: the patches the
FPFH descriptor pipeline (reference src/comparator.cpp:824-875, processFPFH) is checked on -- points only, no colour is read --
and the binary files of build/fpfh_host and build/fpfh_driver (tests/cpp/fpfh_host.cpp)."""
import subprocess
from pathlib import Path

import numpy as np

import rift_util
from pointcloudcomparator_amd import synth

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "build" / "fpfh_host"
DRIVER = ROOT / "build" / "fpfh_driver"
BINS = 33


def _duplicates():
    """volume300 with 20 of its points repeated exactly, shuffled: d2 == 0 is skipped in the weighting, f4 == 0 in the SPFH, and both
    are still counted in the row's length"""
    p = rift_util.scene("volume300")[0]
    rng = np.random.default_rng(23)
    src = rng.choice(len(p), 20, replace=False)
    pts = np.concatenate([p, p[src]])
    order = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[order])


def duplicate_pairs(points):
    """(a, b) index pairs of points that are bit for bit the same"""
    _, first, inverse = np.unique(points, axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    out = []
    for i in range(len(points)):
        if first[inverse[i]] != i:
            out.append((int(first[inverse[i]]), i))
    return out


def _short_rows():
    """a lattice patch of one layer, 14 x 14 = 196 points 0.024 apart, jittered by 0.002 in the layer and 0.004 across it (a
    surface with relief: every normal is well defined): r = 0.05 rows of 5 (a corner) to 14 entries, all below one chunk.
    (A cubic 0.03 lattice was tried first: its neighbourhoods have no preferred normal and 5 ... 30 % of its points fail the
    condition of the vote-count test, whatever the seed.)"""
    g = np.stack(np.meshgrid(np.arange(14), np.arange(14), [0], indexing="ij"), -1).reshape(-1, 3).astype(np.float64) * 0.024
    g += np.random.default_rng(31).uniform(-1, 1, g.shape) * [0.002, 0.002, 0.004]
    return np.ascontiguousarray((g + 0.2).astype(np.float32))


# name -> points (n, 3) float32.  SMALL: the NumPy restatement (O(n^2) memory) can take them.
SMALL = {name: (lambda name=name: rift_util.scene(name)[0]) for name in ("volume300", "volume", "slab", "near-plane", "isolated", "non-finite")}
SMALL["duplicates"] = _duplicates
SMALL["short-rows"] = _short_rows
BIG = {"volume20000": lambda: rift_util.scene("volume20000")[0]}


def scene(name):
    return (SMALL.get(name) or BIG[name])()


def write_cloud(path, points):
    rift_util.write_cloud(path, points, np.zeros((len(points), 3), np.uint8))


def read_result(path):
    raw = Path(path).read_bytes()
    m = int(np.frombuffer(raw[:4], np.int32)[0])
    assert len(raw) == 4 + m * (BINS + 1) * 4
    hist = np.frombuffer(raw[4:4 + m * BINS * 4], np.float32).reshape(m, BINS)
    index = np.frombuffer(raw[4 + m * BINS * 4:], np.int32)
    return hist, index


def run_host(points, tmp, tag="c", radii=(), normals=None, counts=False, timeout=600):
    """build/fpfh_host on a cloud: (hist, index, stdout), and the SPFH vote counts int32 (n, 33) behind them with counts=True.
    radii: (normal, FPFH); normals: (n, 3) float32 read by the tool instead of fitted"""
    tmp = Path(tmp)
    fin, fout = tmp / f"{tag}.in", tmp / f"{tag}.out"
    write_cloud(fin, points)
    cmd = [str(HOST), str(fin), str(fout)]
    if radii:
        cmd += ["--radii"] + [repr(float(x)) for x in radii]
    if normals is not None:
        np.ascontiguousarray(normals, dtype=np.float32).tofile(tmp / f"{tag}.normals")
        cmd += ["--normals", str(tmp / f"{tag}.normals")]
    if counts:
        cmd += ["--counts", str(tmp / f"{tag}.counts")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = read_result(fout) + (r.stdout,)
    if counts:
        res += (np.fromfile(tmp / f"{tag}.counts", np.int32).reshape(len(points), BINS),)
    return res


def run_pairs(points, normals, pairs, tmp, tag="p"):
    """build/fpfh_host --pairs: the pair features of the listed (p, q): (f (m, 4) float32: f1 .. f4, ok (m,) bool, swapped (m,) bool)"""
    tmp = Path(tmp)
    fin, fnrm, fpq, fout = (tmp / f"{tag}.{x}" for x in ("in", "normals", "pairs", "out"))
    write_cloud(fin, points)
    np.ascontiguousarray(normals, dtype=np.float32).tofile(fnrm)
    pq = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    with open(fpq, "wb") as f:
        f.write(np.int32(len(pq)).tobytes())
        f.write(pq.tobytes())
    r = subprocess.run([str(HOST), "--pairs", str(fin), str(fnrm), str(fpq), str(fout)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rec = np.fromfile(fout, dtype=[("f", "<f4", 4), ("ok", "<i4"), ("swapped", "<i4")])
    assert len(rec) == len(pq)
    return rec["f"], rec["ok"] != 0, rec["swapped"] != 0


def run_driver(points, tmp, tag="d", timeout=600):
    """build/fpfh_driver (pcc::processFPFH through the library) on a cloud: (hist, index, stdout)"""
    fin, fout = Path(tmp) / f"{tag}.in", Path(tmp) / f"{tag}.out"
    write_cloud(fin, points)
    r = subprocess.run([str(DRIVER), str(fin), str(fout)], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return read_result(fout) + (r.stdout,)


def scene_pairs(points, normals, count=1250, seed=3):
    """(a, b): up to `count` ordered pairs of distinct points of cloud2 (finite normal) less than 0.05 apart, drawn without replacement"""
    ok = np.isfinite(points).all(1) & np.isfinite(normals).all(1)
    p = np.where(ok[:, None], points, 0).astype(np.float64)
    d = p[:, None, :] - p[None, :, :]
    near = ((d * d).sum(-1) < 0.05 * 0.05) & ok[None, :] & ok[:, None] & ~np.eye(len(p), dtype=bool)
    a, b = np.nonzero(near)
    pick = np.sort(np.random.default_rng(seed).choice(len(a), min(count, len(a)), replace=False))
    return a[pick], b[pick]


def xyzrgb_records(points):
    return synth.xyzrgb_records(points, np.zeros((len(points), 3), np.uint8))
