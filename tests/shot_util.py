"""Scenes and file plumbing shared by tests/test_shot_cpu.py, tests/test_shot_gpu.py, tests/test_libm_f64_cpu.py and
tools/exp_shot.py: the patches the SHOT352 descriptor pipeline (reference src/comparator.cpp:941-986, the deterministic part
of processSHOT) is checked on -- points only, no colour is read -- and the binary files of build/shot_host and build/shot_driver
(tests/cpp/shot_host.cpp)."""
import subprocess
from pathlib import Path

import numpy as np

import fpfh_util

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "build" / "shot_host"
DRIVER = ROOT / "build" / "shot_driver"
BINS = 352
FIVE_RULE_SIZES = (4, 5, 6, 7)


def _five_rule():
    """40 isolated groups of 4, 5, 6 and 7 points (ten of each size), every group inside a cube of side 0.017 (all its points
    less than 0.03 apart: one row at either radius), the groups 0.25 apart, uniform in all three axes (relief in each).  The
    first group of every size holds an exact duplicate: its last point repeats its first.  Both "fewer than 5" rules are met
    exactly: a row counts p itself (4: NaN descriptor), the frame's `valid` counts neither p nor its copies (row 5: valid 4,
    NaN frame; row 6: valid 5, a frame -- or valid 4 for a point with a copy)."""
    rng = np.random.default_rng(57)
    groups = []
    for g in range(40):
        size = FIVE_RULE_SIZES[g % 4]
        centre = np.array([g % 7, g // 7, (g * 3) % 5], np.float64) * 0.25 + 0.3
        pts = centre + rng.uniform(0, 0.017, (size, 3))
        if g < 4:
            pts[-1] = pts[0]
        groups.append(pts)
    pts = np.concatenate(groups).astype(np.float32)
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


SMALL = dict(fpfh_util.SMALL)  # volume300, volume, slab, near-plane, isolated, non-finite, duplicates, short-rows
SMALL["five-rule"] = _five_rule
BIG = dict(fpfh_util.BIG)      # volume20000


def scene(name):
    return (SMALL.get(name) or BIG[name])()


def read_result(path):
    raw = Path(path).read_bytes()
    m = int(np.frombuffer(raw[:4], np.int32)[0])
    assert len(raw) == 4 + m * (BINS + 9 + 1) * 4
    desc = np.frombuffer(raw[4:4 + m * BINS * 4], np.float32).reshape(m, BINS)
    rf = np.frombuffer(raw[4 + m * BINS * 4:4 + m * (BINS + 9) * 4], np.float32).reshape(m, 9)
    index = np.frombuffer(raw[4 + m * (BINS + 9) * 4:], np.int32)
    return desc, rf, index


def run_host(points, tmp, tag="c", radii=(), normals=None, rf=None, lrf_out=False, timeout=600):
    """build/shot_host on a cloud: (desc (m, 352), rf (m, 9), index (m,), stdout), and the frames of ALL points float32 (n, 9)
    behind them with lrf_out=True.  radii: (normal, SHOT); normals: (n, 3) float32 read by the tool instead of fitted; rf: (n, 9)
    float32 by original index, taken as the frames instead of estimated"""
    tmp = Path(tmp)
    fin, fout = tmp / f"{tag}.in", tmp / f"{tag}.out"
    fpfh_util.write_cloud(fin, points)
    cmd = [str(HOST), str(fin), str(fout)]
    if radii:
        cmd += ["--radii"] + [repr(float(x)) for x in radii]
    if normals is not None:
        np.ascontiguousarray(normals, dtype=np.float32).tofile(tmp / f"{tag}.normals")
        cmd += ["--normals", str(tmp / f"{tag}.normals")]
    if rf is not None:
        np.ascontiguousarray(rf, dtype=np.float32).tofile(tmp / f"{tag}.rf")
        cmd += ["--rf", str(tmp / f"{tag}.rf")]
    if lrf_out:
        cmd += ["--lrf-out", str(tmp / f"{tag}.lrf")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = read_result(fout) + (r.stdout,)
    if lrf_out:
        res += (np.fromfile(tmp / f"{tag}.lrf", np.float32).reshape(len(points), 9),)
    return res


def run_driver(points, tmp, tag="d", timeout=600):
    """build/shot_driver (pcc::processSHOT through the library) on a cloud: (desc (m, 352), rf (m, 9), index (m,), stdout); the
    fallback descriptor of an empty result belongs to no point and carries the index -1"""
    fin, fout = Path(tmp) / f"{tag}.in", Path(tmp) / f"{tag}.out"
    fpfh_util.write_cloud(fin, points)
    r = subprocess.run([str(DRIVER), str(fin), str(fout)], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return read_result(fout) + (r.stdout,)


def run_libm(fn, values, tmp, tag="libm"):
    """build/shot_host --libm: lm_acos over (m,) float64, or lm_atan2 over (m, 2) float64 pairs (y, x): (m,) float64"""
    tmp = Path(tmp)
    v = np.ascontiguousarray(values, dtype=np.float64)
    v.tofile(tmp / f"{tag}.in")
    r = subprocess.run([str(HOST), "--libm", fn, str(tmp / f"{tag}.in"), str(tmp / f"{tag}.out")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = np.fromfile(tmp / f"{tag}.out", np.float64)
    assert len(out) == (len(v) if fn == "acos" else len(v.reshape(-1, 2)))
    return out


def run_jacobi(matrices, tmp, tag="jacobi"):
    """build/shot_host --jacobi over (m, 6) float64 (xx, xy, xz, yy, yz, zz): (eigenvalues (m, 3), V (m, 3, 3) with the
    eigenvectors in its columns, sweeps (m,) int)"""
    tmp = Path(tmp)
    a = np.ascontiguousarray(matrices, dtype=np.float64).reshape(-1, 6)
    a.tofile(tmp / f"{tag}.in")
    r = subprocess.run([str(HOST), "--jacobi", str(tmp / f"{tag}.in"), str(tmp / f"{tag}.out")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = np.fromfile(tmp / f"{tag}.out", np.float64).reshape(len(a), 13)
    return out[:, :3], out[:, 3:12].reshape(-1, 3, 3), out[:, 12].astype(np.int64)


def xyzrgb_records(points):
    return fpfh_util.xyzrgb_records(points)
