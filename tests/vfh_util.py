"""Scenes and file plumbing shared by tests/test_vfh_cpu.py, tests/test_vfh_gpu.py and tools/exp_vfh.py: the clouds the VFH
descriptor (reference src/comparator.cpp:482-516, processVHF) and matchVHF (:471-480) are checked on -- points only, no colour
is read -- and the binary files of build/vfh_host and build/vfh_driver (tests/cpp/vfh_host.cpp)."""
import subprocess
from pathlib import Path

import numpy as np

import fpfh_util
from pointcloudcomparator_amd import synth

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "build" / "vfh_host"
DRIVER = ROOT / "build" / "vfh_driver"
BINS = 308
COUNTERS = 263
CENTRE = np.array([0.5, 0.25, 0.5], np.float32)  # of the centroid-hit scene


def _centroid_hit():
    """a 5 x 5 x 5 lattice of spacing 1 / 128 around the lattice point CENTRE, shuffled: every coordinate is a multiple of 2^-7
    below 1, so every partial sum of the three float chains is exact, the sum is 125 x CENTRE and the centroid IS the centre
    point, bit for bit -- that point has f4 == 0 and gives no pair-feature vote, but it still counts in n."""
    g = np.stack(np.meshgrid(*[np.arange(-2, 3)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32) / np.float32(128)
    p = (g + CENTRE).astype(np.float32)
    return np.ascontiguousarray(p[np.random.default_rng(41).permutation(len(p))])


def _sized(n):
    return lambda: synth.rift_cloud(n, 29)[0]


# name -> points (n, 3) float32, every point finite.  SMALL: the NumPy restatement can take them.
SMALL = {name: fpfh_util.SMALL[name] for name in ("volume300", "volume", "slab", "near-plane", "isolated", "duplicates")}
SMALL["centroid-hit"] = _centroid_hit
# the wave edges of every kernel and the tile edge of the centroid chains (512 points a tile)
EDGES = {f"n{n}": _sized(n) for n in (2, 63, 64, 65, 511, 512, 513)}
BIG = {"volume20000": fpfh_util.BIG["volume20000"]}


def scene(name):
    return (SMALL.get(name) or EDGES.get(name) or BIG[name])()


write_cloud = fpfh_util.write_cloud


def write_descriptors(path, hist):
    h = np.ascontiguousarray(hist, dtype=np.float32).reshape(-1, BINS)
    with open(path, "wb") as f:
        f.write(np.int32(len(h)).tobytes())
        f.write(h.tobytes())


def read_result(path):
    """(m, 308) float32, m = 0 or 1"""
    raw = Path(path).read_bytes()
    m = int(np.frombuffer(raw[:4], np.int32)[0])
    assert m in (0, 1) and len(raw) == 4 + m * BINS * 4
    return np.frombuffer(raw[4:], np.float32).reshape(m, BINS)


def run_host(points, tmp, tag="c", radius=None, normals=None, counts=False, votes=False, timeout=600, check=True):
    """build/vfh_host on a cloud: dict with hist (m, 308), stdout, returncode and -- on request -- counts int32 (263,) and votes
    int32 (n, 4).  radius: the normal radius; normals: (n, 3) float32 read by the tool instead of fitted"""
    tmp = Path(tmp)
    fin, fout = tmp / f"{tag}.in", tmp / f"{tag}.out"
    write_cloud(fin, points)
    cmd = [str(HOST), str(fin), str(fout)]
    if radius is not None:
        cmd += ["--radius", repr(float(radius))]
    if normals is not None:
        np.ascontiguousarray(normals, dtype=np.float32).tofile(tmp / f"{tag}.normals")
        cmd += ["--normals", str(tmp / f"{tag}.normals")]
    if counts:
        cmd += ["--counts", str(tmp / f"{tag}.counts")]
    if votes:
        cmd += ["--votes", str(tmp / f"{tag}.votes")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    res = {"stdout": r.stdout, "stderr": r.stderr, "returncode": r.returncode}
    if check:
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    if r.returncode == 0:
        res["hist"] = read_result(fout)
        if counts:
            res["counts"] = np.fromfile(tmp / f"{tag}.counts", np.int32)
            assert res["counts"].shape == (COUNTERS,)
        if votes:
            res["votes"] = np.fromfile(tmp / f"{tag}.votes", np.int32).reshape(-1, 4)
    return res


def run_match(h1, h2, tmp, tag="m"):
    """build/vfh_host --match: the (n1, n2) float64 distances"""
    tmp = Path(tmp)
    f1, f2, fout = (tmp / f"{tag}.{x}" for x in ("h1", "h2", "out"))
    write_descriptors(f1, h1)
    write_descriptors(f2, h2)
    r = subprocess.run([str(HOST), "--match", str(f1), str(f2), str(fout)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    n1, n2 = (len(np.asarray(h).reshape(-1, BINS)) for h in (h1, h2))
    return np.fromfile(fout, np.float64).reshape(n1, n2)


def run_driver(points, tmp, tag="d", timeout=600):
    """build/vfh_driver (pcc::processVHF through the library) on a cloud: (hist (m, 308), stdout)"""
    fin, fout = Path(tmp) / f"{tag}.in", Path(tmp) / f"{tag}.out"
    write_cloud(fin, points)
    r = subprocess.run([str(DRIVER), str(fin), str(fout)], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return read_result(fout), r.stdout


def run_driver_match(a, b, tmp, tag="dm", timeout=600):
    """build/vfh_driver --match: pcc::matchVHF(pcc::processVHF(a), pcc::processVHF(b)) as a float64"""
    f1, f2, fout = (Path(tmp) / f"{tag}.{x}" for x in ("in1", "in2", "out"))
    write_cloud(f1, a)
    write_cloud(f2, b)
    r = subprocess.run([str(DRIVER), "--match", str(f1), str(f2), str(fout)], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return float(np.fromfile(fout, np.float64)[0])


def xyzrgb_records(points):
    return synth.xyzrgb_records(points, np.zeros((len(points), 3), np.uint8))
