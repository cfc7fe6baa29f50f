"""Scenes and file plumbing shared by tests/test_sift_cpu.py, tests/test_sift_gpu.py and tools/exp_sift.py: the coloured
clouds the SIFT keypoint detector (reference src/comparator.cpp:435-469, processSift) is checked on, and the binary files of
build/sift_host and build/sift_driver (tests/cpp/sift_host.cpp, tests/cpp/sift_driver.cpp)."""
import re
import subprocess
from pathlib import Path

import numpy as np

import rift_util
from pointcloudcomparator_amd import synth

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "build" / "sift_host"
DRIVER = ROOT / "build" / "sift_driver"
DEFAULTS = (0.005, 5, 5, 0.001)  # min_scale, nr_octaves, nr_scales_per_octave, min_contrast (the reference's four constants)


def _tiny(m):
    """m distinct points of a 3 x 3 x 3 lattice with spacing 0.005, each in a voxel of its own at leaf 0.005 (and at most eight
    voxels at leaf 0.01: a second octave never passes the 25-point gate)"""
    k = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij"), -1).reshape(-1, 3)[:m]
    p = (k * 0.005 + 0.0025).astype(np.float32)
    rgb = np.stack([(37 * k[:, 0] + 101 * k[:, 1] + 53 * k[:, 2]) % 256, (91 * k[:, 0] + 17 * k[:, 2]) % 256, (200 - 60 * k[:, 1]) % 256], -1)
    return np.ascontiguousarray(p), np.ascontiguousarray(rgb.astype(np.uint8))


def _dups():
    p, rgb = synth.rift_cloud(300, 7)
    again = np.arange(5, 300, 10)  # 30 points
    return np.ascontiguousarray(np.concatenate([p, p[again]])), np.ascontiguousarray(np.concatenate([rgb, rgb[again]]))


# name -> (points (n, 3) float32, rgb (n, 3) uint8).  SMALL: the NumPy restatement (O(n^2) memory) can take them.
SMALL = {
    "sift300": lambda: synth.rift_cloud(300, 7),
    "sift600": lambda: synth.rift_cloud(600, 7),
    "sift2000": lambda: synth.rift_cloud(2000, 17, extent=0.18),
}
EDGE = {
    "tiny24": lambda: _tiny(24),
    "tiny25": lambda: _tiny(25),
    "dups": _dups,
    "non-finite": rift_util._nonfinite,
}
BIG = {"sift8000": lambda: synth.rift_cloud(8000, 17, extent=0.285)}


def scene(name):
    return (SMALL.get(name) or EDGE.get(name) or BIG[name])()


def read_keypoints(raw):
    """(keypoints (m, 4) float32, rest of the bytes)"""
    m = int(np.frombuffer(raw[:4], np.int32)[0])
    return np.frombuffer(raw[4:4 + m * 16], np.float32).reshape(m, 4), raw[4 + m * 16:]


def read_dump(path):
    """every processed octave of a sift_host dump: dict(cloud (n, 3), rgb words (n,), inten (n,), dog (n, columns), scales)"""
    raw = Path(path).read_bytes()
    n_oct = int(np.frombuffer(raw[:4], np.int32)[0])
    at, out = 4, []
    for _ in range(n_oct):
        n, s = (int(v) for v in np.frombuffer(raw[at:at + 8], np.int32))
        at += 8
        rec = np.frombuffer(raw[at:at + n * 16], dtype=[("p", "<f4", 3), ("c", "<u4")])
        at += n * 16
        inten = np.frombuffer(raw[at:at + n * 4], np.float32)
        at += n * 4
        dog = np.frombuffer(raw[at:at + n * (s - 1) * 4], np.float32).reshape(n, s - 1)
        at += n * (s - 1) * 4
        scales = np.frombuffer(raw[at:at + s * 4], np.float32)
        at += s * 4
        out.append(dict(cloud=rec["p"], rgb=rec["c"], inten=inten, dog=dog, scales=scales))
    assert at == len(raw)
    return out


def run_host(points, rgb, tmp, tag="c", params=DEFAULTS, dump=False, timeout=600):
    """build/sift_host on a cloud: dict(keypoints (m, 4), ids (m, 3) octave / point / column, info (the printed line as a
    dict of strings), octaves (with dump))"""
    fin, fout, fdump = Path(tmp) / f"{tag}.in", Path(tmp) / f"{tag}.out", Path(tmp) / f"{tag}.dump"
    rift_util.write_cloud(fin, points, rgb)
    args = [str(HOST), str(fin), str(fout)]
    if dump or tuple(params) != DEFAULTS:
        args += [repr(float(params[0])), str(int(params[1])), str(int(params[2])), repr(float(params[3]))]
    if dump:
        args.append(str(fdump))
    r = subprocess.run(args, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    kp, rest = read_keypoints(fout.read_bytes())
    ids = np.frombuffer(rest, np.int32).reshape(len(kp), 3)
    info = dict(re.findall(r"(\w+)=(\S+)", r.stdout))
    return dict(keypoints=kp, ids=ids, info=info, octaves=read_dump(fdump) if dump else None)


def run_driver(points, rgb, tmp, tag="d", timeout=600):
    """build/sift_driver on a cloud: (keypoints (m, 4), histograms (n_des, 32), indices into the snapped cloud, stdout)"""
    fin, fout = Path(tmp) / f"{tag}.in", Path(tmp) / f"{tag}.out"
    rift_util.write_cloud(fin, points, rgb)
    r = subprocess.run([str(DRIVER), str(fin), str(fout)], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    kp, rest = read_keypoints(fout.read_bytes())
    n_des = int(np.frombuffer(rest[:4], np.int32)[0])
    hist = np.frombuffer(rest[4:4 + n_des * 128], np.float32).reshape(n_des, 32)
    index = np.frombuffer(rest[4 + n_des * 128:], np.int32)
    assert len(index) == n_des
    return kp, hist, index, r.stdout
