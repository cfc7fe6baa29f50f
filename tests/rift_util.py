"""Scenes and file plumbing shared by tests/test_rift_cpu.py, tests/test_rift_gpu.py and tools/exp_rift.py: the coloured
patches the RIFT descriptor pipeline (reference src/comparator.cpp:590-684) is checked on, and the binary files of
build/rift_host and build/rift_driver (tests/cpp/rift_host.cpp)."""
import subprocess
from pathlib import Path

import numpy as np

from pointcloudcomparator_amd import synth

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "build" / "rift_host"
DRIVER = ROOT / "build" / "rift_driver"


def _isolated():
    """a dense patch plus points that each compaction removes: singles and pairs (no normal: first compaction), and hubs
    whose three neighbours each see only the hub (the hub keeps a normal, its neighbours do not, so its row of cloud2 holds
    one entry: NaN gradient, NaN histogram, second compaction).  Shuffled, so that kept indices are not a prefix."""
    p, rgb = synth.rift_cloud(500, 11)
    rng = np.random.default_rng(5)
    extra = []
    for k in range(6):
        hub = np.array([0.5 + 0.3 * k, 0.5, 0.5])
        extra += [hub, hub + [0.025, 0.001, 0.0], hub + [0.0, 0.025, 0.002], hub + [0.001, 0.0, -0.025]]  # spokes 0.035 apart
    for k in range(6):
        extra.append(np.array([-0.5 - 0.2 * k, 0.1, 0.3]))                                  # singles
    for k in range(3):
        a = np.array([0.2, -0.5 - 0.2 * k, 0.1])
        extra += [a, a + [0.01, 0.0, 0.0]]                                                  # pairs
    extra = np.array(extra, dtype=np.float32)
    pts = np.concatenate([p, extra])
    col = np.concatenate([rgb, rng.integers(0, 256, (len(extra), 3), dtype=np.uint8)])
    order = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[order]), np.ascontiguousarray(col[order])


def _nonfinite():
    p, rgb = synth.rift_cloud(500, 13)
    p = p.copy()
    bad = np.arange(7, 500, 41)
    p[bad[0::3], 0] = np.nan
    p[bad[1::3], 1] = np.inf
    p[bad[2::3], 2] = -np.inf
    return p, rgb


# name -> (points (n, 3) float32, rgb (n, 3) uint8).  SMALL: the NumPy restatement (O(n^2) memory) can take them.
SMALL = {
    "volume": lambda: synth.rift_cloud(600, 7),
    "volume300": lambda: synth.rift_cloud(300, 7),
    "slab": lambda: synth.rift_cloud(600, 7, flat=0.004),
    "near-plane": lambda: synth.rift_cloud(600, 7, flat=1e-5),
    "isolated": _isolated,
    "non-finite": _nonfinite,
}
# one cluster of 20 000 points at the density of the volume scene (600 points per 0.12 m cube)
BIG = {"volume20000": lambda: synth.rift_cloud(20000, 17, extent=0.386)}


def scene(name):
    return (SMALL.get(name) or BIG[name])()


def write_cloud(path, points, rgb):
    rec = np.zeros(len(points), dtype=[("p", "<f4", 3), ("c", "<u4")])
    rec["p"] = points
    rec["c"] = synth.pack_rgb(rgb)
    with open(path, "wb") as f:
        f.write(np.int32(len(points)).tobytes())
        f.write(rec.tobytes())


def read_result(path):
    raw = Path(path).read_bytes()
    m = int(np.frombuffer(raw[:4], np.int32)[0])
    hist = np.frombuffer(raw[4:4 + m * 128], np.float32).reshape(m, 32)
    index = np.frombuffer(raw[4 + m * 128:4 + m * 132], np.int32)
    assert len(raw) == 4 + m * 132
    return hist, index


def run_tool(exe, points, rgb, tmp, tag="c", timeout=600, radii=()):
    """build/rift_host or build/rift_driver on a cloud: (hist, index, stdout).  radii (rift_host only): normal, gradient, RIFT"""
    fin, fout = Path(tmp) / f"{tag}.in", Path(tmp) / f"{tag}.out"
    write_cloud(fin, points, rgb)
    r = subprocess.run([str(exe), str(fin), str(fout)] + [repr(float(x)) for x in radii], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return read_result(fout) + (r.stdout,)
