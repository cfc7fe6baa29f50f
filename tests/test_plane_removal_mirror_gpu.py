"""pcc::removePlanes (include/pcc/comparator_nn.hpp) against the SACSegmentation + ExtractIndices loop it replaces
(tests/cpp/plane_removal_driver.cpp), and the example CLI's -e path with and without --planes-device."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from ply_util import write_ply

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_cpp_remove_planes_equals_the_loop(gpu):
    exe = ROOT / "build" / "plane_removal_driver"
    if not exe.exists():
        subprocess.check_call(["make", "build/plane_removal_driver"], cwd=ROOT)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plane removal driver ok" in r.stdout and "DIFFERENT" not in r.stdout
    assert "stop 1.0: 0 planes" in r.stdout and "grown" in r.stdout


def _scene(seed, shift=(0.0, 0.0, 0.0)):
    """tests/test_cli_gpu.py's scene at a third of the size: a floor and four boxes on a 0.03 lattice with +-0.002 jitter (no two
    points share a 0.025 voxel), plus a wall, so that the loop removes two planes"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(36), np.arange(36), indexing="ij"), -1).reshape(-1, 2) * 0.03
    floor = np.concatenate([g, np.zeros((len(g), 1))], 1)
    wall = np.concatenate([np.full((len(g), 1), -0.06), g + 0.03], 1)
    c = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 3) * 0.03
    boxes = [c + o for o in [(0.15, 0.15, 0.3), (0.75, 0.15, 0.45), (0.15, 0.75, 0.6), (0.75, 0.75, 0.3)]]
    pts = np.concatenate([floor, wall] + boxes)
    pts = pts + rng.uniform(-0.002, 0.002, pts.shape) + 0.01 + np.asarray(shift)
    return np.ascontiguousarray(pts[rng.permutation(len(pts))].astype(np.float32))


def test_cli_planes_device_prints_and_writes_the_same(gpu, tmp_path):
    exe = ROOT / "build" / "comparator"
    if not exe.exists():
        subprocess.check_call(["make", "cli"], cwd=ROOT)
    fa, fb = tmp_path / "a.ply", tmp_path / "b.ply"
    write_ply(fa, _scene(1), fmt="binary")
    write_ply(fb, _scene(2, shift=(0.004, -0.003, 0.002)), fmt="binary")
    runs = []
    for flags in ([], ["--planes-device"]):
        res = tmp_path / f"results{len(runs)}.txt"
        r = subprocess.run([str(exe), "-e", *flags, str(fa), str(fb), "--results", str(res)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 1, r.stdout + r.stderr  # the reference always returns 1 (src/comparator.cpp:1704)
        runs.append((r.stdout, res.read_text()))
    assert runs[0][0] == runs[1][0]
    assert runs[0][1] == runs[1][1] and runs[0][1]
    out = runs[1][0]
    assert out.count("PointCloud representing the planar component:") >= 4  # two planes per scene
    assert out.count("PointCloud representing the Cluster:") == 8
