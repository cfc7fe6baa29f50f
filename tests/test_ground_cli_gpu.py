"""build/ground_segments (tests/cpp/ground_segments.cpp over include/pcc/ground.hpp): the two PLY files the reference's
ground_segmentation writes (src/segmentation.cpp:330-387), against Index.ground_segmentation."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from pointcloudcomparator_amd import capi
import ground_util as gu
from ply_util import write_ply

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "build" / "ground_segments"


def read_xyz(path):
    raw = Path(path).read_bytes()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode().splitlines()
    assert lines[0] == "ply" and "binary_little_endian" in lines[1] and [l for l in lines if l.startswith("property")] == [
        "property float x", "property float y", "property float z"]
    n = int([l for l in lines if l.startswith("element vertex")][0].split()[-1])
    assert len(body) == 12 * n
    return np.frombuffer(body, "<f4").reshape(n, 3)


def test_tool_writes_what_the_python_call_gives(gpu, tmp_path):
    if not EXE.exists():
        subprocess.check_call(["make", "build/ground_segments"], cwd=ROOT)
    pts = gu.terrain(1500, 4)
    src, prefix = tmp_path / "in.ply", tmp_path / "tile"
    write_ply(src, pts, fmt="binary")
    p = gu.TERRAIN
    args = ["0.05", str(p["max_window_size"]), str(p["slope"]), str(p["initial_distance"]), str(p["max_distance"]), str(p["cell_size"]),
            str(p["base"]), "1"]
    r = subprocess.run([str(EXE), str(src), str(prefix), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    with capi.Index(np.zeros((1, 3), np.float32)) as ix:
        cloud = np.zeros((len(pts), 4), np.float32)  # pcl::PointXYZ records, as the tool passes them
        cloud[:, :3], cloud[:, 3] = pts, 1.0
        want = ix.ground_segmentation(cloud, leaf=0.05, **p)
    ground, obj = read_xyz(str(prefix) + "_ground.ply"), read_xyz(str(prefix) + "_object.ply")
    assert 0 < len(ground) < len(want["filtered"])
    assert np.array_equal(ground.view(np.uint32), want["ground_points"][:, :3].view(np.uint32))
    assert np.array_equal(obj.view(np.uint32), np.ascontiguousarray(want["object_points"][:, :3]).view(np.uint32))
    assert f"Ground cloud after filtering: {len(ground)}" in r.stdout and f"Object cloud after filtering: {len(obj)}" in r.stdout
    assert f"filtered {len(want['filtered'])}" in r.stdout and f"class_ground {len(ground)}" in r.stdout


def test_tool_usage_and_errors(gpu, tmp_path):
    if not EXE.exists():
        subprocess.check_call(["make", "build/ground_segments"], cwd=ROOT)
    assert subprocess.run([str(EXE)], capture_output=True, text=True).returncode == 2
    src = tmp_path / "in.ply"
    write_ply(src, gu.terrain(50, 1), fmt="binary")
    r = subprocess.run([str(EXE), str(src), str(tmp_path / "x"), "0.05", "2", "1", "0.05", "0.5", "0"], capture_output=True, text=True)
    assert r.returncode == 1 and "cell size" in r.stdout
