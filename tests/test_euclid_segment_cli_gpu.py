"""pcc::euclideanClusterSegmentation (include/pcc/comparator_nn.hpp) against the VoxelGrid + SACSegmentation + ExtractIndices +
EuclideanClusterExtraction objects it replaces (tests/cpp/euclid_segment_driver.cpp), and the example CLI's -e path with and without
--euclidean-device, in the manner of tests/test_segment_cli_gpu.py."""
import subprocess
from pathlib import Path

import pytest

from euclid_segment_util import _room
from ply_util import write_ply

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "build" / "comparator"
DRIVER = ROOT / "build" / "euclid_segment_driver"


def _driver(*args):
    if not DRIVER.exists():
        subprocess.check_call(["make", "build/euclid_segment_driver"], cwd=ROOT)
    r = subprocess.run([str(DRIVER), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "euclid segment driver ok" in r.stdout and "DIFFERENT" not in r.stdout
    assert r.stdout.count(": equal") == 8 and "empty cloud: empty" in r.stdout
    assert r.stdout.count("2 planes, 759 remain, 3 clusters: equal") >= 4 and r.stdout.count("0 planes,") == 2
    return r.stdout


def test_cpp_euclidean_cluster_segmentation_equals_the_objects(gpu):
    _driver()


def test_cpp_mirror_repeats_after_both_overflows(gpu):
    """room for one plane and one cluster at first: the call overflows on the planes, then on the clusters, then fits"""
    _driver("1", "1")


def _four_boxes(seed, side):
    """a floor, a wall and four boxes of 216 points: two planes, then four clusters"""
    return _room(seed, side, [(6, 6, 6, (0.15, 0.15, 0.3)), (6, 6, 6, (0.75, 0.15, 0.45)), (6, 6, 6, (0.15, 0.75, 0.6)),
                              (6, 6, 6, (0.75, 0.75, 0.3))])


def test_cli_euclidean_device_prints_and_writes_the_same(gpu, tmp_path):
    if not EXE.exists():
        subprocess.check_call(["make", "cli"], cwd=ROOT)
    fa, fb = tmp_path / "a.ply", tmp_path / "b.ply"
    write_ply(fa, _four_boxes(1, 36), fmt="binary")
    write_ply(fb, _four_boxes(2, 34), fmt="binary")
    runs = []
    for flags in (["-e"], ["-e", "--euclidean-device"]):
        res = tmp_path / f"results{len(runs)}.txt"
        prefix = tmp_path / f"cl{len(runs)}"
        r = subprocess.run([str(EXE), *flags, str(fa), str(fb), "--results", str(res), "--dump-clusters", str(prefix)], capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 1, r.stdout + r.stderr  # the reference always returns 1 (src/comparator.cpp:1704)
        dumps = {p.name[len(prefix.name):]: p.read_bytes() for p in sorted(tmp_path.glob(prefix.name + "_*.ply"))}
        runs.append((r.stdout, res.read_text(), dumps))
    assert runs[0][0] == runs[1][0]
    assert runs[0][1] == runs[1][1] and runs[0][1]
    assert runs[0][2] == runs[1][2] and len(runs[0][2]) == 8  # four boxes per scene, byte for byte
    out = runs[1][0]
    assert "Euclidean cluster segmentation was selected" in out
    assert "PointCloud after filtering has: 3456 data points." in out and "PointCloud after filtering has: 3176 data points." in out
    assert out.count("PointCloud representing the Cluster: 216 data points.") == 8
    assert out.count("PointCloud representing the planar component:") >= 4


def test_cli_usage_names_the_flag(gpu):
    if not EXE.exists():
        subprocess.check_call(["make", "cli"], cwd=ROOT)
    r = subprocess.run([str(EXE), "-h"], capture_output=True, text=True)
    assert "--euclidean-device" in r.stdout and "pcc_euclidean_cluster_segmentation" in r.stdout
    # directly after --segment-device's lines
    tail = r.stdout[r.stdout.index("--segment-device"):]
    flags = [line.split()[0] for line in tail.splitlines() if line.startswith("--")]
    assert flags[:3] == ["--segment-device", "--euclidean-device", "--results"]
