"""pcc::regionGrowingSegmentation (include/pcc/comparator_nn.hpp) against the VoxelGrid + NormalEstimation + RegionGrowing objects
it replaces (tests/cpp/segment_driver.cpp), and the example CLI's default path with and without --segment-device, in the manner of
tests/test_cli_gpu.py."""
import subprocess
from pathlib import Path

import pytest

from ply_util import write_ply
from test_cli_gpu import _scene, _walls

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "build" / "comparator"


def test_cpp_region_growing_segmentation_equals_the_objects(gpu):
    exe = ROOT / "build" / "segment_driver"
    if not exe.exists():
        subprocess.check_call(["make", "build/segment_driver"], cwd=ROOT)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "segment driver ok" in r.stdout and "DIFFERENT" not in r.stdout
    assert r.stdout.count("3 clusters: equal") == 6 and "empty cloud: empty" in r.stdout and "k = 0: refused" in r.stdout


def test_cli_segment_device_prints_and_writes_the_same(gpu, tmp_path):
    if not EXE.exists():
        subprocess.check_call(["make", "cli"], cwd=ROOT)
    fa, fb = tmp_path / "a.ply", tmp_path / "b.ply"
    write_ply(fa, _walls(27, 3), fmt="binary")
    write_ply(fb, _walls(24, 4), fmt="binary")
    runs = []
    for flags in ([], ["--segment-device"]):
        res = tmp_path / f"results{len(runs)}.txt"
        prefix = tmp_path / f"cl{len(runs)}"
        r = subprocess.run([str(EXE), *flags, str(fa), str(fb), "--results", str(res), "--dump-clusters", str(prefix)], capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 1, r.stdout + r.stderr  # the reference always returns 1 (src/comparator.cpp:1704)
        dumps = {p.name[len(prefix.name):]: p.read_bytes() for p in sorted(tmp_path.glob(prefix.name + "_*.ply"))}
        runs.append((r.stdout, res.read_text(), dumps))
    assert runs[0][0] == runs[1][0]
    assert runs[0][1] == runs[1][1] and runs[0][1]
    assert runs[0][2] == runs[1][2] and len(runs[0][2]) == 6  # three plates per scene, byte for byte
    out = runs[1][0]
    assert "PointCloud after filtering has: 2187 data points." in out and "PointCloud after filtering has: 1728 data points." in out
    assert out.count("Number of clusters is equal to 3") == 2


def test_cli_usage_names_the_flag_and_e_ignores_it(gpu, tmp_path):
    if not EXE.exists():
        subprocess.check_call(["make", "cli"], cwd=ROOT)
    r = subprocess.run([str(EXE), "-h"], capture_output=True, text=True)
    assert "--segment-device" in r.stdout and "pcc_region_growing_segmentation" in r.stdout
    assert r.stdout.index("--planes-device") < r.stdout.index("--segment-device") < r.stdout.index("--results F")
    fa, fb = tmp_path / "a.ply", tmp_path / "b.ply"
    write_ply(fa, _scene(1), fmt="binary")
    write_ply(fb, _scene(2, shift=(0.004, -0.003, 0.002)), fmt="binary")
    outs = []
    for flags in (["-e"], ["-e", "--segment-device"]):
        r = subprocess.run([str(EXE), *flags, str(fa), str(fb), "--results", str(tmp_path / "r.txt")], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 1, r.stdout + r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1] and "Euclidean cluster segmentation was selected" in outs[0]
