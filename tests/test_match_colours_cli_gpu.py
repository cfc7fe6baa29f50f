"""The example CLI with and without --colours-device: the colour-element counts of all accepted matches through one
pcc_match_colour_elements call (report::clusterSections' colours_device, pcc::matchColourElements) write the same report, byte
for byte, alone and together with --matching-device; on a scene pair whose descriptors make two clusters of scene 1 accept the
SAME cluster of scene 2, so that the call's deduplication is on the path.  After tests/test_cluster_matching_cli_gpu.py."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _painted(pts, seed):
    """one colour per 0.6 x 0.6 tile of the ground plan, +-2 levels of noise: every box is one colour element"""
    rng = np.random.default_rng(seed)
    base = np.array([[180, 170, 150], [90, 60, 40], [40, 90, 160], [200, 40, 40]], np.int32)
    which = (np.floor(pts[:, 0] / 0.9).astype(int) + 2 * np.floor(pts[:, 1] / 0.9).astype(int)) % 4
    return np.clip(base[which] + rng.integers(-2, 3, (len(pts), 3)), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def scene(gpu, tmp_path_factory):
    import test_cli_gpu as cli
    from ply_util import write_ply
    tmp = tmp_path_factory.mktemp("match_colours_cli")
    if not cli.EXE.exists():
        subprocess.check_call(["make", "cli"], cwd=ROOT)
    a, b = cli._scene(1), cli._scene(2, shift=(0.004, -0.003, 0.002))
    fa, fb = tmp / "a.ply", tmp / "b.ply"
    write_ply(fa, a, _painted(a, 3), fmt="binary")
    write_ply(fb, b, _painted(b, 4), fmt="binary")
    r = subprocess.run([str(cli.EXE), "-e", str(fa), str(fb), "--results", str(tmp / "r0.txt"), "--dump-clusters", str(tmp / "cl")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1
    cen = [[cli._centroid_f32(cli._read_cluster_ply(tmp / f"cl_{k}_{j}.ply")) for j in range(4)] for k in (1, 2)]
    order = [np.argsort([np.linalg.norm(cen[0][i] - c2) for c2 in cen[1]], kind="stable") for i in range(4)]
    twin = [int(o[0]) for o in order]
    assert sorted(twin) == [0, 1, 2, 3]
    # a second cluster of scene 1 that has cluster 0's twin among its three nearest
    second = next(i for i in range(1, 4) if twin[0] in [int(j) for j in order[i][:3]])
    others = [i for i in range(1, 4) if i != second]
    rng = np.random.default_rng(13)
    mk = lambda n: rng.random((n, 32)).astype(np.float32)
    des1, des2 = {}, {}
    des1[0] = mk(10); des2[twin[0]] = des1[0].copy()        # accepted: its twin
    des1[second] = des1[0].copy(); des2[twin[second]] = mk(3)  # its own twin holds 3 descriptors and is never tried: cluster 0's twin again
    des1[others[0]] = mk(10); des2[twin[others[0]]] = des1[others[0]].copy()  # accepted: its twin
    des1[others[1]] = mk(3); des2[twin[others[1]]] = mk(3)  # never tried
    cli._write_descriptors(tmp / "d1.txt", des1)
    cli._write_descriptors(tmp / "d2.txt", des2)

    def run(tag, *flags):
        res = tmp / f"{tag}.txt"
        rr = subprocess.run([str(cli.EXE), "-e", str(fa), str(fb), "--results", str(res), "--descriptors1", str(tmp / "d1.txt"),
                             "--descriptors2", str(tmp / "d2.txt"), *flags], capture_output=True, text=True, timeout=300)
        assert rr.returncode == 1, rr.stdout + rr.stderr
        return rr.stdout.replace(str(res), "RESULTS"), res.read_bytes()

    return run, twin, second, others


@pytest.mark.parametrize("flags", [(), ("--matching-device",)], ids=["alone", "with --matching-device"])
def test_cli_colours_device_writes_the_same_report(scene, flags):
    run, twin, second, others = scene
    host = run("host", *flags)
    device = run("device", "--colours-device", *flags)
    assert device[1] == host[1] and host[1]                                  # the report, byte for byte
    assert device[0] == host[0]                                              # ... and what is printed
    txt = device[1].decode()
    # three accepted matches, two of which name the same cluster of scene 2
    assert f"\tMatched cluster 0 of PCL 1 with cluster {twin[0]} of PCL 2:\n" in txt
    assert f"\tMatched cluster {second} of PCL 1 with cluster {twin[0]} of PCL 2:\n" in txt
    assert f"\tMatched cluster {others[0]} of PCL 1 with cluster {twin[others[0]]} of PCL 2:\n" in txt
    assert f"\t\tCluster {others[1]} of PCL 1 has no match in PCL 2\n" in txt
    assert "Total number of matches found: 3\n" in txt
    assert txt.count("color differences") == 3


def test_cli_colours_device_agrees_with_the_batch_flag(scene):
    run = scene[0]
    assert run("device", "--colours-device")[1] == run("batch", "--rgb-batch")[1]


def test_cli_usage_names_the_flag(gpu):
    exe = ROOT / "build" / "comparator"
    if not exe.exists():
        subprocess.check_call(["make", "cli"], cwd=ROOT)
    r = subprocess.run([str(exe), "-h"], capture_output=True, text=True)
    assert "--colours-device" in r.stdout and "pcc_match_colour_elements" in r.stdout
