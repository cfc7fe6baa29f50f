"""The example CLI with and without --matching-device: the cluster-matching loop through one pcc_cluster_matching call
(report::clusterSections' matching_device, pcc::matchClusters) prints the same lines and writes the same report, byte for byte,
on three and on 32 bins, alone and together with --rgb-batch; on the scene of tests/test_match_dims_gpu.py's CLI test."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def scene(gpu, tmp_path_factory):
    import test_cli_gpu as cli
    tmp = tmp_path_factory.mktemp("cluster_matching_cli")
    if not cli.EXE.exists():
        subprocess.check_call(["make", "cli"], cwd=ROOT)
    a, b = cli._scene(1), cli._scene(2, shift=(0.004, -0.003, 0.002))
    fa, fb = tmp / "a.ply", tmp / "b.ply"
    cli.write_ply(fa, a, fmt="binary")
    cli.write_ply(fb, b, fmt="binary")
    r = subprocess.run([str(cli.EXE), "-e", str(fa), str(fb), "--results", str(tmp / "r0.txt"), "--dump-clusters", str(tmp / "cl")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1
    cen = [[cli._centroid_f32(cli._read_cluster_ply(tmp / f"cl_{k}_{j}.ply")) for j in range(4)] for k in (1, 2)]
    twin = [int(np.argmin([np.linalg.norm(cen[0][i] - c2) for c2 in cen[1]])) for i in range(4)]
    rng = np.random.default_rng(12)

    def mk(n):
        d = rng.random((n, 32)).astype(np.float32)
        d[:, :3] = np.float32(0.5)
        return d

    des1, des2 = {}, {}
    des1[0] = mk(10); des2[twin[0]] = des1[0].copy()                        # the same in every bin
    des1[1] = mk(10); des2[twin[1]] = mk(10)                                # the same in bins 0 - 2 only
    des1[2] = mk(11); des2[twin[2]] = des1[2][:10].copy()                   # n1 = n2 + 1, all matched: "Match accepted"
    des1[3] = mk(3); des2[twin[3]] = mk(3)                                  # 3 descriptors: never tried
    cli._write_descriptors(tmp / "d1.txt", des1)
    cli._write_descriptors(tmp / "d2.txt", des2)

    def run(tag, *flags):
        res = tmp / f"{tag}.txt"
        rr = subprocess.run([str(cli.EXE), "-e", str(fa), str(fb), "--results", str(res), "--descriptors1", str(tmp / "d1.txt"),
                             "--descriptors2", str(tmp / "d2.txt"), *flags], capture_output=True, text=True, timeout=300)
        assert rr.returncode == 1, rr.stdout + rr.stderr
        return rr.stdout.replace(str(res), "RESULTS"), res.read_bytes()

    return run, twin


@pytest.mark.parametrize("flags", [(), ("--descriptor-dims", "32"), ("--rgb-batch",)], ids=["three bins", "32 bins", "with --rgb-batch"])
def test_cli_matching_device_prints_and_writes_the_same(scene, flags):
    run, twin = scene
    host = run("host", *flags)
    device = run("device", "--matching-device", *flags)
    assert device[0] == host[0]                                              # stdout, byte for byte
    assert device[1] == host[1] and host[1]                                  # the report
    out, txt = device[0], device[1].decode()
    assert f"\tMatched cluster 0 of PCL 1 with cluster {twin[0]} of PCL 2:\n" in txt
    assert "Des pcl 1: 10" in out and "Percentage of RIFT correspondences of clusters 0 and" in out
    assert "Match accepted" in out                                           # (printed where cluster 1's count is the larger)
    assert f"\tMatched cluster 2 of PCL 1 with cluster {twin[2]} of PCL 2:\n" in txt
    assert "\t\tCluster 3 of PCL 1 has no match in PCL 2\n" in txt
    full = "32" in flags
    assert (f"\tMatched cluster 1 of PCL 1 with cluster {twin[1]} of PCL 2:\n" in txt) == (not full)


def test_cli_usage_names_the_flag(gpu):
    exe = ROOT / "build" / "comparator"
    if not exe.exists():
        subprocess.check_call(["make", "cli"], cwd=ROOT)
    r = subprocess.run([str(exe), "-h"], capture_output=True, text=True)
    assert "--matching-device" in r.stdout and "pcc_cluster_matching" in r.stdout
