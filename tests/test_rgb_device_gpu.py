"""pcc_region_growing_rgb on the GPU (csrc/region_rgb.hip; reference src/segmentation.cpp:161-216): labels and cluster count
of Index.region_growing_rgb against the oracle's restatement fed the rows of the SAME index -- bit for bit, no tolerance."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle
from pointcloudcomparator_amd import capi

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import rgb_device_util as util  # noqa: E402
from ply_util import write_ply  # noqa: E402
from test_rgb_cpu import big_segment_scene  # noqa: E402
from test_rgb_gpu import _scenes  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes(gpu):
    return {name: (pts, rgb, par) for name, pts, rgb, par in _scenes()}


@pytest.fixture(scope="module")
def rows(gpu, scenes):
    """the K = min(100, n) rows of every scene, from the library, searched once"""
    out = {}
    for name, (pts, rgb, par) in scenes.items():
        with capi.Index(pts) as ix:
            out[name] = ix.knn(pts, min(100, len(pts)))
    return out


def _both(pts, rgb, ki=None, kd=None, **kw):
    """((labels, n) of the library, (labels, n) of the oracle over the same index's rows, stats of the call)"""
    K = min(kw.get("region_nn", 100), len(pts))
    with capi.Index(pts) as ix:
        if ki is None:
            ki, kd = ix.knn(pts, K)
        got = ix.region_growing_rgb(rgb, **kw)
        stats = ix.stats()
    want = oracle.region_growing_rgb(pts, rgb, neighbours=ki, neighbour_d2=kd, **kw)
    return got, want, stats, (ki, kd)


def _same(got, want, what):
    assert got[1] == want[1], (what, got[1], want[1])
    assert got[0].dtype == np.int32 and (got[0] == want[0]).all(), (what, np.nonzero(got[0] != want[0])[0][:10])


@pytest.mark.parametrize("name", ["room", "noise", "patches", "tiny", "near"])
def test_existing_scenes(scenes, rows, name):
    pts, rgb, (dist, p2p, r2r, mn) = scenes[name]
    ki, kd = rows[name]
    got, want, stats, _ = _both(pts, rgb, ki, kd, distance=dist, point_colour=p2p, region_colour=r2r, min_size=mn)
    print(f"{name}: {len(pts)} points, {stats[0]} segments, {stats[1]} pairs, {stats[7]} sweeps, {got[1]} clusters")
    _same(got, want, name)


@pytest.mark.parametrize("name", ["patches", "noise"])
def test_growing_stage_alone(scenes, rows, name):
    """region_colour = 0, min_size = 1: nothing merges, folds or is dropped -- the clusters are the grown segments"""
    pts, rgb, _ = scenes[name]
    ki, kd = rows[name]
    got, want, stats, _ = _both(pts, rgb, ki, kd, region_colour=0.0, min_size=1)
    _same(got, want, name)
    assert stats[0] == want[1]
    assert (got[0] == util.order_free_segments(rgb, ki)[0]).all()


@pytest.fixture(scope="module")
def cascades(gpu):
    """the density cascade of tests/test_rgb_device_cpu.py in both index orders: (points, colours, library result, oracle
    result over the same index's rows, stats, rows)"""
    out = {}
    for name, pts, rgb in util.fixpoint_scenes()[4:]:
        got, want, stats, (ki, kd) = _both(pts, rgb, region_colour=0.0, min_size=1)
        out[name] = (pts, rgb, got, want, stats, ki)
    return out


@pytest.mark.parametrize("name", ["cascade", "cascade_rev"])
def test_one_way_edges(cascades, name):
    """a union-find over undirected edges alone is wrong here (the dense clumps are reached from the sparse ones, never the
    other way round), and the labels need several sweeps to settle"""
    pts, rgb, got, want, stats, ki = cascades[name]
    print(f"{name}: {want[1]} segments, {stats[7]} sweeps")
    _same(got, want, name)
    assert stats[0] == want[1] == util.order_free_segments(rgb, ki)[0].max() + 1
    src, nb = util.valid_edges(rgb, ki)
    back = set(zip(nb.tolist(), src.tolist()))
    assert any((a, b) not in back for a, b in zip(src.tolist(), nb.tolist())), "the scene must hold one-way edges"


def test_one_way_edges_make_the_index_order_matter(cascades):
    """the same points in reversed order: every clump is seeded before a sparser one reaches it"""
    fwd, rev = cascades["cascade"][3][1], cascades["cascade_rev"][3][1]
    assert fwd < rev
    assert cascades["cascade"][4][7] > 1, "the forward order needs more than one sweep"


@pytest.mark.parametrize("kw", [dict(region_nn=3), dict(nn=5, region_nn=100)], ids=["region_nn3", "nn5"])
def test_pair_stage(scenes, kw):
    pts, rgb, (dist, p2p, r2r, mn) = scenes["patches"]
    got, want, stats, got_rows = _both(pts, rgb, distance=dist, point_colour=p2p, region_colour=r2r, min_size=mn, **kw)
    ki = got_rows[0]
    _same(got, want, kw)
    # the oracle's own segments: with nothing merged, folded or dropped its clusters are the grown segments
    seg, nseg = oracle.region_growing_rgb(pts, rgb, neighbours=ki, neighbour_d2=got_rows[1], point_colour=p2p, region_colour=0.0, min_size=1, **kw)
    assert stats[0] == nseg == seg.max() + 1
    assert stats[1] == util.ordered_pair_count(seg, ki)
    assert stats[1] > 0


@pytest.mark.parametrize("n", [1, 2, 11])
def test_tiny_clouds(gpu, n):
    rng = np.random.default_rng(11)
    pts = rng.random((n, 3)).astype(np.float32)
    rgb = np.full((n, 3), 90, np.uint8) if n == 2 else (rng.integers(0, 2, (n, 3)) * 50).astype(np.uint8)
    got, want, stats, _ = _both(pts, rgb, min_size=1)
    _same(got, want, n)
    assert got[1] >= 1


def test_non_finite_points_take_part_in_nothing(scenes):
    pts, rgb, (dist, p2p, r2r, mn) = scenes["patches"]
    pts = pts.copy()
    bad = [5, 1777, len(pts) - 1]
    pts[bad[0], 0] = np.nan
    pts[bad[1], 2] = np.inf
    pts[bad[2]] = np.nan
    keep = np.isfinite(pts).all(1)
    got, want, stats, _ = _both(pts[keep], rgb[keep], distance=dist, point_colour=p2p, region_colour=r2r, min_size=mn)
    _same(got, want, "stripped")
    with capi.Index(pts) as ix:
        labels, ncl = ix.region_growing_rgb(rgb, distance=dist, point_colour=p2p, region_colour=r2r, min_size=mn)
    expect = np.full(len(pts), -1, np.int32)
    expect[keep] = want[0]
    assert ncl == want[1] and (labels == expect).all()
    assert (labels[bad] == -1).all()


def test_integer_colour_sums_and_kept_rows(gpu):
    """a segment whose channel sums pass 2^24 (exact integer sums: 2 clusters, a float sum merges them); then the kept rows
    of PCC_OPT_KNN_CACHE_K serve the call: the same labels"""
    pts, rgb = big_segment_scene()
    with capi.Index(pts) as ix:
        ki, kd = ix.knn(pts, 100)
        host = ix.region_growing_rgb(rgb, min_size=50)
        ix.set_option(capi.OPT_KNN_CACHE_K, 100)
        cached = ix.region_growing_rgb(rgb, min_size=50)
        again = ix.region_growing_rgb(rgb, min_size=50)   # (the second call finds the rows kept)
    want = oracle.region_growing_rgb(pts, rgb, neighbours=ki, neighbour_d2=kd, min_size=50)
    assert want[1] == 2
    for what, got in (("host", host), ("cached", cached), ("again", again)):
        _same(got, want, what)


def test_labels_in_device_memory(scenes, rows):
    import torch
    pts, rgb, (dist, p2p, r2r, mn) = scenes["patches"]
    kw = dict(distance=dist, point_colour=p2p, region_colour=r2r, min_size=mn)
    with capi.Index(pts) as ix:
        host = ix.region_growing_rgb(rgb, **kw)
        labels, ncl = ix.region_growing_rgb(rgb, device=torch.device("cuda", 0), **kw)
        assert labels.is_cuda and labels.dtype == torch.int32
        # colours already on the device, as packed words: nothing is staged
        words = torch.from_numpy((rgb[:, 2].astype(np.int32) | (rgb[:, 1].astype(np.int32) << 8) | (rgb[:, 0].astype(np.int32) << 16))).cuda()
        labels2, ncl2 = ix.region_growing_rgb(words, **kw)
        assert labels2.is_cuda
    want = oracle.region_growing_rgb(pts, rgb, neighbours=rows["patches"][0], neighbour_d2=rows["patches"][1], **kw)
    _same(host, want, "host")
    _same((labels.cpu().numpy(), ncl), want, "device")
    _same((labels2.cpu().numpy(), ncl2), want, "device words")


def _tool(tool, ply, *args):
    exe = ROOT / "build" / tool
    assert exe.exists(), "make cli"
    out = subprocess.run([str(exe), str(ply)] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


@pytest.mark.parametrize("name", ["room", "patches"])
def test_mirror_with_device_segmentation_prints_what_the_host_path_prints(scenes, tmp_path, name):
    pts, rgb, par = scenes[name]
    ply = tmp_path / "c.ply"
    write_ply(ply, pts, rgb)
    host = _tool("rgb_segments", ply, *par)
    dev = _tool("rgb_segments_device", ply, *par)
    assert host.split("\n")[0].split()[1] == str(len(pts))
    assert dev == host


def test_cli_rgb_device_writes_the_same_report(gpu, tmp_path):
    """examples/comparator_main.cpp --rgb-device: the two colour segmentations of every accepted match through
    pcc_region_growing_rgb; results file and console output are those of the run without the flag, byte for byte"""
    import test_cli_gpu as cli
    a, b = cli._scene(1), cli._scene(2, shift=(0.004, -0.003, 0.002))
    fa, fb = tmp_path / "a.ply", tmp_path / "b.ply"
    write_ply(fa, a, fmt="binary")
    write_ply(fb, b, fmt="binary")
    exe = ROOT / "build" / "comparator"
    assert exe.exists(), "make cli"
    r = subprocess.run([str(exe), "-e", str(fa), str(fb), "--results", str(tmp_path / "r0.txt"), "--dump-clusters", str(tmp_path / "cl")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1
    cen = [[cli._centroid_f32(cli._read_cluster_ply(tmp_path / f"cl_{k}_{j}.ply")) for j in range(4)] for k in (1, 2)]
    twin = [int(np.argmin([np.linalg.norm(cen[0][i] - c2) for c2 in cen[1]])) for i in range(4)]
    rng = np.random.default_rng(9)
    des = [rng.random((10, 32)).astype(np.float32) for _ in range(4)]
    cli._write_descriptors(tmp_path / "d1.txt", {i: des[i] for i in range(4)})
    cli._write_descriptors(tmp_path / "d2.txt", {twin[i]: des[i].copy() for i in range(4)})
    runs = []
    for tag, extra in (("host", []), ("device", ["--rgb-device"])):
        res = tmp_path / f"{tag}.txt"
        r = subprocess.run([str(exe), "-e", str(fa), str(fb), "--results", str(res), "--descriptors1", str(tmp_path / "d1.txt"),
                            "--descriptors2", str(tmp_path / "d2.txt")] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 1, r.stderr[-1000:]
        runs.append((res.read_bytes(), r.stdout.replace(str(res), "RESULTS")))
    assert runs[0][0].count(b"color differences") >= 2, "the report must hold matches, or the flag is not exercised"
    assert runs[1][0] == runs[0][0]
    assert runs[1][1] == runs[0][1]
