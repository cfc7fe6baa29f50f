"""pcc_rift_descriptors on the GPU (reference src/comparator.cpp:590-684, processRIFT) against the host mirror of the same
pipeline (build/rift_host: the headers the kernels are compiled from, exhaustive rows, one core): the kept point indices are
equal and every histogram carries the mirror's BITS -- same header, same order of operations, same acosf.  What the mirror
itself is worth is tests/test_rift_cpu.py's subject (NumPy restatement in float64).  Also: both histogram kernel layouts,
host and device memory, packed colours and 32-byte pcl::PointXYZRGB records, numpy and torch; the normal stage against
oracle.normals_radius; pcc::processRIFT through a C++ driver; the CLI's --rift switch."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle
import rift_util
from ply_util import write_ply
from pointcloudcomparator_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "build" / "comparator"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_same(got, want, what=""):
    gh, gi = got
    wh, wi = want
    assert np.array_equal(np.asarray(gi), wi), f"{what}: kept point indices differ"
    assert gh.shape == wh.shape == (len(wi), 32)
    differ = (_bits(gh) != _bits(wh)).any(1)
    assert not differ.any(), f"{what}: {int(differ.sum())} of {len(wi)} histograms differ in their bits, first {int(np.argmax(differ))}"


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    """name -> (hist, index) of build/rift_host, computed once"""
    tmp = tmp_path_factory.mktemp("rift_host")
    cache = {}

    def get(name):
        if name not in cache:
            p, rgb = rift_util.scene(name)
            cache[name] = rift_util.run_tool(rift_util.HOST, p, rgb, tmp, tag=name.replace("-", "_"))[:2]
        return cache[name]
    return get


@pytest.mark.parametrize("layout", [1, 0])
@pytest.mark.parametrize("name", list(rift_util.SMALL) + list(rift_util.BIG))
def test_descriptors_carry_the_host_mirrors_bits(gpu, mirror, name, layout):
    p, rgb = rift_util.scene(name)
    want = mirror(name)
    assert len(want[1]) > 0
    with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
        ix.set_option(capi.OPT_RIFT_LAYOUT, layout)
        got = ix.rift_descriptors(rgb)
        _assert_same(got, want, f"{name}, layout {layout}")
        again = ix.rift_descriptors(synth.pack_rgb(rgb))  # packed words; the handle's buffers reused
        _assert_same(again, want, f"{name}, layout {layout}, second call")
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32
    assert (np.diff(got[1]) > 0).all()  # ascending original indices
    nrm = np.sqrt((got[0].astype(np.float64) ** 2).sum(1))
    assert np.abs(nrm - 1.0).max() < 1e-5  # unit histograms


def test_memory_spaces_strides_and_torch(gpu, mirror):
    import torch
    p, rgb = rift_util.scene("isolated")
    want = mirror("isolated")
    rec = synth.xyzrgb_records(p, rgb)  # pcl::PointXYZRGB: 32-byte stride, colour word at offset 16
    with capi.Index(rec, engine=capi.ENGINE_GRID, device=0) as ix:
        _assert_same(ix.rift_descriptors(rec), want, "numpy records")
        h, i = ix.rift_descriptors(torch.from_numpy(rec))
        assert isinstance(h, np.ndarray) or not h.is_cuda
        _assert_same((np.asarray(h), np.asarray(i)), want, "torch host records")
        h, i = ix.rift_descriptors(torch.from_numpy(rgb))
        _assert_same((np.asarray(h), np.asarray(i)), want, "torch host r, g, b")
    drec = torch.from_numpy(rec).cuda()
    with capi.Index(drec, engine=capi.ENGINE_GRID, device=0) as ix:
        h, i = ix.rift_descriptors(drec)
        assert h.is_cuda and i.is_cuda and h.shape == (len(want[1]), 32)
        torch.cuda.synchronize()
        _assert_same((h.cpu().numpy(), i.cpu().numpy()), want, "device records")
        dw = torch.from_numpy(synth.pack_rgb(rgb).view(np.int32)).cuda()
        h, i = ix.rift_descriptors(dw)
        torch.cuda.synchronize()
        _assert_same((h.cpu().numpy(), i.cpu().numpy()), want, "device packed words")
        h, i = ix.rift_descriptors(torch.from_numpy(rgb).cuda())
        torch.cuda.synchronize()
        _assert_same((h.cpu().numpy(), i.cpu().numpy()), want, "device r, g, b")


def test_other_radii(gpu, tmp_path):
    """gradient radius != normal radius: a CSR of its own for the gradient stage"""
    p, rgb = rift_util.scene("volume300")
    want = rift_util.run_tool(rift_util.HOST, p, rgb, tmp_path, radii=(0.025, 0.035, 0.045))[:2]
    assert len(want[1]) > 250
    with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
        _assert_same(ix.rift_descriptors(rgb, 0.025, 0.035, 0.045), want, "radii 0.025 / 0.035 / 0.045")


def test_refusals_on_a_live_handle(gpu):
    p, rgb = rift_util.scene("volume300")
    with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
        with pytest.raises(Exception, match="only 4 distance x 8 gradient bins"):
            ix.rift_descriptors(rgb, nr_distance_bins=8, nr_gradient_bins=4)
        with pytest.raises(Exception, match="bad radius"):
            ix.rift_descriptors(rgb, rift_radius=0.0)
        h, i = ix.rift_descriptors(rgb)  # and the handle still works
        assert len(i) == 300


def test_normal_stage_against_the_oracle(gpu):
    """the first stage is pcc_normals_radius, unchanged: the oracle's bits on a RIFT scene"""
    p, _ = rift_util.scene("isolated")
    want = oracle.normals_radius(p, 0.03)
    with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
        got = ix.normals_radius(0.03)
    same = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))
    assert same.all()
    assert np.isnan(want[:, 0]).sum() == 30  # the points the first compaction removes


def test_cpp_processRIFT_equals_the_python_result(gpu, mirror, tmp_path):
    for name in ("isolated", "non-finite"):
        p, rgb = rift_util.scene(name)
        h, i, out = rift_util.run_tool(rift_util.DRIVER, p, rgb, tmp_path, tag=name.replace("-", "_"))
        assert f"kept={len(i)}" in out
        with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
            _assert_same(ix.rift_descriptors(rgb), (h, i), f"pcc::processRIFT, {name}")
        _assert_same((h, i), mirror(name), f"pcc::processRIFT vs mirror, {name}")


# ---- the CLI: two PLY files give a verdict ---------------------------------------------------------------------------------
def _cli_scene(seed, boxes=4):
    """A floor (one point per 0.03 lattice site) and `boxes` coloured blocks sampled twice per 0.025 voxel and axis, so that
    the VoxelGrid leaves 7 x 7 x 7 points per block on a 0.025 lattice: 3 cm rows of 4 to 7 points, every normal and every
    gradient defined.  The floor holds more than 70 % of the filtered points: the plane loop of the -e path removes it and
    stops (src/segmentation.cpp:79-117), the blocks become the clusters."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(62), np.arange(62), indexing="ij"), -1).reshape(-1, 2) * 0.03
    floor = np.concatenate([g + 0.01, np.full((len(g), 1), 0.01)], 1)
    k = np.arange(7)[:, None] * 0.025 + np.array([0.004, 0.0165])[None, :]
    c = np.stack(np.meshgrid(k.reshape(-1), k.reshape(-1), k.reshape(-1), indexing="ij"), -1).reshape(-1, 3)
    origins = [(0.3, 0.3, 0.3), (1.2, 0.3, 0.45), (0.3, 1.2, 0.6), (1.2, 1.2, 0.3)][:boxes]
    blocks = [c + np.asarray(o) for o in origins]
    pts = np.concatenate([floor] + blocks)
    pts = pts + rng.uniform(-0.001, 0.001, pts.shape)
    f = 128 + 100 * np.sin(40 * pts[:, 0]) * np.cos(30 * pts[:, 1] + 20 * pts[:, 2])
    rgb = np.clip(np.stack([f, 0.8 * f, 255 - f], 1) + rng.normal(0, 4, (len(pts), 3)), 0, 255).astype(np.uint8)
    order = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[order].astype(np.float32)), np.ascontiguousarray(rgb[order])


def _run(args, timeout=300):
    if not EXE.exists():
        subprocess.check_call(["make", "cli"], cwd=ROOT)
    r = subprocess.run([str(EXE)] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 1, r.stdout[-2000:] + r.stderr[-2000:]  # the reference always returns 1
    return r.stdout


def test_cli_rift_gives_a_verdict(gpu, tmp_path):
    a, ca = _cli_scene(1)
    b, cb = _cli_scene(2, boxes=3)
    fa, fb, res = tmp_path / "a.ply", tmp_path / "b.ply", tmp_path / "results.txt"
    write_ply(fa, a, rgb=ca, fmt="binary")
    write_ply(fb, b, rgb=cb, fmt="binary")
    # without the switch: today's text
    out = _run(["-e", fa, fb, "--results", res])
    assert "No descriptor files were given (--descriptors1/2): clusters were not matched, no verdict" in out
    assert "(no descriptor files given: clusters could not be matched, no verdict)" in res.read_text()
    # with it: descriptors per cluster, a score block and a verdict
    out = _run(["--rift", "-e", fa, fb, "--results", res, "--dump-descriptors", tmp_path / "des"])
    txt = res.read_text()
    assert "no verdict" not in out and "no verdict" not in txt
    counts = [int(x) for x in re.findall(r"Number of descriptors: (\d+)", txt)]
    assert len(counts) == 7 and all(c > 0 for c in counts), counts  # 3 clusters of PCL2, then 4 of PCL 1
    assert "points score pcl1: " in txt and "descriptors score pcl1: " in txt and "Total number of matches found: " in txt
    assert sum(s in out for s in ("The first point cloud has more information", "The second point cloud has more information",
                                  "Both point clouds have the same information")) == 1
    # the dumped descriptors are the ones --descriptors1/2 read back: same report
    res2 = tmp_path / "results2.txt"
    out2 = _run(["-e", fa, fb, "--results", res2, "--descriptors1", tmp_path / "des_1.txt", "--descriptors2", tmp_path / "des_2.txt"])
    strip = lambda t: t.split("\n", 1)[1]  # (the first line names the files)
    assert strip(res2.read_text()) == strip(txt)
    assert [l for l in out2.splitlines() if "information" in l] == [l for l in out.splitlines() if "information" in l]


def test_cli_rift_two_copies_of_one_scene_are_the_same(gpu, tmp_path):
    a, ca = _cli_scene(3)
    fa, fb, res = tmp_path / "a.ply", tmp_path / "b.ply", tmp_path / "results.txt"
    write_ply(fa, a, rgb=ca, fmt="binary")
    write_ply(fb, a, rgb=ca, fmt="binary")
    out = _run(["--rift", "-e", fa, fb, "--results", res])
    txt = res.read_text()
    counts = [int(x) for x in re.findall(r"Number of descriptors: (\d+)", txt)]
    assert len(counts) == 8 and all(c > 0 for c in counts) and counts[:4] == counts[4:]
    assert "Total number of matches found: 4" in txt
    assert "Both point clouds have the same information" in out


def test_cli_help_names_the_switch_and_its_caveat(gpu):
    out = _run(["-h"])
    assert "--rift" in out and "700 points" in out and "--dump-descriptors" in out
