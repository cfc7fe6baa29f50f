"""pcc_change_detection on the GPU (the reference's spatial_change_detection, src/comparator.cpp:54-110) against the NumPy
restatement of its contract (tests/change_ref.py).  Every comparison is exact: index arrays with np.array_equal, records byte
for byte."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from pointcloudcomparator_amd import capi, synth
import change_ref as cr
from ply_util import write_ply

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
DRIVER, TOOL, CLI = ROOT / "build" / "change_driver", ROOT / "build" / "spatial_change", ROOT / "build" / "comparator"
NAN, INF = np.float32("nan"), np.float32("inf")


@pytest.fixture(scope="module")
def ctx(gpu):
    with capi.Index(np.zeros((1, 3), np.float32)) as ix:
        yield ix


def on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def to_numpy(a):
    return a.cpu().numpy() if capi._is_torch(a) else np.asarray(a)


def check(ctx, a, b, res, min_points=0):
    got = to_numpy(ctx.change_detection(a, b, res, min_points))
    want = cr.change_detection(to_numpy(a), to_numpy(b), res, min_points)
    assert got.dtype == np.int32 and got.shape == want.shape, (res, min_points, got.shape, want.shape)
    assert np.array_equal(got, want), (res, min_points, np.flatnonzero(got != want)[:5])
    assert (np.diff(got) > 0).all()
    return got


@pytest.fixture(scope="module")
def room():
    """A: 3 000 random points in a 2 m cube; B: half of A jittered by 1 cm, then 500 fresh points"""
    rng = np.random.default_rng(0xC4A6E)
    a = (rng.random((3000, 3)) * 2.0).astype(np.float32)
    moved = a[rng.permutation(3000)[:1500]] + ((rng.random((1500, 3)) - 0.5) * 0.02).astype(np.float32)
    b = np.concatenate([moved, (rng.random((500, 3)) * 2.0).astype(np.float32)])
    return a, np.ascontiguousarray(b)


@pytest.mark.parametrize("res", [0.25, 0.1, 0.03])
def test_indices_equal_the_restatement(ctx, room, res):
    a, b = room
    anc = cr.anchor(a, b, res)
    voxels = len(set(map(tuple, cr.voxels(a, anc, res)[1].tolist())))
    assert {0.25: 20, 0.1: 1000, 0.03: 2900}[res] <= voxels <= {0.25: 1000, 0.1: 3000, 0.03: 3000}[res]  # tens to thousands of voxels
    sizes = []
    for min_points in (0, 1, 3):
        got = check(ctx, a, b, res, min_points)
        again = ctx.change_detection(a, b, res, min_points)  # a second identical call
        assert again.dtype == np.int32 and np.array_equal(again, got)
        sizes.append(len(got))
    assert sizes[0] == sizes[1] >= sizes[2] and sizes[0] > 0
    if res == 0.03:
        assert sizes[2] < sizes[1]  # (fine voxels rarely hold three points: the threshold bites)


def test_voxel_faces_and_negative_keys(ctx):
    """resolution 0.25, A's first point (1, 1, 1): the anchor is 0.75 + 2^-24 per axis, and a + k * 0.25 is a float for k = -7 ... 0"""
    res, e = 0.25, cr.EPS / 2
    face = np.array([0.75 + 0.25 * k + e for k in range(-7, 1)])
    assert (face.astype(np.float32).astype(np.float64) == face).all()
    face = face.astype(np.float32)
    below = np.nextafter(face, np.float32(-2))
    rng = np.random.default_rng(5)
    both = np.concatenate([face, below])
    a = np.concatenate([np.ones((1, 3), np.float32), both[rng.integers(0, 16, (40, 3))]])
    b = both[rng.integers(0, 16, (400, 3))]
    anc = cr.anchor(a, b, res)
    assert anc.tolist() == [0.75 + e] * 3
    kf = cr.voxels(np.stack([face] * 3, 1), anc, res)[1][:, 0]
    kb = cr.voxels(np.stack([below] * 3, 1), anc, res)[1][:, 0]
    assert kf.tolist() == list(range(-7, 1)) and kb.tolist() == list(range(-8, 0))  # on a face: the upper voxel; one step below: the lower
    assert (cr.voxels(b, anc, res)[1] < 0).mean() > 0.8  # most keys are negative
    got = check(ctx, a, b, res)
    assert 0 < len(got) < len(b)
    check(ctx, a, b, res, 2)
    check(ctx, on_device(a), on_device(b), res)


def test_non_finite_points(ctx, room):
    a, b = (x.copy() for x in room)
    rng = np.random.default_rng(9)
    for cloud in (a, b):
        rows = rng.permutation(len(cloud))[:90]
        cloud[rows[:30], 0] = NAN
        cloud[rows[30:60], 1] = INF
        cloud[rows[60:], 2] = -INF
    got = check(ctx, a, b, 0.1)
    assert cr.finite_rows(b)[got].all()
    # A's first records are non-finite: the anchor is its first finite one
    a2 = a.copy()
    a2[0], a2[1, 2], a2[2, 0] = NAN, INF, -INF
    assert cr.anchor(a2, b, 0.1).tolist() != cr.anchor(a, b, 0.1).tolist()
    check(ctx, a2, b, 0.1)
    # A without a finite point: every finite point of B is reported, the anchor is B's
    none = np.full((7, 3), NAN, np.float32)
    none[3] = INF
    got = check(ctx, none, b, 0.1)
    assert np.array_equal(got, np.flatnonzero(cr.finite_rows(b)))
    b2 = b.copy()
    b2[0] = NAN
    assert np.array_equal(check(ctx, none, b2, 0.1), np.flatnonzero(cr.finite_rows(b2)))
    # B without a finite point: nothing; neither has one: nothing
    assert len(check(ctx, a, none, 0.1)) == 0 and len(check(ctx, none, none, 0.1)) == 0
    assert len(check(ctx, on_device(none), on_device(none), 0.1)) == 0


def test_identical_disjoint_and_permuted_clouds(ctx, room):
    a, b = room
    for res in (0.25, 0.03):
        assert len(check(ctx, a, a, res)) == 0
    far = b + np.float32(100.0)
    far[5] = NAN
    assert np.array_equal(check(ctx, a, far, 0.1), np.flatnonzero(cr.finite_rows(far)))
    # permuting A behind its first point changes nothing
    want = check(ctx, a, b, 0.1)
    perm = np.concatenate([[0], 1 + np.random.default_rng(3).permutation(len(a) - 1)])
    assert np.array_equal(check(ctx, np.ascontiguousarray(a[perm]), b, 0.1), want)
    # ... replacing its first point shifts the lattice: resolution 1, the faces are at k + eps/2 behind (0, 0, 0) and at
    # k + 0.5 + eps/2 behind (0.5, 0, 0), so (0.3, 0, 0) and (0.9, 0, 0) share a voxel in the first lattice only
    b1 = np.array([[0.9, 0, 0]], np.float32)
    a1 = np.array([[0, 0, 0], [0.3, 0, 0]], np.float32)
    a2 = np.array([[0.5, 0, 0], [0.3, 0, 0]], np.float32)
    assert check(ctx, a1, b1, 1.0).tolist() == [] and check(ctx, a2, b1, 1.0).tolist() == [0]


def test_table_stress(ctx):
    # 20 000 distinct voxels, their keys multiples of 1024 along x (2 000 of them) times ten along y
    i, j = np.meshgrid(np.arange(2000), np.arange(10), indexing="ij")
    b = np.stack([1024.0 * i.ravel() + 0.5, j.ravel() + 0.5, np.full(i.size, 0.5)], 1).astype(np.float32)
    a = np.ascontiguousarray(b[::2][::-1])
    anc = cr.anchor(a, b, 1.0)
    kb = cr.voxels(b, anc, 1.0)[1]
    assert len(set(map(tuple, kb.tolist()))) == 20000 and ((kb[:, 0] - kb[:, 0].min()) % 1024 == 0).all()
    assert len(check(ctx, a, b, 1.0)) == 10000
    check(ctx, on_device(a), on_device(b), 1.0, 1)
    # 20 000 points of B in one voxel: the counter
    rng = np.random.default_rng(2)
    heap = (5.0 + rng.random((20000, 3)) * 0.2).astype(np.float32)
    a = np.zeros((3, 3), np.float32)
    assert len(set(map(tuple, cr.voxels(heap, cr.anchor(a, heap, 1.0), 1.0)[1].tolist()))) == 1
    assert len(check(ctx, a, heap, 1.0, 20000)) == 20000 and len(check(ctx, a, heap, 1.0, 20001)) == 0
    mixed = np.concatenate([heap[:5000], heap[:70] + np.float32(3.0), heap[5000:]])
    assert len(check(ctx, a, mixed, 1.0, 71)) == 20000 and len(check(ctx, a, mixed, 1.0, 70)) == 20070


def test_one_handle_small_large_small(gpu):
    rng = np.random.default_rng(7)
    with capi.Index(np.zeros((1, 3), np.float32)) as ix:
        for n in (200, 40000, 200):
            a = (rng.random((n, 3)) * 2.0).astype(np.float32)
            b = np.concatenate([a[: n // 2] + np.float32(0.004), (rng.random((n // 2, 3)) * 2.0).astype(np.float32)])
            got = check(ix, a, b, 0.05)
            assert 0 < len(got) < n
            check(ix, a, b, 0.05, 2)


def test_layouts_memory_spaces_and_records(ctx, room):
    import torch
    a, b = room
    rng = np.random.default_rng(11)
    ca, cb = (rng.integers(0, 256, (len(x), 3)).astype(np.uint8) for x in (a, b))
    a4, b4 = (np.concatenate([x, np.ones((len(x), 1), np.float32)], 1) for x in (a, b))
    layouts_a = {12: a, 16: a4, 32: synth.xyzrgb_records(a, ca)}
    layouts_b = {12: b, 16: b4, 32: synth.xyzrgb_records(b, cb)}
    layouts_b[32][:, 5:] = rng.random((len(b), 3)).astype(np.float32)  # (padding travels too)
    want = cr.change_detection(a, b, 0.1)
    assert 0 < len(want) < len(b)
    for sa, sb in ((12, 12), (12, 32), (32, 16), (16, 12), (32, 32), (16, 32)):
        ra, rb = layouts_a[sa], layouts_b[sb]
        for wrap in (lambda x: x, torch.from_numpy, on_device):
            idx, rec = ctx.change_detection(wrap(ra), wrap(rb), 0.1, with_records=True)
            assert capi._is_torch(idx) == capi._is_torch(rec) == (wrap is on_device) and (not capi._is_torch(idx) or idx.is_cuda)
            idx, rec = to_numpy(idx), to_numpy(rec)
            assert idx.dtype == np.int32 and np.array_equal(idx, want), (sa, sb)
            assert rec.dtype == np.float32 and rec.shape == (len(want), sb // 4)
            assert np.array_equal(rec.view(np.uint32), rb[want].view(np.uint32)), (sa, sb)  # byte for byte, colour word included
            assert np.array_equal(to_numpy(ctx.change_detection(wrap(ra), wrap(rb), 0.1)), want)
    # a strided view of wider records as A and as B (no records asked for: the rows need not be back to back)
    assert np.array_equal(ctx.change_detection(layouts_a[32][:, :3], layouts_b[32][:, :4], 0.1), want)
    # one cloud on the device, the other on the host: moved beside it
    assert np.array_equal(to_numpy(ctx.change_detection(on_device(a), b, 0.1)), want)
    assert np.array_equal(to_numpy(ctx.change_detection(a, on_device(b), 0.1)), want)


def test_refusals_on_a_live_handle(ctx, room):
    a, b = room

    def raw(a_, b_, res):
        idx = np.full(len(b_), 7, np.int32)
        rec = np.full(b_.shape, 7.0, np.float32)
        n = C.c_size_t(7)
        st = capi.LIB.pcc_change_detection(ctx._h, a_.ctypes.data, len(a_), 12, b_.ctypes.data, len(b_), 12, 0, res, 0, idx.ctypes.data,
                                           rec.ctypes.data, C.byref(n))
        return st, n.value, (idx == 7).all() and (rec == 7).all(), capi.LIB.pcc_last_error().decode()

    # coordinates 10^9 apart at a resolution of 0.01: a voxel coordinate beyond 2^31
    far = b.copy()
    far[17, 1] = 1e9
    st, n, untouched, msg = raw(a, far, 0.01)
    assert st == -5 and n == 0 and untouched and "along y" in msg and "2^31" in msg and "span" in msg, msg
    with pytest.raises(capi.PccError) as e:
        ctx.change_detection(on_device(far), on_device(b), 0.01)
    assert e.value.status == -5
    # within 2^31 but more than 2^21 voxels along an axis: the message holds the span
    wide = a.copy()
    wide[-1, 2] = 30000.0
    st, n, untouched, msg = raw(wide, b, 0.01)
    assert st == -5 and n == 0 and untouched and "along z" in msg, msg
    span = int(re.search(r"span (\d+) voxels", msg).group(1))
    k = np.concatenate([cr.voxels(wide, cr.anchor(wide, b, 0.01), 0.01)[1], cr.voxels(b, cr.anchor(wide, b, 0.01), 0.01)[1]])[:, 2]
    assert span == k.max() - k.min() + 1 > 2 ** 21
    # just inside: 2^21 voxels along x pass
    edge_a = np.array([[0, 0, 0]], np.float32)
    edge_b = np.array([[2 ** 21 - 1.5, 0, 0], [2 ** 21 - 0.5, 0, 0], [-0.5, 0, 0]], np.float32)
    kx = cr.voxels(edge_b, cr.anchor(edge_a, edge_b, 1.0), 1.0)[1][:, 0]
    assert kx.tolist() == [2 ** 21 - 1, 2 ** 21, 0]
    assert check(ctx, edge_a, edge_b[[0, 2]], 1.0).tolist() == [0]  # span 2^21
    st, n, untouched, msg = raw(edge_a, edge_b, 1.0)                # span 2^21 + 1
    assert st == -5 and untouched and "span 2097153 voxels along x" in msg, msg
    # the handle works afterwards
    st, n, untouched, msg = raw(a, b, 0.1)
    assert st == 0 and n == len(cr.change_detection(a, b, 0.1)) and not untouched
    check(ctx, a, b, 0.1)


def _records_file(path, pts, rgb):
    synth.xyzrgb_records(pts, rgb).tofile(path)


def test_cpp_class_gives_the_python_result(ctx, room, tmp_path):
    if not DRIVER.exists():
        subprocess.check_call(["make", "build/change_driver"], cwd=ROOT)
    rng = np.random.default_rng(13)
    a, b = (x.copy() for x in room)
    b[3], a[0] = NAN, INF
    small_a = np.array([[0, 0, 0], [0.3, 0, 0]], np.float32)
    small_b = np.array([[0.9, 0, 0], [4.2, 4.2, 4.2], [4.6, 4.6, 4.6], [-3, 1, 1]], np.float32)  # -> [1, 2] with two points a leaf
    for tag, (pa, pb, res, min_points) in {"room": (a, b, 0.1, 0), "room3": (a, b, 0.25, 3), "small": (small_a, small_b, 1.0, 2)}.items():
        fa, fb = tmp_path / f"{tag}_a.bin", tmp_path / f"{tag}_b.bin"
        _records_file(fa, pa, rng.integers(0, 256, (len(pa), 3)).astype(np.uint8))
        _records_file(fb, pb, rng.integers(0, 256, (len(pb), 3)).astype(np.uint8))
        r = subprocess.run([str(DRIVER), str(fa), str(fb), repr(res), str(min_points)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = r.stdout.splitlines()
        got = np.array(lines[0].split()[1:], np.int32)
        assert lines[0].startswith("indices") and np.array_equal(got, check(ctx, pa, pb, float(np.float32(res)), min_points))
        assert lines[1] == "free function: same" and lines[2] == f"no previous buffer: {int(cr.finite_rows(pb).sum())}"


def _read_xyzrgb(path):
    raw = Path(path).read_bytes()
    head, body = raw.split(b"end_header\n", 1)
    n = int(re.search(rb"element vertex (\d+)", head).group(1))
    rec = np.frombuffer(body, np.dtype([("p", "<f4", 3), ("c", "u1", 3)]))
    assert len(rec) == n
    return rec["p"], rec["c"]


def test_tool_writes_the_records_the_restatement_selects(gpu, room, tmp_path):
    if not TOOL.exists():
        subprocess.check_call(["make", "build/spatial_change"], cwd=ROOT)
    a, b = room
    rng = np.random.default_rng(17)
    ca, cb = (rng.integers(0, 256, (len(x), 3)).astype(np.uint8) for x in (a, b))
    fa, fb, out = tmp_path / "a.ply", tmp_path / "b.ply", tmp_path / "diff.ply"
    write_ply(fa, a, rgb=ca, fmt="binary")
    write_ply(fb, b, rgb=cb, fmt="binary")
    r = subprocess.run([str(TOOL), str(fa), str(fb), "0.1", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    want = cr.change_detection(a, b, 0.1)
    p, c = _read_xyzrgb(out)
    assert f"Points of B in voxels A leaves empty: {len(want)}" in r.stdout and 0 < len(want) < len(b)
    assert np.array_equal(p.view(np.uint32), b[want].view(np.uint32)) and np.array_equal(c, cb[want])
    assert subprocess.run([str(TOOL)], capture_output=True, text=True).returncode == 2
    r = subprocess.run([str(TOOL), str(fa), str(fb), "0", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "resolution" in r.stdout


# ---- the CLI: --changes after the verdict ----------------------------------------------------------------------------------
def _cli_scene(seed, boxes=4):
    """The scene of tests/test_rift_gpu.py: a floor (one point per 0.03 lattice site) and `boxes` coloured blocks of 14^3 points;
    the plane loop of the -e path removes the floor, the blocks become the clusters."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(62), np.arange(62), indexing="ij"), -1).reshape(-1, 2) * 0.03
    floor = np.concatenate([g + 0.01, np.full((len(g), 1), 0.01)], 1)
    k = np.arange(7)[:, None] * 0.025 + np.array([0.004, 0.0165])[None, :]
    c = np.stack(np.meshgrid(k.reshape(-1), k.reshape(-1), k.reshape(-1), indexing="ij"), -1).reshape(-1, 3)
    origins = [(0.3, 0.3, 0.3), (1.2, 0.3, 0.45), (0.3, 1.2, 0.6), (1.2, 1.2, 0.3)][:boxes]
    pts = np.concatenate([floor] + [c + np.asarray(o) for o in origins])
    pts = pts + rng.uniform(-0.001, 0.001, pts.shape)
    f = 128 + 100 * np.sin(40 * pts[:, 0]) * np.cos(30 * pts[:, 1] + 20 * pts[:, 2])
    rgb = np.clip(np.stack([f, 0.8 * f, 255 - f], 1) + rng.normal(0, 4, (len(pts), 3)), 0, 255).astype(np.uint8)
    order = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[order].astype(np.float32)), np.ascontiguousarray(rgb[order])


def _run(args, timeout=300):
    if not CLI.exists():
        subprocess.check_call(["make", "cli"], cwd=ROOT)
    r = subprocess.run([str(CLI)] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 1, r.stdout[-2000:] + r.stderr[-2000:]  # the reference always returns 1
    return r.stdout


FIRST = "The first point cloud has more information"
SECOND = "The second point cloud has more information"
SAME = "Both point clouds have the same information"
IN_FIRST = "Points that are in the first pcl, that are not in the other:"
IN_SECOND = "Points that are in the second pcl, that are not in the other:"


def test_cli_changes_follow_the_verdict(gpu, tmp_path):
    a, ca = _cli_scene(1)
    b, cb = _cli_scene(2, boxes=3)
    fa, fb, res, dump = tmp_path / "a.ply", tmp_path / "b.ply", tmp_path / "results.txt", tmp_path / "changes.ply"
    write_ply(fa, a, rgb=ca, fmt="binary")
    write_ply(fb, b, rgb=cb, fmt="binary")
    plain = _run(["--rift", "-e", fa, fb, "--results", res])
    assert "Points that are in" not in plain
    out = _run(["--rift", "-e", fa, fb, "--results", res, "--changes", "0.1", "--dump-changes", dump])
    lines = out.splitlines()
    verdict = [l for l in lines if l in (FIRST, SECOND, SAME)]
    assert len(verdict) == 1
    if verdict[0] == SAME:
        # nothing after verdict 0, as in the reference
        assert out == plain and not dump.exists()
        return
    # the richer cloud is B of the change detection (reference :1690, :1697)
    (sentence, old, new, colours) = (IN_FIRST, b, a, ca) if verdict[0] == FIRST else (IN_SECOND, a, b, cb)
    want = cr.change_detection(old, new, 0.1)
    at = lines.index(verdict[0])
    assert lines[at + 1] == sentence and lines[at + 2] == f"{len(want)} points" and len(want) > 0
    assert (IN_FIRST in out) != (IN_SECOND in out)
    p, c = _read_xyzrgb(dump)
    assert np.array_equal(p.view(np.uint32), new[want].view(np.uint32)) and np.array_equal(c, colours[want])
    # without --changes the stdout is what it was: the two lines are all that the switch adds
    assert lines[:at + 1] + lines[at + 3:] == plain.splitlines()


def test_cli_same_information_prints_no_changes(gpu, tmp_path):
    a, ca = _cli_scene(3)
    fa, fb, res, dump = tmp_path / "a.ply", tmp_path / "b.ply", tmp_path / "results.txt", tmp_path / "changes.ply"
    write_ply(fa, a, rgb=ca, fmt="binary")
    write_ply(fb, a, rgb=ca, fmt="binary")
    out = _run(["--rift", "-e", fa, fb, "--results", res, "--changes", "0.1", "--dump-changes", dump])
    assert SAME in out and "Points that are in" not in out and not dump.exists()


def test_cli_help_names_the_switches(gpu):
    out = _run(["-h"])
    assert "--changes RES" in out and "--dump-changes" in out
