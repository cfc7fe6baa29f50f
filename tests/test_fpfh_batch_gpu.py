"""pcc_fpfh_descriptors_batch on the GPU (processFPFH, reference src/comparator.cpp:824-875, for every cluster in one call).
The expected values come from the host mirror of the pipeline (build/fpfh_host: the headers the kernels are compiled from,
exhaustive rows, one core) run on each cluster ALONE: every slice of a batch -- histogram bits and local point indices --
equals the mirror's.  The GPU is never compared with the code under test.  No tolerance anywhere."""
import ctypes as C
import gc
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fpfh_util
from pointcloudcomparator_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
BATCH_DRIVER = ROOT / "build" / "fpfh_batch_driver"
EMPTY = np.zeros((0, 3), np.float32)
NOTHING = (np.zeros((0, 33), np.float32), np.zeros(0, np.int32))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _host(x):
    return x.cpu().numpy() if capi._is_torch(x) else np.asarray(x)


def _assert_same(got, want, what=""):
    gh, gi = _host(got[0]), _host(got[1])
    wh, wi = want
    assert np.array_equal(gi, wi), f"{what}: kept point indices differ"
    assert gh.shape == wh.shape == (len(wi), 33)
    differ = (_bits(gh) != _bits(wh)).any(1)
    assert not differ.any(), f"{what}: {int(differ.sum())} of {len(wi)} histograms differ in their bits, first {int(np.argmax(differ))}"


def _cloud(n, seed=None):
    """the generator of the single call's scenes at their density (600 points per 0.12 m cube), in the same corner of space
    whatever n: clusters of one batch overlap, so a neighbour from another cluster would change bits"""
    return synth.rift_cloud(n, 100 + n if seed is None else seed, extent=0.12 * (n / 600) ** (1 / 3))[0]


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    """tag, points[, radii] -> (hist, index) of build/fpfh_host on that cluster alone, computed once per tag and left unchanged"""
    tmp = tmp_path_factory.mktemp("fpfh_batch_host")
    cache = {}

    def get(tag, points, radii=()):
        key = (tag, tuple(radii))
        if key not in cache:
            got = NOTHING if len(points) == 0 else fpfh_util.run_host(points, tmp, tag=f"{tag}_{len(cache)}", radii=radii)[:2]
            got[0].setflags(write=False)
            got[1].setflags(write=False)
            cache[key] = got
        return cache[key]
    return get


@pytest.fixture(scope="module")
def ctx(gpu):
    """one context handle for the module: it indexes a cloud of its own, which no batch may read or change"""
    pts = synth.corridor_cloud(5000, synth.SEED_A)
    with capi.Index(pts, engine=capi.ENGINE_GRID, device=0) as ix:
        yield ix, pts


def _check(ix, clouds, want, what, **kw):
    got = ix.fpfh_descriptors_batch(clouds, **kw)
    assert len(got) == len(clouds)
    for k, (g, w) in enumerate(zip(got, want)):
        _assert_same(g, w, f"{what}, cluster {k}")
        assert (np.diff(_host(g[1])) > 0).all()  # ascending local indices
    return got


SIZES = (1, 2, 3, 63, 64, 65, 257, 700, 2049)


@pytest.mark.parametrize("layout", [1, 0])
def test_overlapping_clusters_carry_the_mirrors_bits(ctx, mirror, layout):
    """sizes around the wave width, the largest query block and the 2048-point LDS tile (2049: one point past it), an empty
    cluster in the middle, and the single call's scenes with non-finite points, exact duplicates and short rows: all in the same
    corner of space"""
    ix, _ = ctx
    clouds = [(f"n{n}", _cloud(n)) for n in SIZES]
    clouds.insert(5, ("empty", EMPTY))
    clouds += [(name, fpfh_util.scene(name)) for name in ("non-finite", "duplicates", "short-rows")]
    want = [mirror(tag, p) for tag, p in clouds]
    # the mirror first: no comparison of empty sets by accident
    for (tag, p), w in zip(clouds, want):
        if tag.startswith("n") and tag != "non-finite":
            assert len(w[1]) == (0 if len(p) < 3 else len(p)), tag
    by_tag = {tag: (p, w) for (tag, p), w in zip(clouds, want)}
    assert 0 < len(by_tag["non-finite"][1][1]) < len(by_tag["non-finite"][0])
    assert not np.isfinite(by_tag["non-finite"][0]).all()
    assert len(fpfh_util.duplicate_pairs(by_tag["duplicates"][0])) == 20 and len(by_tag["duplicates"][1][1]) > 300
    assert len(by_tag["short-rows"][1][1]) > 150
    ix.set_option(capi.OPT_FPFH_LAYOUT, layout)
    try:
        got = _check(ix, [p for _, p in clouds], want, f"layout {layout}")
        stats = ix.stats()
    finally:
        ix.set_option(capi.OPT_FPFH_LAYOUT, 1)
    assert got[0][0].dtype == np.float32 and got[0][1].dtype == np.int32
    assert (int(stats[0]), int(stats[1]), int(stats[2])) == (sum(len(p) for _, p in clouds), 0, 1)


# ---- the prefix boundary ---------------------------------------------------------------------------------------------------------
NORMAL_R = 0.03125  # its square, 2^-10, is exact in float32


def _boundary_lattice():
    """12 x 12 points of one layer, 2^-6 apart in x and y from 0.25 on, z a relief of multiples of 2^-9 that depends on (i mod 2,
    j mod 2) alone: every coordinate and every difference is exact, and points two steps apart along an axis have dz = 0 and
    d2 = (2^-5)^2 = 2^-10 EXACTLY -- outside the row at NORMAL_R (strict <), inside the row at 0.05"""
    relief = np.array([[0.0, 3.0], [5.0, 2.0]])
    i, j = np.meshgrid(np.arange(12), np.arange(12), indexing="ij")
    pts = np.stack([0.25 + i * 2.0 ** -6, 0.25 + j * 2.0 ** -6, 0.25 + relief[i % 2, j % 2] * 2.0 ** -9], -1).reshape(-1, 3)
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)
    return np.ascontiguousarray(pts.astype(np.float32))


def test_entries_exactly_at_the_normal_radius_end_the_prefix(ctx, mirror):
    ix, _ = ctx
    p = _boundary_lattice()
    d = p[:, None, :] - p[None, :, :]
    d = d * d
    d2 = (d[..., 0] + d[..., 1]) + d[..., 2]  # the library's arithmetic, in float32
    assert d2.dtype == np.float32
    r2n, r2f = np.float32(NORMAL_R * NORMAL_R), np.float32(0.05 * 0.05)
    assert r2n == np.float32(2.0 ** -10)
    on_boundary = int((d2 == r2n).sum())
    assert on_boundary >= 2 * 2 * 12 * 10 and (r2n < r2f)  # every point's partners two steps along x and y, both directions
    assert int(((d2 < r2n).sum(1) >= 3).sum()) == len(p)
    want = mirror("boundary", p, radii=(NORMAL_R, 0.05))
    assert len(want[1]) > len(p) // 2
    _check(ix, [p, _cloud(65), p], [want, mirror("n65b", _cloud(65), radii=(NORMAL_R, 0.05)), want], "boundary lattice",
           normal_radius=NORMAL_R, fpfh_radius=0.05)
    assert int(ix.stats()[2]) == 1


@pytest.mark.parametrize("radii, n_csr", [((0.025, 0.045), 1), ((0.04, 0.04), 1), ((0.05, 0.03), 2)])
def test_other_radii(ctx, mirror, radii, n_csr):
    """a prefix at radii of the call's own; equal radii: the prefix is the whole row; normal_radius > fpfh_radius: two CSRs"""
    ix, _ = ctx
    clouds = [fpfh_util.scene("volume300"), _cloud(65), fpfh_util.scene("isolated")]
    want = [mirror(f"radii{k}", p, radii=radii) for k, p in enumerate(clouds)]
    assert len(want[0][1]) > 250 and len(want[2][1]) > 0
    _check(ix, clouds, want, f"radii {radii}", normal_radius=radii[0], fpfh_radius=radii[1])
    assert int(ix.stats()[2]) == n_csr


# ---- table indexing ----------------------------------------------------------------------------------------------------------------
def test_the_same_cluster_several_times(ctx, mirror):
    ix, _ = ctx
    a, iso = _cloud(257), fpfh_util.scene("isolated")
    wa, wi = mirror("n257", a), mirror("isolated", iso)
    assert len(wa[1]) == 257 and 0 < len(wi[1]) < len(iso)
    _check(ix, [a, iso, a, a, iso], [wa, wi, wa, wa, wi], "repeated")


def test_many_small_clusters(ctx, mirror):
    """200 clusters of 24 ... 40 points: table indexing and bases"""
    ix, _ = ctx
    clouds = [_cloud(24 + k % 17, seed=1000 + k) for k in range(200)]
    want = [mirror(f"small{k}", p) for k, p in enumerate(clouds)]
    assert sum(len(w[1]) for w in want) > 0.9 * sum(len(p) for p in clouds)
    _check(ix, clouds, want, "200 clusters")


def test_full_query_blocks(ctx, mirror):
    """96 clusters of 700 points: the one batch of this file large enough for the table to keep its blocks of 64 queries"""
    ix, _ = ctx
    clouds = [_cloud(700, seed=3000 + k) for k in range(96)]
    want = [mirror(f"full{k}", p) for k, p in enumerate(clouds)]
    assert sum(len(w[1]) for w in want) == 96 * 700
    _check(ix, clouds, want, "96 clusters of 700")


def test_long_rows_and_several_lds_tiles(ctx, mirror):
    """4000 points in the 0.12 m cube: most 5 cm rows are longer than the 512 entries the register sort takes (the long-row
    sort), and the cluster is two LDS tiles; alone and beside a small cluster"""
    ix, _ = ctx
    big, small = synth.rift_cloud(4000, 31, extent=0.12)[0], _cloud(300)
    rows = np.zeros(len(big), np.int64)
    for s in range(0, len(big), 500):  # the library's arithmetic: ((dx * dx) + dy * dy) + dz * dz in float32
        d = big[s:s + 500, None, :] - big[None, :, :]
        d = d * d
        rows[s:s + 500] = (((d[..., 0] + d[..., 1]) + d[..., 2]) < np.float32(0.05 * 0.05)).sum(1)
    assert (rows > 512).sum() > 1000
    wb, ws = mirror("big4000", big), mirror("n300", small)
    assert len(wb[1]) == 4000 and len(ws[1]) == 300
    _check(ix, [big], [wb], "4000 points alone")
    _check(ix, [small, big], [ws, wb], "300 points beside 4000")


# ---- the work-handle route ---------------------------------------------------------------------------------------------------------
def test_work_handle_route_gives_the_same_bits(ctx, mirror):
    import torch
    ix, _ = ctx
    clouds = [_cloud(300), _cloud(600), _cloud(700)]
    want = [mirror(f"n{len(p)}", p) for p in clouds]
    assert [len(w[1]) for w in want] == [300, 600, 700]
    default = ix.get_option(capi.OPT_FPFH_BATCH_BRUTE_MAX)
    assert default >= 700
    dev = torch.from_numpy(np.concatenate(clouds)).cuda()
    offsets = np.cumsum([0] + [len(p) for p in clouds])
    ix.set_option(capi.OPT_FPFH_BATCH_BRUTE_MAX, 500)
    try:
        _check(ix, clouds, want, "limit 500, host")
        stats = ix.stats()
        got = ix.fpfh_descriptors_batch(dev, offsets)
        torch.cuda.synchronize()
        for k, (g, w) in enumerate(zip(got, want)):
            _assert_same(g, w, f"limit 500, device, cluster {k}")
        # a large cluster in front of and between small ones: the splice's other order
        _check(ix, [clouds[2], clouds[0], clouds[1], clouds[0]], [want[2], want[0], want[1], want[0]], "limit 500, large first")
    finally:
        ix.set_option(capi.OPT_FPFH_BATCH_BRUTE_MAX, default)
    assert (int(stats[0]), int(stats[1])) == (300, 1300)
    _check(ix, clouds, want, "limit back")  # the same handle, the limit set back
    stats = ix.stats()
    assert (int(stats[0]), int(stats[1])) == (1600, 0)


# ---- memory spaces -----------------------------------------------------------------------------------------------------------------
def test_memory_spaces_and_strides_give_the_same_bits(ctx, mirror):
    import torch
    ix, _ = ctx
    clouds = [_cloud(257), EMPTY, fpfh_util.scene("isolated"), _cloud(65)]
    want = [mirror("n257", clouds[0]), NOTHING, mirror("isolated", clouds[2]), mirror("n65", clouds[3])]
    offsets = np.cumsum([0] + [len(p) for p in clouds])
    allp = np.concatenate(clouds)
    rec = fpfh_util.xyzrgb_records(allp)  # pcl::PointXYZRGB: 32-byte records
    got = _check(ix, clouds, want, "a list of host arrays")
    assert all(isinstance(h, np.ndarray) and isinstance(i, np.ndarray) for h, i in got)
    _check(ix, [fpfh_util.xyzrgb_records(p) for p in clouds], want, "a list of host records")
    for what, pts in (("host records + offsets", rec), ("host points + offsets", allp), ("torch host points + offsets", torch.from_numpy(allp))):
        got = ix.fpfh_descriptors_batch(pts, offsets)
        assert all(isinstance(h, np.ndarray) for h, _ in got)
        for k, (g, w) in enumerate(zip(got, want)):
            _assert_same(g, w, f"{what}, cluster {k}")
    # device memory: 32-byte records (16-byte loads) and 12-byte points that start 4 bytes into an allocation (scalar loads)
    flat = torch.zeros(3 * len(allp) + 1, dtype=torch.float32, device="cuda")
    odd = flat[1:].view(len(allp), 3)
    odd.copy_(torch.from_numpy(allp))
    assert odd.data_ptr() % 16 == 4 and odd.stride(0) == 3
    d_rec = torch.from_numpy(rec).cuda()
    assert d_rec.data_ptr() % 16 == 0
    for what, pts in (("device records + offsets", d_rec), ("device points at an odd alignment", odd)):
        got = ix.fpfh_descriptors_batch(pts, offsets)
        torch.cuda.synchronize()
        assert all(h.is_cuda and i.is_cuda and h.dtype == torch.float32 and i.dtype == torch.int32 for h, i in got)
        for k, (g, w) in enumerate(zip(got, want)):
            _assert_same(g, w, f"{what}, cluster {k}")
    # offsets that do not start at 0: the records in front are not read
    got = ix.fpfh_descriptors_batch(d_rec, offsets[2:])
    torch.cuda.synchronize()
    for k, (g, w) in enumerate(zip(got, want[2:])):
        _assert_same(g, w, f"offsets from {offsets[2]}, cluster {k}")
    # a list of device tensors
    got = ix.fpfh_descriptors_batch([torch.from_numpy(p).cuda() for p in clouds])
    torch.cuda.synchronize()
    assert all(h.is_cuda for h, _ in got)
    for k, (g, w) in enumerate(zip(got, want)):
        _assert_same(g, w, f"a list of device tensors, cluster {k}")


# ---- the chain, and nothing else changes ---------------------------------------------------------------------------------------
def test_device_resident_slices_feed_match_fpfh_batch(ctx, mirror):
    import torch
    ix, _ = ctx
    scene1 = [_cloud(257), _cloud(65), EMPTY, fpfh_util.scene("isolated")]
    # (descriptors of unrelated clusters are further apart than the threshold: scene 2 holds two clusters of scene 1 again)
    scene2 = [_cloud(257), _cloud(64), _cloud(63), fpfh_util.scene("isolated")[::-1].copy()]
    out = []
    for scene in (scene1, scene2):
        dev = torch.from_numpy(np.concatenate(scene)).cuda()
        got = ix.fpfh_descriptors_batch(dev, np.cumsum([0] + [len(p) for p in scene]))
        base = got[0][0].data_ptr()
        assert all(h.is_cuda for h, _ in got)
        at = 0
        for h, _ in got:  # views of ONE output array, one behind the other
            assert len(h) == 0 or (h.data_ptr() == base + at * 132 and (len(h) < 2 or h.stride(0) == 33))
            at += len(h)
        out.append(got)
    torch.cuda.synchronize()
    for k, p in enumerate(scene1):
        _assert_same(out[0][k], mirror(f"chain1_{k}", p), f"scene 1, cluster {k}")
    pairs_dev = [(a[0], b[0]) for a, b in zip(out[0], out[1])]
    assert len(pairs_dev) == 4 and len(pairs_dev[2][0]) == 0 and len(pairs_dev[2][1]) > 0
    pairs_host = [(a.cpu().numpy(), b.cpu().numpy()) for a, b in pairs_dev]
    rows_dev, d2_dev = ix.match_fpfh_batch(pairs_dev, return_d2=True)
    rows_host, d2_host = ix.match_fpfh_batch(pairs_host, return_d2=True)
    assert len(rows_dev) == 4
    assert len(rows_host[0]) == 1 + 257 and len(rows_host[3]) > 1 + 400  # the repeated clusters match: more than the dummies
    for k in range(4):
        assert np.array_equal(rows_dev[k], rows_host[k]) and np.array_equal(_bits(d2_dev[k]), _bits(d2_host[k])), k
    assert len(rows_host[2]) == 1  # the empty side: the dummy alone


def test_the_call_changes_nothing_else(ctx, mirror):
    """between two ordinary searches on the context handle: its own cloud answers as before"""
    import oracle
    ix, pts = ctx
    q = synth.corridor_cloud(1000, synth.SEED_B)
    oi, od = oracle.nn1_exhaustive(pts, q)
    i0, d0 = ix.nn1(q)
    p = _cloud(257)
    got = ix.fpfh_descriptors_batch([p, p[:65]])
    i1, d1 = ix.nn1(q)
    _assert_same(got[0], mirror("n257", p), "between two searches")
    assert len(got[1][1]) > 0
    for i, d in ((i0, d0), (i1, d1)):
        assert np.array_equal(i, oi) and np.array_equal(_bits(d), _bits(od))
    assert ix.size == 5000
    # and the module-level form with a handle of its own
    own = capi.fpfh_descriptors_batch([p])
    _assert_same(own[0], mirror("n257", p), "one-point context")


def _live():
    gc.collect()
    v = (C.c_uint64 * 2)()
    assert capi.LIB.pcc_debug_live_buffers(v) == 0
    return int(v[0]), int(v[1])


def test_a_destroyed_handle_gives_back_what_both_routes_took(gpu, mirror):
    import torch
    clouds = [_cloud(300), _cloud(600), _cloud(700)]
    want = [mirror(f"n{len(p)}", p) for p in clouds]
    dev = torch.from_numpy(np.concatenate(clouds)).cuda()
    offsets = np.cumsum([0] + [len(p) for p in clouds])
    before = _live()
    with capi.Index(np.zeros((1, 3), np.float32), engine=capi.ENGINE_BRUTE, device=0) as ix:
        _check(ix, clouds, want, "batch route")
        ix.set_option(capi.OPT_FPFH_BATCH_BRUTE_MAX, 500)
        _check(ix, clouds, want, "both routes, host")
        got = ix.fpfh_descriptors_batch(dev, offsets)
        torch.cuda.synchronize()
        _assert_same(got[2], want[2], "both routes, device")
        assert _live() != before
    assert _live() == before


def test_refusals_on_a_live_handle(ctx, mirror):
    ix, _ = ctx
    p = _cloud(300)
    with pytest.raises(Exception, match=r"only 11 \+ 11 \+ 11 bins"):
        ix.fpfh_descriptors_batch([p], nr_bins=(11, 11, 10))
    with pytest.raises(Exception, match="bad radius"):
        ix.fpfh_descriptors_batch([p], fpfh_radius=0.0)
    assert ix.fpfh_descriptors_batch([]) == []
    _check(ix, [p], [mirror("n300", p)], "after the refusals")  # and the handle still works


def test_cpp_processFPFHBatch_equals_the_loop_and_the_mirror(gpu, mirror, tmp_path):
    if not BATCH_DRIVER.exists():
        subprocess.check_call(["make", "build/fpfh_batch_driver"], cwd=ROOT)
    clouds = [("isolated", fpfh_util.scene("isolated")), ("empty", EMPTY), ("n65", _cloud(65)), ("non_finite", fpfh_util.scene("non-finite"))]
    files = []
    for tag, p in clouds:
        files.append(tmp_path / f"{tag}.in")
        fpfh_util.write_cloud(files[-1], p)
    r = subprocess.run([str(BATCH_DRIVER), str(tmp_path / "out")] + [str(f) for f in files], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "clouds=4" in r.stdout and "differ_from_loop=0" in r.stdout  # pcc::processFPFH per cloud, compared in the driver
    for k, (tag, p) in enumerate(clouds):
        _assert_same(fpfh_util.read_result(tmp_path / f"out.{k}"), mirror(tag, p), f"pcc::processFPFHBatch vs mirror, {tag}")
