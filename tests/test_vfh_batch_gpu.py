"""pcc_vfh_descriptors_batch on the GPU (processVHF, reference src/comparator.cpp:482-516, for every cluster in one call).
The expected values come from the host mirror of the pipeline (build/vfh_host: the headers the kernels are compiled from,
exhaustive rows, one core) run on each cluster ALONE -- where a test has hundreds of tiny clusters, from the existing single
call pcc_vfh_descriptor on each cluster -- and never from the code under test.  Bits are compared: no tolerance anywhere.  All
clusters of a batch lie in the same corner of space, and every test first asserts that the expected descriptors of its
distinct clusters differ from one another."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fpfh_util
import vfh_util
import vfh_batch_util as U
from pointcloudcomparator_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "pointcloudcomparator_amd" / "csrc"


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return U.Mirror(tmp_path_factory.mktemp("vfh_batch_host"))


@pytest.fixture(scope="module")
def ctx(gpu):
    """one context handle for the module: it indexes a cloud of its own, which no batch may read or change"""
    pts = synth.corridor_cloud(5000, synth.SEED_A)
    with capi.Index(pts, engine=capi.ENGINE_GRID, device=0) as ix:
        yield ix, pts


def _check(ix, clouds, want, what, **kw):
    got = ix.vfh_descriptors_batch(clouds, **kw)
    assert len(got) == len(clouds)
    for k, (g, w) in enumerate(zip(got, want)):
        U.assert_same(g, w, f"{what}, cluster {k}")
    return got


def _offsets(clouds):
    return np.cumsum([0] + [len(p) for p in clouds])


# the wave edges, the 512-point tile edge of the chains and both sides of the 1024-point vote item
SIZES = (0, 1, 2, 3, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025)
SCENES = ("centroid-hit", "isolated", "duplicates", "slab")


def test_overlapping_clusters_carry_the_mirrors_bits(ctx, mirror):
    ix, _ = ctx
    # the sizes above are the edges of what the kernels are built with
    dev = (CSRC / "vfh_device.hpp").read_text()
    assert "VFH_CENT_ROWS = 8" in dev and "VFH_CENT_TILE = 64 * VFH_CENT_ROWS" in dev and U.CENT_TILE == 64 * 8
    assert "vfh_centroid_chains(" in (CSRC / "vfh_batch.hip").read_text()  # the batch kernel parks the single call's tile
    assert f"VFH_BATCH_VOTE_POINTS = {U.VOTE_POINTS}" in (CSRC / "vfh_batch_plan.hpp").read_text()
    for edge in (U.CENT_TILE, U.VOTE_POINTS):
        assert {edge - 1, edge, edge + 1} <= set(SIZES)
    clouds = [(f"n{n}", U.cloud(n)) for n in SIZES]
    clouds.insert(7, ("empty", U.EMPTY))  # an empty cluster in the middle
    clouds += [(name, vfh_util.scene(name)) for name in SCENES]
    want = [mirror(tag, p) for tag, p in clouds]
    assert [len(w) for w in want] == [U.expected_rows(len(p)) for _, p in clouds]
    U.assert_distinct(want, "edges and scenes")
    got = _check(ix, [p for _, p in clouds], want, "edges and scenes")
    stats = ix.stats()
    assert isinstance(got[4], np.ndarray) and got[4].dtype == np.float32
    n_batch = sum(len(p) for _, p in clouds if len(p) >= 2)
    assert (int(stats[0]), int(stats[1]), int(stats[2])) == (n_batch, 0, sum(len(w) for w in want))
    # what the mirror says of the scenes: the isolated points have NaN normals and still vote (bin 0 of the viewpoint component)
    iso = want[[t for t, _ in clouds].index("isolated")][0]
    assert abs(float(iso[180:].sum(dtype=np.float64)) - 100.0) < 1e-2 and iso[180] > 0


def test_repeated_clusters_and_offsets_that_start_later(ctx, mirror):
    """the same cluster twice in one batch: both rows equal, and equal to the mirror; offsets[0] != 0, with unused records in
    front of the first cluster and behind the last"""
    import torch
    ix, _ = ctx
    a, b = U.cloud(257), vfh_util.scene("isolated")
    wa, wb = mirror("n257", a), mirror("isolated", b)
    U.assert_distinct([wa, wb], "repeated")
    got = _check(ix, [a, b, a, a, b], [wa, wb, wa, wa, wb], "repeated")
    assert np.array_equal(U.bits(got[0]), U.bits(got[2])) and np.array_equal(U.bits(got[1]), U.bits(got[4]))
    junk_front, junk_back = U.cloud(100, seed=7), U.cloud(50, seed=8)
    clouds = [a, U.EMPTY, b, a[:65]]
    want = [wa, U.NO_ROW, wb, mirror("n257_65", a[:65])]
    allp = np.concatenate([junk_front] + clouds + [junk_back])
    offsets = len(junk_front) + _offsets(clouds)
    assert offsets[0] == 100 and offsets[-1] + 50 == len(allp)
    for what, pts in (("host", allp), ("device", torch.from_numpy(allp).cuda()), ("device records", torch.from_numpy(vfh_util.xyzrgb_records(allp)).cuda())):
        got = ix.vfh_descriptors_batch(pts, offsets)
        for k, (g, w) in enumerate(zip(got, want)):
            U.assert_same(g, w, f"offsets from 100, {what}, cluster {k}")


def test_many_small_clusters(ctx):
    """300 clusters of 2 .. 40 points: the counter indexing, the one-workgroup-per-descriptor finish and the record array at
    more clusters than the other tests have.  Expected: the existing single call pcc_vfh_descriptor on each cluster."""
    ix, _ = ctx
    clouds = [U.cloud(2 + k % 39, seed=1000 + k) for k in range(300)]
    with capi.Index(clouds[0], engine=capi.ENGINE_GRID, device=0) as one:
        want = [U.single_call(one, p) for p in clouds]
    assert all(len(w) == 1 for w in want)
    # (a cluster of 2 or 3 points has NaN normals and a handful of votes: two of them may well share a descriptor; from 8
    # points on 308 bins of counts of distinct point sets do not)
    U.assert_distinct([w for w, p in zip(want, clouds) if len(p) >= 8], "300 clusters")
    _check(ix, clouds, want, "300 clusters")
    assert [int(v) for v in ix.stats()[:3]] == [sum(len(p) for p in clouds), 0, 300]


def test_both_routes_in_one_call(ctx, mirror):
    import torch
    ix, _ = ctx
    sizes = (30, 499, 1, 500, 501, 65, 1200, 0, 3)
    clouds = [U.cloud(n) for n in sizes]
    want = [mirror(f"n{n}", p) for n, p in zip(sizes, clouds)]
    U.assert_distinct(want, "both routes")
    default = ix.get_option(capi.OPT_VFH_BATCH_BRUTE_MAX)
    assert default == 8192
    dev = torch.from_numpy(np.concatenate(clouds)).cuda()
    offsets = _offsets(clouds)
    try:
        ix.set_option(capi.OPT_VFH_BATCH_BRUTE_MAX, 500)
        _check(ix, clouds, want, "limit 500, host")
        assert [int(v) for v in ix.stats()[:3]] == [30 + 499 + 500 + 65 + 3, 501 + 1200, 7]
        got = ix.vfh_descriptors_batch(dev, offsets)
        for k, (g, w) in enumerate(zip(got, want)):
            U.assert_same(g, w, f"limit 500, device, cluster {k}")
        assert [int(v) for v in ix.stats()[:3]] == [30 + 499 + 500 + 65 + 3, 501 + 1200, 7]
        hist, off = ix.vfh_descriptors_batch(dev, offsets, return_packed=True)  # rows in cluster order, whichever route wrote them
        assert off.tolist() == [0, 1, 2, 2, 3, 4, 5, 6, 6, 7] and tuple(hist.shape) == (7, 308)
        rows = [w for w in want if len(w)]
        for k in range(7):
            U.assert_same(hist[k], rows[k], f"limit 500, packed row {k}")
        ix.set_option(capi.OPT_VFH_BATCH_BRUTE_MAX, 0)  # everything on the work handle
        _check(ix, clouds, want, "limit 0, host")
        assert [int(v) for v in ix.stats()[:3]] == [0, sum(n for n in sizes if n >= 2), 7]
        got = ix.vfh_descriptors_batch(dev, offsets)
        for k, (g, w) in enumerate(zip(got, want)):
            U.assert_same(g, w, f"limit 0, device, cluster {k}")
    finally:
        ix.set_option(capi.OPT_VFH_BATCH_BRUTE_MAX, default)
    _check(ix, clouds, want, "limit back")
    assert [int(v) for v in ix.stats()[:3]] == [sum(n for n in sizes if n >= 2), 0, 7]


def test_memory_spaces_strides_and_another_radius(ctx, mirror):
    import torch
    ix, _ = ctx
    clouds = [U.cloud(257), U.EMPTY, vfh_util.scene("isolated"), U.cloud(65), U.cloud(1)]
    tags = ("n257", "empty", "isolated", "n65", "n1")
    offsets = _offsets(clouds)
    allp = np.concatenate(clouds)
    rec = vfh_util.xyzrgb_records(allp)  # pcl::PointXYZRGB: 32-byte records
    # device memory: 32-byte records (16-byte loads) and 12-byte points that start 4 bytes into an allocation (scalar loads)
    flat = torch.zeros(3 * len(allp) + 1, dtype=torch.float32, device="cuda")
    odd = flat[1:].view(len(allp), 3)
    odd.copy_(torch.from_numpy(allp))
    assert odd.data_ptr() % 16 == 4 and odd.stride(0) == 3
    d_rec = torch.from_numpy(rec).cuda()
    assert d_rec.data_ptr() % 16 == 0
    for radius in (0.03, 0.045):
        want = [mirror(t, p, radius=None if radius == 0.03 else radius) for t, p in zip(tags, clouds)]
        U.assert_distinct(want, f"radius {radius}")
        if radius != 0.03:  # the mirror differs at the other radius: the radius reaches the kernels
            assert (U.bits(want[0]) != U.bits(mirror("n257", clouds[0]))).any()
        got = _check(ix, clouds, want, f"a list of host arrays, {radius}", normal_radius=radius)
        assert all(isinstance(h, np.ndarray) for h in got)
        _check(ix, [vfh_util.xyzrgb_records(p) for p in clouds], want, f"a list of host records, {radius}", normal_radius=radius)
        for what, pts in (("host records + offsets", rec), ("host points + offsets", allp), ("torch host points + offsets", torch.from_numpy(allp))):
            got = ix.vfh_descriptors_batch(pts, offsets, radius)
            assert all(isinstance(h, np.ndarray) for h in got)
            for k, (g, w) in enumerate(zip(got, want)):
                U.assert_same(g, w, f"{what}, {radius}, cluster {k}")
        for what, pts in (("device records + offsets", d_rec), ("device points at an odd alignment", odd)):
            got = ix.vfh_descriptors_batch(pts, offsets, radius)
            assert all(h.is_cuda and h.dtype == torch.float32 for h in got)
            base = got[0].data_ptr()  # views of the call's ONE output tensor, one row behind the other
            assert got[2].data_ptr() == base + 308 * 4 and got[3].data_ptr() == base + 2 * 308 * 4
            for k, (g, w) in enumerate(zip(got, want)):
                U.assert_same(g, w, f"{what}, {radius}, cluster {k}")
        got = ix.vfh_descriptors_batch([torch.from_numpy(p).cuda() for p in clouds], normal_radius=radius)
        assert all(h.is_cuda for h in got)
        for k, (g, w) in enumerate(zip(got, want)):
            U.assert_same(g, w, f"a list of device tensors, {radius}, cluster {k}")
    # the module-level form with a handle of its own
    own = capi.vfh_descriptors_batch([clouds[0]])
    U.assert_same(own[0], mirror("n257", clouds[0]), "one-point context")
    assert ix.vfh_descriptors_batch([]) == []


def test_a_second_smaller_call_and_other_calls_on_the_handle(ctx, mirror):
    """fewer and smaller clusters after a larger call (the counters are zeroed again, stale records are not read), alternating
    with fpfh_descriptors_batch and vfh_descriptor on the same handle; the handle's own cloud still answers"""
    import oracle
    ix, pts = ctx
    q = synth.corridor_cloud(1000, synth.SEED_B)
    oi, od = oracle.nn1_exhaustive(pts, q)
    big = [U.cloud(n) for n in (513, 300, 257, 1025, 65, 64)]
    small = [U.cloud(63), U.cloud(300), U.cloud(3)]
    want_big = [mirror(f"n{len(p)}", p) for p in big]
    want_small = [mirror(f"n{len(p)}", p) for p in small]
    U.assert_distinct(want_big + [want_small[0], want_small[2]], "second call")
    own_before = np.array(ix.vfh_descriptor())
    assert own_before.shape == (308,)
    _check(ix, big, want_big, "first call")
    _check(ix, small, want_small, "second, smaller call")
    fp = ix.fpfh_descriptors_batch([small[1], big[4]])
    assert len(fp) == 2 and len(fp[0][1]) == 300
    _check(ix, big, want_big, "after fpfh_descriptors_batch")
    own_after = np.array(ix.vfh_descriptor())
    assert np.array_equal(U.bits(own_before), U.bits(own_after))
    _check(ix, small, want_small, "after vfh_descriptor")
    i1, d1 = ix.nn1(q)
    assert np.array_equal(i1, oi) and np.array_equal(U.bits(d1), U.bits(od)) and ix.size == 5000


def _raw_call(ix, pts_ptr, stride, offsets, mem, hist_ptr, out):
    off = np.ascontiguousarray(offsets, dtype=np.uintp)
    return capi.LIB.pcc_vfh_descriptors_batch(ix._h, pts_ptr, stride, off.ctypes.data, len(off) - 1, mem, 0.03, hist_ptr, out.ctypes.data)


def test_non_finite_points(ctx, mirror):
    import torch
    ix, _ = ctx
    good = [U.cloud(65), U.cloud(100), U.cloud(1), U.cloud(100, seed=5), U.cloud(64)]
    want = [mirror("n65", good[0]), mirror("n100", good[1]), U.NO_ROW, mirror("n100s5", good[3]), mirror("n64", good[4])]
    U.assert_distinct(want, "non-finite")
    bad = [p.copy() for p in good]
    bad[1][17, 1] = np.nan   # cluster 1: the lowest-numbered offender
    bad[3][5, 2] = np.inf    # cluster 3: a later one
    offsets = _offsets(bad)
    allp = np.concatenate(bad)
    dev = torch.from_numpy(allp).cuda()
    for what, mem, ptr, hist in (("host", capi.MEM_HOST, allp.ctypes.data, np.zeros((5, 308), np.float32)),
                                 ("device", capi.MEM_DEVICE, dev.data_ptr(), torch.zeros((5, 308), dtype=torch.float32, device="cuda"))):
        out = np.full(6, 99, np.uintp)
        torch.cuda.synchronize()
        st = _raw_call(ix, ptr, 12, offsets, mem, hist.ctypes.data if mem == capi.MEM_HOST else hist.data_ptr(), out)
        msg = capi.LIB.pcc_last_error()
        assert st == -5 and b"non-finite" in msg, (what, st, msg)
        assert b"cluster 1)" in msg, (what, msg)  # the lowest-numbered one (atomicMin from device memory, the first met from host memory)
        assert out.tolist() == [99] * 6, what  # out_offsets is untouched
        with pytest.raises(capi.PccError, match="non-finite") as e:
            ix.vfh_descriptors_batch(allp if mem == capi.MEM_HOST else dev, offsets)
        assert e.value.status == -5
        # the next call on the handle carries the right bits
        _check(ix, good, want, f"after the refusal, {what}")
    # a 1-point cluster holding a NaN is not an error: it is never read
    lone = [p.copy() for p in good]
    lone[2][0, 0] = np.nan
    _check(ix, lone, want, "NaN in a 1-point cluster, host")
    got = ix.vfh_descriptors_batch(torch.from_numpy(np.concatenate(lone)).cuda(), _offsets(lone))
    for k, (g, w) in enumerate(zip(got, want)):
        U.assert_same(g, w, f"NaN in a 1-point cluster, device, cluster {k}")
    # above the limit the work handle meets the point: the same status, the cluster named
    default = ix.get_option(capi.OPT_VFH_BATCH_BRUTE_MAX)
    try:
        ix.set_option(capi.OPT_VFH_BATCH_BRUTE_MAX, 80)
        with pytest.raises(capi.PccError, match=r"non-finite.*cluster 1\)") as e:
            ix.vfh_descriptors_batch(allp, offsets)
        assert e.value.status == -5
    finally:
        ix.set_option(capi.OPT_VFH_BATCH_BRUTE_MAX, default)
    _check(ix, good, want, "after the work handle's refusal")


def test_device_resident_descriptors_feed_match_vfh(ctx, mirror, tmp_path):
    """the chain: the packed device outputs of two batches go into match_vfh; the n1 x n2 float64 matrix carries the bits of
    the mirror's matchVHF on the mirror's descriptors"""
    import torch
    ix, _ = ctx
    scene1 = [("n257", U.cloud(257)), ("n1", U.cloud(1)), ("isolated", vfh_util.scene("isolated")), ("n65", U.cloud(65))]
    scene2 = [("n64", U.cloud(64)), ("slab", vfh_util.scene("slab")), ("empty", U.EMPTY), ("n257", U.cloud(257)), ("n63", U.cloud(63))]
    packed, wants = [], []
    for scene in (scene1, scene2):
        want = [mirror(t, p) for t, p in scene]
        U.assert_distinct(want, "chain")
        dev = torch.from_numpy(np.concatenate([p for _, p in scene])).cuda()
        hist, off = ix.vfh_descriptors_batch(dev, _offsets([p for _, p in scene]), return_packed=True)
        assert hist.is_cuda and off.tolist() == np.cumsum([0] + [len(w) for w in want]).tolist()
        packed.append(hist)
        wants.append(np.concatenate([w for w in want if len(w)]))
    assert tuple(packed[0].shape) == (3, 308) and tuple(packed[1].shape) == (4, 308)
    base = packed[0].data_ptr()
    dist = ix.match_vfh(packed[0], packed[1])
    assert packed[0].data_ptr() == base and dist.is_cuda and dist.dtype == torch.float64 and tuple(dist.shape) == (3, 4)
    expect = vfh_util.run_match(wants[0], wants[1], tmp_path)
    got = dist.cpu().numpy()
    assert np.array_equal(got.view(np.uint64), expect.view(np.uint64)), (got, expect)
    assert got[0, 2] == 0.0 and (got[got != got[0, 2]] > 0).all() and (got > 0).sum() == 11  # the repeated cluster, and only it


def test_cpp_processVHFBatch_and_the_matchVHF_matrix(ctx, mirror, tmp_path):
    if not U.BATCH_DRIVER.exists():
        subprocess.check_call(["make", "build/vfh_batch_driver"], cwd=ROOT)
    ix, _ = ctx
    clouds = [("isolated", vfh_util.scene("isolated")), ("empty", U.EMPTY), ("n65", U.cloud(65)), ("n1", U.cloud(1)), ("slab", vfh_util.scene("slab")),
              ("n64", U.cloud(64))]
    want = [mirror(t, p) for t, p in clouds]
    U.assert_distinct(want, "driver")
    des, dist, stdout = U.run_batch_driver([p for _, p in clouds], 3, tmp_path)
    assert "clouds=6 descriptors=4 differ_from_loop=0" in stdout  # pcc::processVHF per cloud, compared in the driver
    py = ix.vfh_descriptors_batch([p for _, p in clouds])
    for k, (tag, _) in enumerate(clouds):
        assert des[k].shape == want[k].shape, tag  # an empty and a 1-point cloud give empty descriptor clouds
        if len(want[k]):
            U.assert_same(des[k][0], want[k], f"pcc::processVHFBatch vs mirror, {tag}")
            assert np.array_equal(U.bits(des[k][0]), U.bits(py[k])), tag
    h1 = np.concatenate([d for d in des[:3] if len(d)])
    h2 = np.concatenate([d for d in des[3:] if len(d)])
    expect = capi.match_vfh(h1, h2, ctx=ix)
    assert dist.shape == expect.shape == (2, 2) and np.array_equal(dist.view(np.uint64), expect.view(np.uint64))
