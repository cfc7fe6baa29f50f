"""pcc_cluster_descriptors on the GPU (the reference's per-cluster descriptor loop, src/comparator.cpp:1224-1290, in one call)
against the host mirrors chained per cluster (build/sift_host -> a NumPy restatement of the snap -> build/rift_host, independent of
the library): every slice carries the chain's BITS in its order, on both routes of the 700-point gate, with misses and
duplicates among the snapped points, from host and from device memory, behind pcc_region_growing_segmentation's device outputs,
on every route of the two batch limits and under both layouts.  Also: the centroids in the reference's order of additions, the
capacity protocol, octave rounds that do not depend on the number of clusters, the context handle left as it was, the C++
surface through a driver and the CLI with and without --descriptors-device."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import cluster_desc_util as cdu
from ply_util import write_ply
from pointcloudcomparator_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "build" / "comparator"
MIXED = ["sift300", "empty", "rift700", "rift701", "tiny25", "sift2000", "dups"]  # 700: the last dense size; 701: the first SIFT one
MISSES = ["sift2000", "rift701", "sift300"]


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    """(name, sift_above, snap_radius) -> the mirror chain's result for that cluster alone, computed once"""
    tmp = tmp_path_factory.mktemp("cluster_desc_chain")
    cache = {}

    def get(name, sift_above=700, snap_radius=0.05):
        pts, rgb = cdu.scene(name)
        key = (name, len(pts) > sift_above, snap_radius if len(pts) > sift_above else None)
        if key not in cache:
            cache[key] = cdu.mirror_chain(pts, rgb, tmp, f"{name.replace('-', '_')}_{len(cache)}", sift_above, snap_radius)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def ctx(gpu):
    """a context handle over a cloud that has nothing to do with the clusters"""
    p, _ = synth.rift_cloud(200, 3)
    with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
        yield ix


@pytest.fixture(scope="module")
def mixed(ctx):
    """MIXED at the reference's gate from host memory, computed once (shared: do not write to it)"""
    pts, rgb, off = cdu.concat(MIXED)
    res = ctx.cluster_descriptors(pts, rgb, off, sift_above=700)
    return pts, rgb, off, res, ctx.stats()


def _assert_chain(res, names, chain, what, **kw):
    assert res["offsets"].shape == (len(names) + 1,) and res["offsets"][0] == 0 and res["offsets"][-1] == len(res["histograms"])
    for c, name in enumerate(names):
        cdu.assert_slice(res, c, chain(name, **kw), f"{what} ({name})")
        if len(cdu.scene(name)[0]):  # (an empty cluster's NaN has no bits to compare)
            assert np.array_equal(cdu.bits(res["centroids"][c]), cdu.bits(cdu.centroid(cdu.scene(name)[0]))), f"{what} ({name}): centroid"


# ---- 1. mixed clusters at the reference's gate -------------------------------------------------------------------------------
def test_mixed_clusters_carry_the_chains_bits(mixed, chain):
    pts, rgb, off, res, stats = mixed
    _assert_chain(res, MIXED, chain, "gate 700")
    size = dict(zip(MIXED, np.diff(res["offsets"])))
    assert chain("rift700")["n_keypoints"] == 0 and res["n_keypoints"][MIXED.index("rift700")] == 0   # 700 points: dense
    assert size["rift700"] == len(chain("rift700")["index"]) > 61
    assert size["rift701"] == 61 and res["n_keypoints"][MIXED.index("rift701")] == 75                    # 701 points: not
    assert size["sift2000"] == 136 and res["n_keypoints"][MIXED.index("sift2000")] == 196
    assert size["empty"] == 0 and size["tiny25"] == len(chain("tiny25")["index"])
    assert np.isnan(res["centroids"][MIXED.index("empty")]).all()
    dense = sum(len(cdu.scene(n)[0]) for n in MIXED if len(cdu.scene(n)[0]) <= 700)
    assert stats[0] == dense and stats[1] == 2701 and stats[3] == 196 + 75 and stats[4] == 196 + 75 and stats[5] == 0
    # the indices of a SIFT-route slice name points of the cluster, with the duplicates the snap produces
    lo, hi = res["offsets"][MIXED.index("sift2000")], res["offsets"][MIXED.index("sift2000") + 1]
    idx = res["point_index"][lo:hi]
    assert (0 <= idx).all() and (idx < 2000).all() and len(np.unique(idx)) < len(idx)


# ---- 2. misses and duplicates ------------------------------------------------------------------------------------------------
def test_misses_are_dropped_and_duplicates_kept(ctx, chain):
    pts, rgb, off = cdu.concat(MISSES)
    res = ctx.cluster_descriptors(pts, rgb, off, sift_above=100, snap_radius=0.004)
    stats = ctx.stats()
    want = [chain(n, sift_above=100, snap_radius=0.004) for n in MISSES]
    assert [(w["n_keypoints"], w["hits"], w["misses"], len(w["index"])) for w in want[:2]] == [(196, 180, 16, 41), (75, 69, 6, 10)]
    _assert_chain(res, MISSES, chain, "radius 0.004", sift_above=100, snap_radius=0.004)
    assert stats[0] == 0 and stats[1] == 3001
    assert stats[3] == sum(w["n_keypoints"] for w in want) and stats[4] == sum(w["hits"] for w in want)


# ---- 3. no keypoints ---------------------------------------------------------------------------------------------------------
def test_a_cluster_without_keypoints_gives_an_empty_slice(ctx, chain):
    pts, rgb, off = cdu.concat(["tiny25"])
    assert chain("tiny25", sift_above=10)["n_keypoints"] == 0
    res = ctx.cluster_descriptors(pts, rgb, off, sift_above=10)
    assert res["offsets"].tolist() == [0, 0] and res["n_keypoints"].tolist() == [0] and len(res["histograms"]) == 0
    assert np.array_equal(cdu.bits(res["centroids"][0]), cdu.bits(cdu.centroid(pts)))
    assert ctx.stats()[1] == 25 and ctx.stats()[3] == 0 and ctx.stats()[4] == 0


# ---- 4. device memory --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["records", "float4 + words", "xyz + words"])
def test_device_tensors_give_the_bits_of_host_arrays(ctx, mixed, layout):
    import torch
    pts, rgb, off, want, _ = mixed
    if layout == "records":  # 32-byte records, rgb = pts + 16
        got = ctx.cluster_descriptors(torch.from_numpy(cdu.records(pts, rgb)).cuda(), None, off, sift_above=700)
    else:  # separate arrays: points 16 or 12 bytes apart, colour words 4 bytes apart
        p = np.concatenate([pts, np.ones((len(pts), 1), np.float32)], 1) if layout == "float4 + words" else pts
        words = torch.from_numpy(synth.pack_rgb(rgb).astype(np.int32)).cuda()
        got = ctx.cluster_descriptors(torch.from_numpy(np.ascontiguousarray(p)).cuda(), words, off, sift_above=700)
    torch.cuda.synchronize()
    cdu.assert_same_result(got, want, layout)


def test_clusters_in_the_middle_of_an_array(ctx, mixed):
    """offsets[0] > 0 and points behind the last cluster: only offsets[0] .. offsets[n] are read, from either memory space"""
    import torch
    pts, rgb, off, want, _ = mixed
    pad = 5
    rec = np.concatenate([np.full((pad, 8), np.nan, np.float32), cdu.records(pts, rgb), np.full((3, 8), np.nan, np.float32)])
    cdu.assert_same_result(ctx.cluster_descriptors(rec, None, off + pad, sift_above=700), want, "host, shifted")
    cdu.assert_same_result(ctx.cluster_descriptors(torch.from_numpy(rec).cuda(), None, off + pad, sift_above=700), want, "device, shifted")


# ---- 5. behind the segmentation call -----------------------------------------------------------------------------------------
def test_chain_behind_region_growing_segmentation_on_the_device(ctx, tmp_path):
    """walls27 with 40 points of clutter and one NaN (tests/segment_util.py): its clusters hold 729 / 728 / 729 points, so a gate
    of 728 takes both routes -- the three walls of plain walls27 are all 729 points and no gate could"""
    import torch
    from segment_util import scene, with_colour
    seg = ctx.region_growing_segmentation(torch.from_numpy(with_colour(scene("walls27+clutter+nan"))).cuda(), has_rgb=True)
    offsets = seg["offsets"]
    sizes = np.diff(offsets)
    gate = int(sizes.min())
    assert seg["n_clusters"] == 3 and sizes.min() < sizes.max() and seg["cluster_points"].is_cuda
    got = ctx.cluster_descriptors(seg["cluster_points"], None, offsets, sift_above=gate)  # in place: records of 32 bytes, rgb = pts + 16
    torch.cuda.synchronize()
    stats = ctx.stats()
    assert stats[0] == int(sizes[sizes <= gate].sum()) > 0 and stats[1] == int(sizes[sizes > gate].sum()) > 0
    # the existing batch calls on the downloaded clusters
    rec = seg["cluster_points"].cpu().numpy()
    clusters = [np.ascontiguousarray(rec[offsets[c]:offsets[c + 1]]) for c in range(3)]
    large = [c for c in range(3) if sizes[c] > gate]
    kp, koff, snap = ctx.sift_keypoints_batch([clusters[c] for c in large], snap_radius=0.05)
    clouds, picked = list(clusters), {}
    for i, c in enumerate(large):
        s = snap[koff[i]:koff[i + 1]]
        picked[c] = s[s >= 0]
        clouds[c] = np.ascontiguousarray(clusters[c][picked[c]])
        assert got["n_keypoints"][c] == koff[i + 1] - koff[i]
    want = ctx.rift_descriptors_batch(clouds)
    for c in range(3):
        h, j = want[c]
        cdu.assert_slice(got, c, (h, picked[c][j].astype(np.int32) if c in picked else j), "behind the segmentation")
        assert np.array_equal(cdu.bits(got["centroids"][c]), cdu.bits(cdu.centroid(clusters[c])))
    # and the mirror says the dense clusters yield descriptors (the SIFT route may find none on this lattice)
    for c in range(3):
        if c in picked:
            continue
        rgb = np.stack([(clusters[c].view(np.uint32)[:, 4] >> s) & 255 for s in (16, 8, 0)], 1).astype(np.uint8)
        m = cdu.mirror_chain(np.ascontiguousarray(clusters[c][:, :3]), rgb, tmp_path, f"wall{c}", sift_above=gate)
        assert len(m["index"]) > 0
        cdu.assert_slice(got, c, (m["hist"], m["index"]), "behind the segmentation, mirror")


# ---- 6. routes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option,value,work_points", [
    (capi.OPT_SIFT_BATCH_BRUTE_MAX, 1000, 2000),                          # sift2000 goes to the work handle
    (capi.OPT_RIFT_BATCH_BRUTE_MAX, 50, 300 + 700 + 75 + 196 + 330),      # only tiny25 stays in the concatenation
    (capi.OPT_SIFT_LAYOUT, 0, 0),
    (capi.OPT_RIFT_LAYOUT, 0, 0),
])
def test_every_route_gives_the_same_bits(ctx, mixed, option, value, work_points):
    pts, rgb, off, want, _ = mixed
    before = ctx.get_option(option)
    ctx.set_option(option, value)
    try:
        got = ctx.cluster_descriptors(pts, rgb, off, sift_above=700)
        stats = ctx.stats()
    finally:
        ctx.set_option(option, before)
    cdu.assert_same_result(got, want, f"option {option} = {value}")
    assert stats[5] == work_points and stats[3] == 196 + 75 and stats[4] == 196 + 75


def test_both_limits_at_once_from_device_memory(ctx, mixed):
    import torch
    pts, rgb, off, want, _ = mixed
    ctx.set_option(capi.OPT_SIFT_BATCH_BRUTE_MAX, 1000)
    ctx.set_option(capi.OPT_RIFT_BATCH_BRUTE_MAX, 50)
    try:
        got = ctx.cluster_descriptors(torch.from_numpy(cdu.records(pts, rgb)).cuda(), None, off, sift_above=700)
    finally:
        ctx.set_option(capi.OPT_SIFT_BATCH_BRUTE_MAX, 8192)
        ctx.set_option(capi.OPT_RIFT_BATCH_BRUTE_MAX, 8192)
    cdu.assert_same_result(got, want, "both limits")


# ---- 7. centroids ------------------------------------------------------------------------------------------------------------
def test_centroids_add_in_index_order(ctx):
    sizes = [1, 63, 64, 65, 129, 2000]
    clouds = [cdu.scene(f"rift{n}") for n in sizes]
    pts = [c[0] + np.float32(3.0) for c in clouds]
    nan = pts[3].copy()
    nan[17, 1] = np.nan
    pts += [np.zeros((0, 3), np.float32), nan]
    rgb = [c[1] for c in clouds] + [cdu.EMPTY[1], clouds[3][1]]
    # the inputs tell the orders apart: at 2000 points the sequential sum is neither the double sum rounded once ...
    big = pts[5]
    seq = np.cumsum(big, axis=0, dtype=np.float32)[-1]
    assert (cdu.bits(seq) != cdu.bits(big.astype(np.float64).sum(0).astype(np.float32))).all()
    tree = np.zeros(3, np.float32)  # ... nor a 64-wide tree sum per tile
    for t0 in range(0, len(big), 64):
        lanes = np.zeros((64, 3), np.float32)
        lanes[:len(big[t0:t0 + 64])] = big[t0:t0 + 64]
        w = 32
        while w:
            lanes[:w] = lanes[:w] + lanes[w:2 * w]
            w //= 2
        tree = tree + lanes[0]
    assert (cdu.bits(seq) != cdu.bits(tree)).any()
    off = np.concatenate([[0], np.cumsum([len(p) for p in pts])])
    res = ctx.cluster_descriptors(np.ascontiguousarray(np.concatenate(pts)), np.ascontiguousarray(np.concatenate(rgb)), off, sift_above=None)
    for c, p in enumerate(pts[:6]):
        assert np.array_equal(cdu.bits(res["centroids"][c]), cdu.bits(cdu.centroid(p))), f"{len(p)} points"
    assert np.isnan(res["centroids"][6]).all()                                       # empty: 0.0f / 0.0f
    assert np.isnan(res["centroids"][7][1]) and np.array_equal(cdu.bits(res["centroids"][7][[0, 2]]), cdu.bits(cdu.centroid(nan)[[0, 2]]))
    assert (res["n_keypoints"] == 0).all() and ctx.stats()[1] == 0


# ---- 8. the capacity protocol ------------------------------------------------------------------------------------------------
def test_short_capacity_overflows_names_the_room_and_the_retry_succeeds(ctx, mixed):
    pts, rgb, off, want, _ = mixed
    need = int(want["offsets"][-1])
    call = cdu.RawClusterDesc(capacity=need - 1, records=cdu.records(pts, rgb), offsets=off)
    assert call(ctx._h) == -6  # PCC_ERR_OVERFLOW
    assert b"descriptors, room for" in capi.LIB.pcc_last_error()
    assert np.array_equal(call.out["out_offsets"].astype(np.int64), want["offsets"])  # the offsets that would have been returned
    assert all((v.view(np.uint8) == 0x5A).all() for k, v in call.out.items() if k != "out_offsets")  # nothing else written
    exact = cdu.RawClusterDesc(capacity=need, records=cdu.records(pts, rgb), offsets=off)
    assert exact(ctx._h) == 0
    cdu.assert_same_result(dict(histograms=exact.out["hist"], point_index=exact.out["index"], offsets=exact.out["out_offsets"].astype(np.int64),
                                n_keypoints=exact.out["nkp"], centroids=exact.out["cent"]), want, "capacity exactly met")
    cdu.assert_same_result(ctx.cluster_descriptors(pts, rgb, off, sift_above=700, capacity=10), want, "the wrapper's retry")


# ---- 9. context and rounds ---------------------------------------------------------------------------------------------------
def test_rounds_do_not_depend_on_the_clusters_and_the_context_is_left_alone(gpu):
    own, _ = synth.rift_cloud(5000, 23)
    q, _ = synth.rift_cloud(700, 29)
    names = ["sift300", "rift701", "sift2000"]
    p3, c3, o3 = cdu.concat(names)
    p30, c30, o30 = cdu.concat(names * 10)
    with capi.Index(own, engine=capi.ENGINE_GRID, device=0) as ix:
        i0, d0 = ix.nn1(q)
        r3 = ix.cluster_descriptors(p3, c3, o3, sift_above=400)
        s3 = ix.stats()
        r30 = ix.cluster_descriptors(p30, c30, o30, sift_above=400)
        s30 = ix.stats()
        i1, d1 = ix.nn1(q)
        assert ix.n_original == 5000
    assert s3[2] == s30[2] > 0 and s30[0] == 10 * s3[0] > 0 and s30[1] == 10 * s3[1] and s30[3] == 10 * s3[3] > 0
    for c in range(30):
        lo, hi = r3["offsets"][c % 3], r3["offsets"][c % 3 + 1]
        cdu.assert_slice(r30, c, (r3["histograms"][lo:hi], r3["point_index"][lo:hi]), "copies")
        assert r30["n_keypoints"][c] == r3["n_keypoints"][c % 3]
    assert np.array_equal(cdu.bits(r30["centroids"]), cdu.bits(np.tile(r3["centroids"], (10, 1))))
    assert np.array_equal(i0, i1) and np.array_equal(cdu.bits(d0), cdu.bits(d1))  # the context's own index is as it was


# ---- 10. C++ and the CLI -----------------------------------------------------------------------------------------------------
def test_cpp_cluster_descriptors_equals_the_python_result(mixed, tmp_path):
    pts, rgb, off, want, _ = mixed
    if not cdu.DRIVER.exists():
        subprocess.check_call(["make", "build/cluster_desc_driver"], cwd=ROOT)
    cdu.assert_same_result(cdu.run_driver(pts, rgb, off, tmp_path, sift_above=700), want, "pcc::clusterDescriptors")


def test_cli_descriptors_device_writes_the_same_results_and_descriptors(gpu, tmp_path):
    from test_rift_batch_gpu import _cli_scene
    a, ca = _cli_scene(1, boxes=2, big=True)
    b, cb = _cli_scene(2, boxes=2, big=True)
    fa, fb = tmp_path / "a.ply", tmp_path / "b.ply"
    write_ply(fa, a, rgb=ca, fmt="binary")
    write_ply(fb, b, rgb=cb, fmt="binary")
    if not EXE.exists():
        subprocess.check_call(["make", "cli"], cwd=ROOT)
    outs = {}
    for tag, extra in (("sequence", []), ("device", ["--descriptors-device"])):
        r = subprocess.run([str(EXE), "--rift", "--sift"] + extra + ["-e", str(fa), str(fb), "--results", str(tmp_path / f"{tag}.txt"),
                                                                     "--dump-descriptors", str(tmp_path / tag)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 1, r.stdout[-2000:] + r.stderr[-2000:]  # the reference always returns 1
        outs[tag] = r.stdout
    assert outs["sequence"] == outs["device"]  # (the CLI prints no timing line)
    assert (tmp_path / "sequence.txt").read_text() == (tmp_path / "device.txt").read_text()
    for k in (1, 2):
        dumped = (tmp_path / f"device_{k}.txt").read_text()
        assert dumped == (tmp_path / f"sequence_{k}.txt").read_text() and dumped.count("\n") > 3
    found = [int(x) for x in re.findall(r"Computed (\d+) SIFT Keypoints", outs["device"])]
    assert len(found) == 2 and all(f > 0 for f in found), found  # one cluster above 700 points per scene
