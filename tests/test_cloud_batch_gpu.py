"""The three "every cloud at once" calls in turn on ONE context handle (pcc_rift_descriptors_batch, pcc_sift_keypoints_batch,
pcc_region_growing_rgb_batch: the host scaffold they share is csrc/cloud_batch.hpp and csrc/entry.hpp), once with every cloud
on the batch route and once with the two largest on the work handle -- the lease of that handle taken three times on the same
context.  Every slice equals the single call on a fresh handle bit for bit, the stats name the split, and afterwards the context
answers a plain search as before: its stream was given back."""
import numpy as np
import pytest

import sift_util
from pointcloudcomparator_amd import capi, synth

pytestmark = pytest.mark.gpu

# 2049: one past an LDS tile of the row builders; 65: one past a query block; 26: one past SIFT's 25-point gate (a lattice whose
# points keep a voxel each at the first leaf, so the cloud passes the gate and scans for its 25 neighbours)
SIZES = [0, 1, 26, 65, 300, 2049]
BRUTE_MAX = (capi.OPT_RIFT_BATCH_BRUTE_MAX, capi.OPT_SIFT_BATCH_BRUTE_MAX, capi.OPT_RGB_BATCH_BRUTE_MAX)
RGB_KW = dict(min_size=1)  # (segments of every size count as clusters: no cloud but the empty one is without one)


def clouds():
    """cut from the generator of the RIFT and SIFT batch tests, at the density of their scenes"""
    one = synth.rift_cloud(300, 7)
    return [(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8)), (one[0][:1].copy(), one[1][:1].copy()), sift_util._tiny(26),
            synth.rift_cloud(65, 7, extent=0.058), one, synth.rift_cloud(2049, 17, extent=0.18)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def alone(gpu):
    """every cloud by the single calls, each on a fresh handle: (descriptors, keypoints, snapped indices, (labels, clusters))"""
    out = []
    for p, rgb in clouds():
        if len(p) == 0:
            out.append(((np.zeros((0, 32), np.float32), np.zeros(0, np.int32)), np.zeros((0, 4), np.float32), np.zeros(0, np.int32),
                        (np.zeros(0, np.int32), 0)))
            continue
        with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
            rift = ix.rift_descriptors(rgb)
        with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
            kp = ix.sift_keypoints(p, rgb)
        with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
            snap = ix.first_within(np.ascontiguousarray(kp[:, :3]), 0.05) if len(kp) else np.zeros(0, np.int32)
        with capi.Index(p, engine=capi.ENGINE_GRID, device=0) as ix:
            grown = ix.region_growing_rgb(rgb, **RGB_KW)
        out.append((rift, kp, snap, grown))
    return out


@pytest.mark.parametrize("limit", [None, 100])
def test_three_batch_calls_on_one_context(gpu, alone, limit):
    cl = clouds()
    assert [len(p) for p, _ in cl] == SIZES
    pts, rgbs = [p for p, _ in cl], [c for _, c in cl]
    probe, _ = synth.rift_cloud(64, 5)
    ctx_cloud, _ = synth.rift_cloud(200, 3)
    with capi.Index(ctx_cloud, engine=capi.ENGINE_GRID, device=0) as ctx:
        before = ctx.nn1(probe)
        if limit is not None:
            for opt in BRUTE_MAX:
                ctx.set_option(opt, limit)
        brute_max = [int(ctx.get_option(opt)) for opt in BRUTE_MAX]
        assert brute_max == ([8192] * 3 if limit is None else [limit] * 3)
        split = (sum(s for s in SIZES if s <= brute_max[0]), sum(s for s in SIZES if s > brute_max[0]))
        assert split == ((2441, 0) if limit is None else (92, 2349))

        rift = ctx.rift_descriptors_batch(pts, rgbs)
        stats = ctx.stats()
        assert (int(stats[0]), int(stats[1])) == split, ("rift", stats[:2])
        kp, off, snap = ctx.sift_keypoints_batch(pts, rgbs, snap_radius=0.05)
        stats = ctx.stats()
        assert (int(stats[0]), int(stats[1])) == split, ("sift", stats[:2])
        grown = ctx.region_growing_rgb_batch(pts, rgbs, **RGB_KW)
        stats = ctx.stats()
        assert (int(stats[2]), int(stats[3])) == split, ("rgb", stats[2:4])

        assert len(rift) == len(grown) == len(SIZES) and off.shape == (len(SIZES) + 1,) and off[0] == 0 and off[-1] == len(kp)
        for c, (w_rift, w_kp, w_snap, w_grown) in enumerate(alone):
            what = (limit, "cloud", c, SIZES[c])
            assert rift[c][0].shape == w_rift[0].shape and np.array_equal(_bits(rift[c][0]), _bits(w_rift[0])), what
            assert np.array_equal(rift[c][1], w_rift[1]), what
            got_kp = kp[off[c]:off[c + 1]]
            assert got_kp.shape == w_kp.shape and np.array_equal(_bits(got_kp), _bits(w_kp)), what
            assert np.array_equal(snap[off[c]:off[c + 1]], w_snap), what
            assert grown[c][1] == w_grown[1] and np.array_equal(grown[c][0], w_grown[0]), what
        # no comparison above was of empty sets, on either route: the 65-point cloud stays on the batch route at both limits and
        # the 2049-point cloud leaves it at 100 (the host mirrors and the oracle give them 65 and 2049 descriptors, 6 and 206
        # keypoints, 58 and 1666 clusters)
        for c in (3, 5):
            assert len(rift[c][1]) > 0 and off[c + 1] > off[c] and grown[c][1] > 0, (limit, c)

        # the context's own stream and index are as they were
        after = ctx.nn1(probe)
        assert np.array_equal(after[0], before[0]) and np.array_equal(_bits(after[1]), _bits(before[1]))
        assert capi.LIB.pcc_index_sync(ctx._h) == 0
