"""The staging the two range-batch calls share (csrc/range_batch.hip: stage_ranges, k_range_pack, the host pack of
csrc/range_batch_plan.hpp) on the GPU, one test per entry point over its four paths: host points, host 32-byte records, device
32-byte records at 16-byte alignment (one 16-byte load a point) and device 12-byte points that start 4 bytes into an allocation
(scalar loads).  The same clusters each time -- 3, 65, 130 and 0 points, the limit lowered to 100 so that both routes run in the
one call -- with records in front of the first cluster (offsets[0] != 0) from host memory too; those records hold NaN and must
not be read.  Expected values come from the host mirrors (build/fpfh_host, build/vfh_host) on each cluster alone, never from
the library; bits are compared."""
import numpy as np
import pytest

import fpfh_util
import vfh_util
import vfh_batch_util as U
from pointcloudcomparator_amd import capi

pytestmark = pytest.mark.gpu
SIZES = (3, 65, 130, 0)
LIMIT = 100
FRONT = 5  # records in front of the first cluster


def _staging_paths(clusters):
    """name -> (points or records as the call takes them, offsets): the four ways into stage_ranges"""
    import torch
    junk = np.full((FRONT, 3), np.nan, np.float32)
    allp = np.ascontiguousarray(np.concatenate([junk] + list(clusters)))
    offsets = FRONT + np.cumsum([0] + [len(p) for p in clusters])
    assert offsets[0] != 0 and [int(n) for n in np.diff(offsets)] == list(SIZES)
    rec = fpfh_util.xyzrgb_records(allp)
    flat = torch.zeros(3 * len(allp) + 1, dtype=torch.float32, device="cuda")
    odd = flat[1:].view(len(allp), 3)
    odd.copy_(torch.from_numpy(allp))
    d_rec = torch.from_numpy(rec).cuda()
    assert rec.strides[0] == 32 and d_rec.data_ptr() % 16 == 0 and (FRONT * 32) % 16 == 0  # the first cluster is 16-byte aligned too
    assert odd.data_ptr() % 16 == 4 and odd.stride(0) == 3
    return {"host points": (allp, offsets), "host records": (rec, offsets), "device records, 16-byte loads": (d_rec, offsets),
            "device points, scalar loads": (odd, offsets)}


@pytest.fixture()
def handle(gpu):
    with capi.Index(np.zeros((1, 3), np.float32), engine=capi.ENGINE_BRUTE, device=0) as ix:
        yield ix


def test_fpfh_every_staging_path_stages_raw_coordinates(handle, tmp_path):
    """the 65-point cluster is the first 65 points of fpfh_util.scene("non-finite") (a NaN and an infinity among them): FPFH's
    instantiation of the shared pack and host loop does not flag -- no path refuses, every path gives the mirror's bits"""
    import torch
    ix = handle
    nf = np.ascontiguousarray(fpfh_util.scene("non-finite")[:65])
    assert len(nf) == 65 and np.isnan(nf).any() and np.isinf(nf).any()
    clusters = [U.cloud(3), nf, U.cloud(130), U.EMPTY]
    want = [fpfh_util.run_host(p, tmp_path, tag=f"c{k}")[:2] if len(p) else (np.zeros((0, 33), np.float32), np.zeros(0, np.int32))
            for k, p in enumerate(clusters)]
    assert 0 < len(want[1][1]) < 65 and len(want[2][1]) == 130  # the mirror drops points of the non-finite cluster, not all of them
    ix.set_option(capi.OPT_FPFH_BATCH_BRUTE_MAX, LIMIT)
    for what, (pts, offsets) in _staging_paths(clusters).items():
        got = ix.fpfh_descriptors_batch(pts, offsets)
        torch.cuda.synchronize()
        stats = ix.stats()
        assert (int(stats[0]), int(stats[1])) == (68, 130), what  # both routes ran
        assert len(got) == 4
        for k, ((gh, gi), (wh, wi)) in enumerate(zip(got, want)):
            gh, gi = U.host(gh), U.host(gi)
            assert np.array_equal(gi, wi), f"{what}, cluster {k}: kept point indices differ"
            assert gh.shape == wh.shape and np.array_equal(U.bits(gh), U.bits(wh)), f"{what}, cluster {k}: histogram bits differ"


def test_vfh_every_staging_path_refuses_a_non_finite_point_and_recovers(handle, tmp_path):
    """a NaN in the 65-point cluster refuses with its cluster's number from host and from device memory (the host loop before
    any launch, the pack kernel's flag word behind the CSR's wait); the next good call on the handle carries the mirror's bits"""
    import torch
    ix = handle
    mirror = U.Mirror(tmp_path)
    clusters = [U.cloud(n) for n in SIZES]
    want = [mirror(f"n{n}", p) for n, p in zip(SIZES, clusters)]
    assert [len(w) for w in want] == [1, 1, 1, 0]
    U.assert_distinct(want, "range batch")
    bad = [p.copy() for p in clusters]
    bad[1][40, 2] = np.nan
    ix.set_option(capi.OPT_VFH_BATCH_BRUTE_MAX, LIMIT)
    good_paths, bad_paths = _staging_paths(clusters), _staging_paths(bad)
    for what in good_paths:
        with pytest.raises(capi.PccError, match=r"non-finite.*cluster 1\)") as e:
            ix.vfh_descriptors_batch(*bad_paths[what])
        assert e.value.status == -5, what
        got = ix.vfh_descriptors_batch(*good_paths[what])
        torch.cuda.synchronize()
        stats = ix.stats()
        assert (int(stats[0]), int(stats[1]), int(stats[2])) == (68, 130, 3), what  # both routes ran
        assert len(got) == 4
        for k, (g, w) in enumerate(zip(got, want)):
            U.assert_same(g, w, f"{what}, after the refusal, cluster {k}")
