"""pcc_cluster_descriptors without a GPU: the symbol, every refusal that happens before the handle is looked at (a NULL handle
comes last, so no device is needed) in the documented order, the Python wrapper's argument handling, the mirror chain's figures
the GPU tests rely on, and the host tables (tests/cpp/test_cluster_desc_plan.cpp), in the manner of
tests/test_euclid_segment_cpu.py."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import cluster_desc_util as cdu
from cluster_desc_util import CLUSTER_DESC_REFUSALS, RawClusterDesc

ROOT = Path(__file__).resolve().parent.parent


def test_symbol_is_exported():
    from pointcloudcomparator_amd import capi
    assert "pcc_cluster_descriptors" in capi.SYMBOLS and hasattr(capi.LIB, "pcc_cluster_descriptors")
    assert callable(capi.Index.cluster_descriptors)


@pytest.mark.parametrize("kw,status,message", CLUSTER_DESC_REFUSALS)
def test_refused_before_the_handle_is_looked_at(kw, status, message):
    from pointcloudcomparator_amd import capi
    call = RawClusterDesc()
    assert call(None, **kw) == status
    assert call.untouched()
    assert message in capi.LIB.pcc_last_error() and b"null index" not in capi.LIB.pcc_last_error()


def test_null_handle_is_refused_last():
    from pointcloudcomparator_amd import capi
    call = RawClusterDesc()
    assert call(None) == -1 and call.untouched()
    assert capi.LIB.pcc_last_error() == b"null index"
    # nothing else wrong, optional outputs left out, other layouts: still the handle
    assert call(None, nkp=None, cent=None) == -1
    assert call(None, capacity=0, hist=None, index=None) == -1          # (no room asked for: no arrays needed)
    assert call(None, sift_above=cdu.SIZE_MAX) == -1 and call(None, sift_above=0) == -1
    assert call(None, mem=1) == -1                                      # (device memory is taken)
    assert call(None, stride=12, rgb_stride=4) == -1
    empty = np.array([4, 4, 4], np.uintp)
    assert call(None, offsets=empty.ctypes.data, pts=None, rgb=None) == -1  # (no cluster holds a point: no arrays needed)
    assert capi.LIB.pcc_last_error() == b"null index" and call.untouched()


def test_no_clusters_is_ok_without_a_handle_or_a_device():
    call = RawClusterDesc()
    none = np.array([5], np.uintp)
    assert call(None, n_clusters=0, offsets=none.ctypes.data) == 0
    assert call.out["out_offsets"][0] == 0
    others = [v for k, v in call.out.items() if k != "out_offsets"]
    assert all((v.view(np.uint8) == 0x5A).all() for v in others) and (call.out["out_offsets"][1:].view(np.uint8) == 0x5A).all()
    # ... but a fault in front of it is still a fault
    assert call(None, n_clusters=0, offsets=none.ctypes.data, snap=0.0) == -1


def test_two_faults_resolve_in_the_documented_order():
    from pointcloudcomparator_amd import capi
    call = RawClusterDesc()
    err = capi.LIB.pcc_last_error
    decreasing, huge = np.array([0, 5, 3], np.uintp), np.array([0, 3, 2 ** 31], np.uintp)
    # 1 the memory space, 2 null arrays, 3 strides, 4 offsets, 5 SIFT parameters, 6 radii and bins, 7 the snap radius
    assert call(None, mem=7, offsets=None) == -1 and b"bad mem space" in err()
    assert call(None, pts=None, stride=10) == -1 and b"null argument" in err()
    assert call(None, stride=10, offsets=decreasing.ctypes.data) == -1 and b"stride 10" in err()
    assert call(None, rgb_stride=6, offsets=huge.ctypes.data) == -1 and b"4-byte aligned" in err()
    assert call(None, offsets=decreasing.ctypes.data, min_scale=0.0) == -1 and b"must not decrease" in err()
    assert call(None, offsets=huge.ctypes.data, octaves=0) == -5 and b"2^31" in err()
    assert call(None, scales=0, rift_r=0.0) == -5 and b"scales per octave" in err()
    assert call(None, contrast=-1.0, d_bins=5) == -1 and b"min_contrast" in err()
    assert call(None, d_bins=5, snap=0.0) == -5 and b"bins" in err()
    assert call(None, normal_r=-1.0, snap=float("nan")) == -1 and b"bad radius" in err()
    assert call(None, snap=-0.05) == -1 and b"bad radius" in err()
    assert call.untouched()


def test_python_wrapper_argument_handling():
    from pointcloudcomparator_amd import capi
    ix = capi.Index.__new__(capi.Index)  # (no handle: the checks below come first)
    ix._h, ix.auto_sync = None, True
    rec = np.zeros((8, 8), np.float32)
    xyz = np.zeros((8, 3), np.float32)
    with pytest.raises(AssertionError):
        ix.cluster_descriptors(rec.astype(np.float64), None, [0, 8])
    with pytest.raises(AssertionError, match="column 4"):
        ix.cluster_descriptors(xyz, None, [0, 8])
    with pytest.raises(AssertionError, match="one colour per point"):
        ix.cluster_descriptors(xyz, np.zeros((7, 3), np.uint8), [0, 8])
    with pytest.raises(AssertionError, match="offsets"):
        ix.cluster_descriptors(rec, None, None)
    with pytest.raises(AssertionError, match="beyond"):
        ix.cluster_descriptors(rec, None, [0, 9])
    with pytest.raises(AssertionError, match="sift_above"):
        ix.cluster_descriptors(rec, None, [0, 8], sift_above=-1)
    with pytest.raises(capi.PccError) as e:
        ix.cluster_descriptors(rec, None, [0, 5, 3])
    assert e.value.status == -1 and "must not decrease" in str(e.value)
    with pytest.raises(capi.PccError) as e:
        ix.cluster_descriptors(xyz, np.zeros((8, 3), np.uint8), [0, 8], snap_radius=0.0)
    assert e.value.status == -1 and "bad radius" in str(e.value)
    with pytest.raises(capi.PccError) as e:
        ix.cluster_descriptors(rec, None, [0, 8], nr_distance_bins=5)
    assert e.value.status == -5
    for kw in (dict(), dict(sift_above=None), dict(capacity=0)):
        with pytest.raises(capi.PccError) as e:  # all arguments good: the NULL handle
            ix.cluster_descriptors(rec, None, [0, 3, 8], **kw)
        assert e.value.status == -1 and "null index" in str(e.value)
    res = ix.cluster_descriptors(rec, None, [0])  # no clusters: no handle needed
    assert res["offsets"].tolist() == [0] and len(res["histograms"]) == 0 and res["centroids"].shape == (0, 3)
    ix._h = None  # (nothing for __del__ to destroy)


# (scene, snap radius) -> keypoints, hits, distinct snapped points, misses, descriptors: the figures of the mirror chain
CHAIN_FIGURES = [
    ("sift2000", 0.05, (196, 196, 48, 0, 136)),
    ("rift701", 0.05, (75, 75, 16, 0, 61)),
    ("sift2000", 0.004, (196, 180, 158, 16, 41)),
    ("rift701", 0.004, (75, 69, 63, 6, 10)),
    ("tiny25", 0.05, (0, 0, 0, 0, 0)),
]


@pytest.mark.parametrize("name,radius,figures", CHAIN_FIGURES)
def test_the_mirror_chain_has_the_figures_the_gpu_tests_rely_on(tmp_path, name, radius, figures):
    assert cdu.sift_util.HOST.exists() and cdu.rift_util.HOST.exists(), "build/sift_host and build/rift_host: run `make hosttest`"
    pts, rgb = cdu.scene(name)
    m = cdu.mirror_chain(pts, rgb, tmp_path, name, sift_above=10, snap_radius=radius)
    assert (m["n_keypoints"], m["hits"], m["distinct"], m["misses"], len(m["index"])) == figures
    assert len(m["hist"]) == len(m["index"]) and (len(m["index"]) == 0 or (0 <= m["index"].min() and m["index"].max() < len(pts)))


def test_centroid_inputs_tell_the_orders_apart():
    """the 2000-point cluster of the GPU centroid test: the sequential float sum differs from the double sum rounded once in
    all three coordinates, and from a 64-wide tree sum in at least one"""
    pts = cdu.scene("rift2000")[0] + np.float32(3.0)
    seq = cdu.centroid(pts)
    once = (pts.astype(np.float64).sum(0)).astype(np.float32) / np.float32(len(pts))
    assert (cdu.bits(seq) != cdu.bits(once)).all()
    tree = np.zeros(3, np.float32)
    for t0 in range(0, len(pts), 64):  # a wave's tree over 64 lanes per tile, tiles in order
        lanes = np.zeros((64, 3), np.float32)
        lanes[:len(pts[t0:t0 + 64])] = pts[t0:t0 + 64]
        w = 32
        while w:
            lanes[:w] = lanes[:w] + lanes[w:2 * w]
            w //= 2
        tree = tree + lanes[0]
    assert (cdu.bits(seq) != cdu.bits(tree / np.float32(len(pts)))).any()


def test_host_tables():
    exe = ROOT / "build" / "test_cluster_desc_plan"
    assert exe.exists(), "build/test_cluster_desc_plan: run `make hosttest`"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
