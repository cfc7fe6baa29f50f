"""Shared by tests/test_cluster_desc_cpu.py, tests/test_cluster_desc_gpu.py and tools/exp_descriptors.py: the clusters
pcc_cluster_descriptors is checked on, the reference for its bits -- the host mirrors build/sift_host and build/rift_host chained
per cluster by a NumPy restatement of the keypoint snap (src/comparator.cpp:696-713), independent of the library --, the
centroid arithmetic of the reference (:1235-1247), and a raw C-ABI call with sentinel-filled outputs for the refusal tests."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import rift_util
import sift_util
from pointcloudcomparator_amd import synth
from segment_util import _Raw

ROOT = Path(__file__).resolve().parent.parent
DRIVER = ROOT / "build" / "cluster_desc_driver"
EMPTY = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))
SIZE_MAX = 2 ** (8 * C.sizeof(C.c_size_t)) - 1


def scene(name):
    """(points (n, 3) float32, rgb (n, 3) uint8) of a named cluster; all of them lie near the origin and overlap"""
    if name == "empty":
        return EMPTY
    if name.startswith("rift"):  # "rift700": synth.rift_cloud(700, 7)
        return synth.rift_cloud(int(name[4:]), 7)
    return sift_util.scene(name)


def concat(names):
    """(points, rgb, offsets) of the named clusters one behind the other"""
    scenes = [scene(n) for n in names]
    pts = np.ascontiguousarray(np.concatenate([s[0] for s in scenes]))
    rgb = np.ascontiguousarray(np.concatenate([s[1] for s in scenes]))
    return pts, rgb, np.concatenate([[0], np.cumsum([len(s[0]) for s in scenes])]).astype(np.int64)


def records(pts, rgb):
    """32-byte pcl::PointXYZRGB records: x, y, z, 1, the colour word, padding"""
    rec = np.zeros((len(pts), 8), np.float32)
    rec[:, :3] = pts
    rec[:, 3] = 1.0
    rec.view(np.uint32)[:, 4] = synth.pack_rgb(rgb)
    return rec


def snap(points, keypoints, radius):
    """the reference's scan (:696-713) per keypoint: the lowest index whose distance -- differences in float, squares, sum
    and sqrt in double -- is < radius, or -1"""
    out = np.full(len(keypoints), -1, np.int32)
    p = np.ascontiguousarray(points[:, :3], np.float32)
    for k, q in enumerate(np.ascontiguousarray(keypoints[:, :3], np.float32)):
        d = (q[None, :] - p).astype(np.float32).astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            hit = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]) < radius
        if hit.any():
            out[k] = int(np.argmax(hit))
    return out


NO_DESCRIPTORS = (np.zeros((0, 32), np.float32), np.zeros(0, np.int32))


def mirror_chain(points, rgb, tmp, tag, sift_above=700, snap_radius=0.05):
    """what pcc_cluster_descriptors must return for one cluster, from the host mirrors: dict(hist (m, 32), index (m,) local to
    the cluster, n_keypoints, hits, distinct, misses)"""
    n = len(points)
    res = dict(hist=NO_DESCRIPTORS[0], index=NO_DESCRIPTORS[1], n_keypoints=0, hits=0, distinct=0, misses=0)
    if n == 0:
        return res
    if n <= sift_above:
        hist, index, _ = rift_util.run_tool(rift_util.HOST, points, rgb, tmp, tag=f"{tag}_dense")
        res.update(hist=hist, index=index)
        return res
    kp = sift_util.run_host(points, rgb, tmp, tag=f"{tag}_sift")["keypoints"]
    s = snap(points, kp, snap_radius)
    hit = s[s >= 0]
    res.update(n_keypoints=len(kp), hits=len(hit), distinct=len(np.unique(hit)), misses=int((s < 0).sum()))
    if len(hit) == 0:
        return res
    hist, j, _ = rift_util.run_tool(rift_util.HOST, np.ascontiguousarray(points[hit]), np.ascontiguousarray(rgb[hit]), tmp, tag=f"{tag}_snapped")
    res.update(hist=hist, index=hit[j].astype(np.int32))
    return res


def centroid(points):
    """the reference's loop (:1235-1247): three float accumulators from 0, += in index order, / float(n); empty: NaN"""
    p = np.ascontiguousarray(points[:, :3], np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if len(p) == 0:
            return np.float32(0) / np.zeros(3, np.float32)
        return np.cumsum(p, axis=0, dtype=np.float32)[-1] / np.float32(len(p))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_slice(res, c, want, what=""):
    """cluster c of a cluster_descriptors result carries `want` (a mirror_chain dict, or (hist, index)) bit for bit, in order"""
    hist, index = (want["hist"], want["index"]) if isinstance(want, dict) else want
    lo, hi = int(res["offsets"][c]), int(res["offsets"][c + 1])
    assert hi - lo == len(index), f"{what}: cluster {c} has {hi - lo} descriptors, expected {len(index)}"
    np.testing.assert_array_equal(res["point_index"][lo:hi], index, err_msg=f"{what}: cluster {c} point indices")
    differ = (bits(res["histograms"][lo:hi]) != bits(hist)).any(1) if hi > lo else np.zeros(0, bool)
    assert not differ.any(), f"{what}: cluster {c}: {int(differ.sum())} of {hi - lo} histograms differ in their bits"
    if isinstance(want, dict):
        assert int(res["n_keypoints"][c]) == want["n_keypoints"], f"{what}: cluster {c} keypoints"


def assert_same_result(got, want, what=""):
    np.testing.assert_array_equal(got["offsets"], want["offsets"], err_msg=f"{what}: offsets")
    np.testing.assert_array_equal(got["point_index"], want["point_index"], err_msg=f"{what}: point indices")
    np.testing.assert_array_equal(got["n_keypoints"], want["n_keypoints"], err_msg=f"{what}: keypoints")
    assert np.array_equal(bits(got["histograms"]), bits(want["histograms"])), f"{what}: histograms"
    assert np.array_equal(bits(got["centroids"]), bits(want["centroids"])), f"{what}: centroids"


def run_driver(pts, rgb, offsets, tmp, sift_above=700, tag="d", timeout=600):
    """build/cluster_desc_driver (pcc::clusterDescriptors) over clusters: the dict Index.cluster_descriptors returns"""
    fin, fout = Path(tmp) / f"{tag}.in", Path(tmp) / f"{tag}.out"
    n_clusters = len(offsets) - 1
    with open(fin, "wb") as f:
        f.write(np.int32(n_clusters).tobytes())
        for c in range(n_clusters):
            lo, hi = int(offsets[c]), int(offsets[c + 1])
            rec = np.zeros(hi - lo, dtype=[("p", "<f4", 3), ("c", "<u4")])
            rec["p"] = pts[lo:hi]
            rec["c"] = synth.pack_rgb(rgb[lo:hi])
            f.write(np.int32(hi - lo).tobytes())
            f.write(rec.tobytes())
    r = subprocess.run([str(DRIVER), str(fin), str(fout), str(int(sift_above))], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    raw = fout.read_bytes()
    at = 4
    assert int(np.frombuffer(raw[:4], np.int32)[0]) == n_clusters
    off = [0]
    hists, idxs, nkp, cent = [], [], [], []
    for _ in range(n_clusters):
        m, k = (int(v) for v in np.frombuffer(raw[at:at + 8], np.int32))
        at += 8
        cent.append(np.frombuffer(raw[at:at + 12], np.float32))
        at += 12
        hists.append(np.frombuffer(raw[at:at + m * 128], np.float32).reshape(m, 32))
        at += m * 128
        idxs.append(np.frombuffer(raw[at:at + m * 4], np.int32))
        at += m * 4
        nkp.append(k)
        off.append(off[-1] + m)
    assert at == len(raw)
    return dict(histograms=np.concatenate(hists) if hists else NO_DESCRIPTORS[0], point_index=np.concatenate(idxs) if idxs else NO_DESCRIPTORS[1],
                offsets=np.array(off, np.int64), n_keypoints=np.array(nkp, np.uint32), centroids=np.array(cent, np.float32).reshape(-1, 3))


class RawClusterDesc(_Raw):
    """pcc_cluster_descriptors through ctypes with every output filled with SENTINEL bytes"""

    def __init__(self, capacity=8, records=None, offsets=None):
        if records is None:  # eight points in two clusters
            records = np.zeros((8, 8), np.float32)
            records[:, :3] = np.arange(24, dtype=np.float32).reshape(8, 3) * 0.01
            offsets = [0, 3, 8]
        self.pts = np.ascontiguousarray(records, np.float32)
        self.offsets = np.array(offsets, np.uintp)
        self.n, self.n_clusters, self.capacity = len(self.pts), len(self.offsets) - 1, capacity
        n_clusters = self.n_clusters
        self.out = dict(hist=np.zeros((capacity, 32), np.float32), index=np.zeros(capacity, np.int32), out_offsets=np.zeros(n_clusters + 1, np.uintp),
                        nkp=np.zeros(n_clusters, np.uint32), cent=np.zeros((n_clusters, 3), np.float32))

    def __call__(self, handle, **kw):
        from pointcloudcomparator_amd import capi
        self._fill()
        a = dict(pts=self.pts.ctypes.data, stride=32, rgb=self.pts.ctypes.data + 16, rgb_stride=32, offsets=self.offsets.ctypes.data,
                 n_clusters=self.n_clusters, mem=0, sift_above=700, min_scale=0.005, octaves=5, scales=5, contrast=0.001, snap=0.05,
                 normal_r=0.03, gradient_r=0.03, rift_r=0.05, d_bins=4, g_bins=8, capacity=self.capacity,
                 **{k: v.ctypes.data for k, v in self.out.items()})
        a.update(kw)
        return capi.LIB.pcc_cluster_descriptors(
            handle, a["pts"], a["stride"], a["rgb"], a["rgb_stride"], a["offsets"], a["n_clusters"], a["mem"], a["sift_above"], a["min_scale"],
            a["octaves"], a["scales"], a["contrast"], a["snap"], a["normal_r"], a["gradient_r"], a["rift_r"], a["d_bins"], a["g_bins"], a["hist"],
            a["index"], a["capacity"], a["out_offsets"], a["nkp"], a["cent"])


def _offsets(*v):
    a = np.array(v, np.uintp)
    return a  # (kept alive by CLUSTER_DESC_REFUSALS)


_DECREASING = _offsets(0, 5, 3)
_HUGE = _offsets(0, 3, 2 ** 31)
# (keyword arguments, status, a piece of the message), in the documented order.  -1 PCC_ERR_INVALID, -5 PCC_ERR_UNSUPPORTED
CLUSTER_DESC_REFUSALS = [
    (dict(mem=7), -1, b"bad mem space"),                                  # 1. the memory space
    (dict(offsets=None), -1, b"null argument"),                           # 2. null arrays
    (dict(out_offsets=None), -1, b"null argument"),
    (dict(pts=None), -1, b"null argument"),
    (dict(rgb=None), -1, b"null argument"),
    (dict(hist=None), -1, b"null argument"),
    (dict(index=None), -1, b"null argument"),
    (dict(stride=10), -1, b"stride 10 must be a multiple of 4 and >= 12"),  # 3. strides and alignment
    (dict(stride=8), -1, b"stride 8"),
    (dict(rgb_stride=2), -1, b"4-byte aligned"),
    (dict(rgb_stride=6), -1, b"4-byte aligned"),
    (dict(offsets=_DECREASING.ctypes.data), -1, b"offsets must not decrease"),  # 4. the offsets
    (dict(offsets=_HUGE.ctypes.data), -5, b"2^31"),
    (dict(min_scale=0.0), -1, b"min_scale"),                              # 5. the SIFT parameters
    (dict(min_scale=float("nan")), -1, b"min_scale"),
    (dict(contrast=-1.0), -1, b"min_contrast"),
    (dict(octaves=0), -1, b"nr_octaves"),
    (dict(scales=0), -5, b"scales per octave"),
    (dict(normal_r=0.0), -1, b"bad radius"),                              # 6. the radii and bins
    (dict(gradient_r=float("nan")), -1, b"bad radius"),
    (dict(rift_r=-1.0), -1, b"bad radius"),
    (dict(d_bins=5), -5, b"bins"),
    (dict(g_bins=4), -5, b"bins"),
    (dict(snap=0.0), -1, b"bad radius"),                                  # 7. the snap radius
    (dict(snap=float("inf")), -1, b"bad radius"),
    (dict(snap=float("nan")), -1, b"bad radius"),
]
