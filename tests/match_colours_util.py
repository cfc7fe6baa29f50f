"""Shared by tests/test_match_colours_cpu.py, tests/test_match_colours_gpu.py and tools/exp_match_colours.py: the restatement of
the counting of the reference's match loop (src/comparator.cpp:1379-1509: color_growing_segmentation on both clusters of every
accepted match, of which the two segment counts are kept) in Python, independent of the library; the record layout
pcc_match_colour_elements takes; the scenes of the GPU tests; and a raw C-ABI call with a sentinel-filled output for the refusal
tests."""
import numpy as np

from segment_util import _Raw

RB_TILE = 2048  # csrc/rift_batch_plan.hpp: points of a cloud a workgroup holds in LDS at a time


def finite_points(pts):
    return int(np.isfinite(np.asarray(pts, np.float32).reshape(-1, 3)).all(1).sum())


def restate(clusters1, clusters2, matches, count_of, min_points=10):
    """The (n_clusters1, 2) table of the match loop.  clusters_s: one (points, colours) per cluster; count_of(points, colours):
    the colour segments of ONE cluster that passed the gate.  The gate (more than min_points finite points, src/segmentation.cpp:
    164-167) is applied here, every distinct (scene, cluster) is counted once, and the count is handed to every row that names it.
    Returns (table, distinct clusters counted or gated, segmentations saved)."""
    out = np.full((len(matches), 2), -1, np.int32)
    seen = {}
    saved = 0
    for i, j in enumerate(matches):
        if j < 0:
            continue
        for side, c in ((0, i), (1, int(j))):
            if (side, c) in seen:
                saved += 1
            else:
                pts, rgb = (clusters2 if side else clusters1)[c]
                seen[(side, c)] = int(count_of(pts, rgb)) if finite_points(pts) > min_points else 0
            out[i, side] = seen[(side, c)]
    return out, len(seen), saved


def words(rgb):
    """PCL's packed colour word (bytes b, g, r, a from the low byte) of (n, 3) uint8 r, g, b"""
    c = np.asarray(rgb).astype(np.uint32).reshape(-1, 3)
    return np.ascontiguousarray(c[:, 2] | (c[:, 1] << 8) | (c[:, 0] << 16))


def records(clusters):
    """the clusters of a scene as the segmentation calls write them: ((n, 8) float32 pcl::PointXYZRGB records -- x, y, z, 1, the
    colour word, padding --, offsets (n_clusters + 1,))"""
    n = [len(p) for p, _ in clusters]
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    rec = np.zeros((int(off[-1]), 8), np.float32)
    for k, (p, c) in enumerate(clusters):
        rec[off[k]:off[k + 1], :3] = p
        rec[off[k]:off[k + 1], 3] = 1.0
        rec[off[k]:off[k + 1], 4] = words(c).view(np.float32)
    return rec, off


def separate(clusters):
    """the same clusters as 16-byte points and 4-byte colour words of their own: ((n, 4) float32, (n,) uint32, offsets)"""
    rec, off = records(clusters)
    return np.ascontiguousarray(rec[:, :4]), np.ascontiguousarray(rec[:, 4]).view(np.uint32), off


def two_level_cloud(rng, n):
    """n points in a cube of 0.3 with one of 27 colours 20 levels apart each: segments of all sizes"""
    return rng.random((n, 3)).astype(np.float32) * np.float32(0.3), (rng.integers(0, 3, (n, 3)) * 20).astype(np.uint8)


def mixed_scenes(fix, room):
    """two scenes of six clusters each, cut from rgb_device_util.fixpoint_scenes() (fix: name -> (points, colours)) and the painted
    room of test_rgb_gpu._scenes() (room: (points, colours)), at most 3000 points a cluster, and a match table with two rows
    without a match"""
    cut = lambda name, lo, hi: (np.ascontiguousarray(fix[name][0][lo:hi]), np.ascontiguousarray(fix[name][1][lo:hi]))
    rcut = lambda lo, hi: (np.ascontiguousarray(room[0][lo:hi]), np.ascontiguousarray(room[1][lo:hi]))
    scene1 = [cut("patches", 0, 3000), cut("near", 0, 1500), cut("noise", 500, 1700), cut("tiny", 0, 20), cut("cascade", 0, 10 ** 6), rcut(0, 3000)]
    scene2 = [rcut(3000, 6000), cut("patches", 1000, 2500), cut("cascade_rev", 0, 10 ** 6), cut("near", 1500, 3000), cut("noise", 0, 900),
              rcut(10000, 12500)]
    return scene1, scene2, np.array([2, -1, 4, 3, -1, 0], np.int32)


def size_scenes(seed=31):
    """clusters of 11, 12, 63, 64, 65, 255, 256, 257, RB_TILE - 1, RB_TILE and RB_TILE + 1 points over two scenes of seven and six
    clusters, an empty cluster between two others in each, and a table that names every cluster (cluster 5 of scene 2 twice)"""
    rng = np.random.default_rng(seed)
    scene1 = [two_level_cloud(rng, n) for n in (11, 63, 0, 65, 256, RB_TILE - 1, RB_TILE + 1)]
    scene2 = [two_level_cloud(rng, n) for n in (12, 64, 255, 0, 257, RB_TILE)]
    return scene1, scene2, np.array([0, 1, 3, 2, 4, 5, 5], np.int32)


class RawMatchColours(_Raw):
    """pcc_match_colour_elements through ctypes with the output filled with SENTINEL bytes.  The default scene: two clusters of
    five records against three, both rows matched."""

    def __init__(self):
        rng = np.random.default_rng(6)
        self.rec1 = rng.random((10, 8), dtype=np.float32)
        self.rec2 = rng.random((15, 8), dtype=np.float32)
        self.offsets1 = np.array([0, 5, 10], np.uintp)
        self.offsets2 = np.array([0, 5, 10, 15], np.uintp)
        self.matches = np.array([2, 0], np.int32)
        self.out = dict(elements=np.zeros((2, 2), np.int32))

    def __call__(self, handle, **kw):
        from pointcloudcomparator_amd import capi
        self._fill()
        a = dict(pts1=self.rec1.ctypes.data, rgb1=self.rec1.ctypes.data + 16, offsets1=self.offsets1.ctypes.data, n_clusters1=2,
                 pts2=self.rec2.ctypes.data, rgb2=self.rec2.ctypes.data + 16, offsets2=self.offsets2.ctypes.data, n_clusters2=3, stride=32,
                 rgb_stride=32, mem=0, matches=self.matches.ctypes.data, min_points=10, distance=10.0, point_colour=6.0, region_colour=5.0,
                 min_size=200, max_size=2 ** 31 - 1, nn=30, region_nn=100, elements=self.out["elements"].ctypes.data)
        a.update(kw)
        return capi.LIB.pcc_match_colour_elements(
            handle, a["pts1"], a["rgb1"], a["offsets1"], a["n_clusters1"], a["pts2"], a["rgb2"], a["offsets2"], a["n_clusters2"], a["stride"],
            a["rgb_stride"], a["mem"], a["matches"], a["min_points"], a["distance"], a["point_colour"], a["region_colour"], a["min_size"],
            a["max_size"], a["nn"], a["region_nn"], a["elements"])


def _array(dtype, *v):
    return np.array(v, dtype)  # (kept alive by the module)


DECREASING = _array(np.uintp, 0, 7, 5)
DECREASING2 = _array(np.uintp, 0, 5, 3, 15)
HUGE = _array(np.uintp, 0, 5, 2 ** 31)
HUGE2 = _array(np.uintp, 0, 5, 10, 2 ** 31)
BAD_MATCH_HIGH = _array(np.int32, 2, 3)
BAD_MATCH_LOW = _array(np.int32, -2, 0)
NO_MATCH = _array(np.int32, -1, -1)
# (keyword arguments, status, a piece of the message), in the documented order.  -1 PCC_ERR_INVALID, -5 PCC_ERR_UNSUPPORTED
MATCH_COLOURS_REFUSALS = [
    (dict(mem=7), -1, b"bad mem space"),                                      # 1. the memory space
    (dict(mem=-1), -1, b"bad mem space"),
    (dict(offsets1=None), -1, b"null argument"),                              # 2. null arrays
    (dict(offsets2=None), -1, b"null argument"),
    (dict(matches=None), -1, b"null argument"),
    (dict(elements=None), -1, b"null argument"),
    (dict(pts1=None), -1, b"null argument"),
    (dict(rgb1=None), -1, b"null argument"),
    (dict(pts2=None), -1, b"null argument"),
    (dict(rgb2=None), -1, b"null argument"),
    (dict(stride=10), -1, b"stride 10 must be a multiple of 4 and >= 12"),    # 3. the strides and the alignment
    (dict(stride=8), -1, b"stride 8"),
    (dict(rgb_stride=2), -1, b"colour words must be 4-byte aligned, stride 2"),
    (dict(rgb_stride=6), -1, b"colour words must be 4-byte aligned, stride 6"),
    (dict(rgb_stride=0), -1, b"colour words must be 4-byte aligned, stride 0"),
    (dict(pts1=2), -1, b"points and colour words must be 4-byte aligned"),
    (dict(rgb2=6), -1, b"points and colour words must be 4-byte aligned"),
    (dict(offsets1=DECREASING.ctypes.data), -1, b"offsets must not decrease"),   # 4. the offsets
    (dict(offsets2=DECREASING2.ctypes.data), -1, b"offsets must not decrease"),
    (dict(offsets1=HUGE.ctypes.data), -5, b"2^31"),
    (dict(offsets2=HUGE2.ctypes.data), -5, b"2^31"),
    (dict(matches=BAD_MATCH_HIGH.ctypes.data), -1, b"matches[1] = 3"),        # 5. the match table
    (dict(matches=BAD_MATCH_LOW.ctypes.data), -1, b"matches[0] = -2"),
    (dict(distance=-1.0), -1, b"bad threshold"),                              # 6. the parameters
    (dict(point_colour=float("nan")), -1, b"bad threshold"),
    (dict(region_colour=float("inf")), -1, b"bad threshold"),
    (dict(nn=0), -5, b"neighbours"),
    (dict(region_nn=0), -5, b"neighbours"),
    (dict(region_nn=10 ** 6), -5, b"neighbours"),
]
