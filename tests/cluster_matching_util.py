"""Shared by tests/test_cluster_matching_cpu.py, tests/test_cluster_matching_gpu.py and tools/exp_cluster_matching.py: the
restatement of the reference's cluster-matching loop (src/comparator.cpp:1296-1366) in Python, independent of the library --
candidates, gates, correspondence counts by a float32 NumPy brute force in index order, acceptance --, the recorded per-cluster
tables (tests/golden/cluster_tables.json) as inputs of pcc_cluster_matching, and a raw C-ABI call with sentinel-filled outputs
for the refusal tests."""
import functools
import json
from pathlib import Path

import numpy as np

import match_dims_util as mdu
from pointcloudcomparator_amd import synth
from segment_util import _Raw

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden" / "cluster_tables.json"
NONE, GATED_COUNTS, GATED_SIZE, SEARCHED = 0, 1, 2, 3


def nearest_free(c, others, taken):
    """nearestFreeCentroid of host/report.hpp: float differences, squares and their sum in double, the sum rounded to float, a
    float square root, strict < against 1e12f; the lowest index among equal distances; -1 when nothing qualifies"""
    arg, best = -1, np.float32(1000000000000.0)
    with np.errstate(all="ignore"):
        for j, o in enumerate(others):
            if j in taken:
                continue
            d2 = np.float32(sum(float(np.float32(c[a]) - np.float32(o[a])) ** 2 for a in range(3)))
            d = np.sqrt(d2, dtype=np.float32)
            if d < best:
                best, arg = d, j
    return arg


def candidates(centroids1, centroids2):
    out = np.full((len(centroids1), 3), -1, np.int32)
    for i, c in enumerate(centroids1):
        taken = set()
        for k in range(3):
            out[i, k] = nearest_free(c, centroids2, taken)
            if k < 2:
                taken.add(int(out[i, k]))
    return out


def states(cand, n1, n2, points1, points2):
    """n1 / n2: the descriptor counts per cluster"""
    out = np.zeros(cand.shape, np.int32)
    for i in range(len(cand)):
        for k in range(3):
            j = int(cand[i, k])
            if j < 0:
                out[i, k] = NONE
            elif n1[i] <= 3 or n2[j] <= 3:
                out[i, k] = GATED_COUNTS
            elif int(points1[i]) == 0 or int(points2[j]) // int(points1[i]) != 1:
                out[i, k] = GATED_SIZE
            else:
                out[i, k] = SEARCHED
    return out


def count(a, b, dim, threshold):
    """1 + the valid records of b whose smallest L2_Simple distance (float32, index order) to a valid record of a is a neighbour
    and < threshold: len(row) of match_dims_util.restate, without the indices"""
    if len(a) == 0 or len(b) == 0:
        return 1
    total = 1
    valid_a = np.isfinite(a[:, :dim]).all(1)
    for q0 in range(0, len(b), 512):  # (blocks of queries: the distance matrix stays small)
        q = np.ascontiguousarray(b[q0:q0 + 512])
        d = mdu.d2_chain(np.ascontiguousarray(a), q, dim)
        d[:, ~valid_a] = np.inf
        d[~np.isfinite(q[:, :dim]).all(1), :] = np.inf
        d[~(d < mdu.F32_MAX)] = np.inf
        best = d.min(1)
        total += int(((best < mdu.F32_MAX) & (best < np.float32(threshold))).sum())
    return total


def accept(cand, state, corr, n1, n2):
    matches = np.full(len(cand), -1, np.int32)
    for i in range(len(cand)):
        best = 0
        for k in range(3):
            if state[i, k] != SEARCHED:
                continue
            j = int(cand[i, k])
            c, denom = int(corr[i, k]), max(int(n1[i]), int(n2[j]))
            if c // denom >= 1 and c > best:
                best, matches[i] = c, j
    return matches


def restate(des1, offsets1, des2, offsets2, centroids1, centroids2, points1, points2, threshold=0.05, dim=3, counts=True):
    """the dict Index.cluster_matching returns (counts=False: correspondences and matches left out)"""
    o1, o2 = np.asarray(offsets1, np.int64), np.asarray(offsets2, np.int64)
    n1, n2 = np.diff(o1), np.diff(o2)
    cand = candidates(np.asarray(centroids1, np.float32).reshape(-1, 3), np.asarray(centroids2, np.float32).reshape(-1, 3))
    state = states(cand, n1, n2, points1, points2)
    res = dict(candidates=cand, state=state)
    if not counts:
        return res
    corr = np.zeros(cand.shape, np.uint32)
    for i, k in zip(*np.nonzero(state == SEARCHED)):
        j = int(cand[i, k])
        corr[i, k] = count(des1[o1[i]:o1[i + 1]], des2[o2[j]:o2[j + 1]], dim, threshold)
    res.update(correspondences=corr, matches=accept(cand, state, corr, n1, n2))
    return res


def assert_same(got, want, what=""):
    for key in ("candidates", "state", "correspondences", "matches"):
        np.testing.assert_array_equal(np.asarray(got[key]).astype(np.int64), np.asarray(want[key]).astype(np.int64), err_msg=f"{what}: {key}")


def runs():
    return json.loads(GOLDEN.read_text())["runs"]


@functools.lru_cache(maxsize=None)
def run_tables(name):
    """(offsets1, offsets2, centroids1, centroids2, points1, points2) of a recorded run"""
    r = runs()[name]
    out = []
    for key in ("clusters1", "clusters2"):
        rows = r[key]
        out.append((np.concatenate([[0], np.cumsum([n for _, n, _ in rows])]).astype(np.int64),
                    np.array([c for _, _, c in rows], np.float32).reshape(-1, 3), np.array([p for p, _, _ in rows], np.int64)))
    (o1, c1, p1), (o2, c2, p2) = out
    return o1, o2, c1, c2, p1, p2


@functools.lru_cache(maxsize=None)
def run_descriptors(name, family, seed=7):
    """(des1, des2), (n, 32) float32 each, for the recorded descriptor counts of a run: every cluster of scene 1 drawn from the
    family; a cluster of scene 2 made of perturbed records of the first scene-1 cluster it is a candidate of (matches on both
    sides of the threshold), else drawn"""
    o1, o2, c1, c2, p1, p2 = run_tables(name)
    n1, n2 = np.diff(o1), np.diff(o2)
    cand = candidates(c1, c2)
    parts1 = [synth.descriptor_cloud(int(n), family, seed * 100003 + 2 * i) for i, n in enumerate(n1)]
    source = {}
    for i in range(len(cand)):
        for j in cand[i]:
            if j >= 0 and n1[i] > 0:
                source.setdefault(int(j), i)
    parts2 = [synth.descriptor_queries(parts1[source[j]], int(n), family, seed * 100003 + 2 * j + 1) if j in source
              else synth.descriptor_cloud(int(n), family, seed * 100003 + 2 * j + 1) for j, n in enumerate(n2)]
    cat = lambda parts: np.ascontiguousarray(np.concatenate(parts + [np.zeros((0, 32), np.float32)]))
    return cat(parts1), cat(parts2)


class RawClusterMatching(_Raw):
    """pcc_cluster_matching through ctypes with every output filled with SENTINEL bytes.  The default scene: two clusters of
    five descriptors against three; cluster 0 of scene 1 has a searched pair."""

    def __init__(self):
        rng = np.random.default_rng(5)
        self.des1 = rng.random((10, 32), dtype=np.float32)
        self.des2 = rng.random((15, 32), dtype=np.float32)
        self.offsets1 = np.array([0, 5, 10], np.uintp)
        self.offsets2 = np.array([0, 5, 10, 15], np.uintp)
        self.centroids1 = np.array([[0, 0, 0], [5, 0, 0]], np.float32)
        self.centroids2 = np.array([[0.1, 0, 0], [5.1, 0, 0], [9, 0, 0]], np.float32)
        self.points1 = np.array([100, 100], np.uintp)
        self.points2 = np.array([150, 120, 100], np.uintp)
        self.out = dict(candidates=np.zeros((2, 3), np.int32), state=np.zeros((2, 3), np.int32), correspondences=np.zeros((2, 3), np.uint32),
                        matches=np.zeros(2, np.int32))

    def __call__(self, handle, **kw):
        from pointcloudcomparator_amd import capi
        self._fill()
        a = dict(des1=self.des1.ctypes.data, offsets1=self.offsets1.ctypes.data, n_clusters1=2, des2=self.des2.ctypes.data,
                 offsets2=self.offsets2.ctypes.data, n_clusters2=3, stride=128, dim=3, mem=0, centroids1=self.centroids1.ctypes.data,
                 centroids2=self.centroids2.ctypes.data, points1=self.points1.ctypes.data, points2=self.points2.ctypes.data, threshold=0.05,
                 **{k: v.ctypes.data for k, v in self.out.items()})
        a.update(kw)
        return capi.LIB.pcc_cluster_matching(
            handle, a["des1"], a["offsets1"], a["n_clusters1"], a["des2"], a["offsets2"], a["n_clusters2"], a["stride"], a["dim"], a["mem"],
            a["centroids1"], a["centroids2"], a["points1"], a["points2"], a["threshold"], a["candidates"], a["state"], a["correspondences"],
            a["matches"])


def _offsets(*v):
    return np.array(v, np.uintp)  # (kept alive by CLUSTER_MATCHING_REFUSALS)


_DECREASING = _offsets(0, 7, 5)
_DECREASING2 = _offsets(0, 5, 3, 15)
_HUGE = _offsets(0, 5, 2 ** 31)
_HUGE2 = _offsets(0, 5, 10, 2 ** 31)
# (keyword arguments, status, a piece of the message), in the documented order.  -1 PCC_ERR_INVALID, -5 PCC_ERR_UNSUPPORTED
CLUSTER_MATCHING_REFUSALS = [
    (dict(dim=0), -5, b"1 ... 32 dimensions"),                                # 1. the width
    (dict(dim=33), -5, b"1 ... 32 dimensions"),
    (dict(dim=-3), -5, b"1 ... 32 dimensions"),
    (dict(mem=7), -1, b"bad mem space"),                                      # 2. the memory space
    (dict(offsets1=None), -1, b"null argument"),                              # 3. null arrays
    (dict(offsets2=None), -1, b"null argument"),
    (dict(centroids1=None), -1, b"null argument"),
    (dict(centroids2=None), -1, b"null argument"),
    (dict(points1=None), -1, b"null argument"),
    (dict(points2=None), -1, b"null argument"),
    (dict(des1=None), -1, b"null argument"),
    (dict(des2=None), -1, b"null argument"),
    (dict(candidates=None), -1, b"null argument"),
    (dict(state=None), -1, b"null argument"),
    (dict(correspondences=None), -1, b"null argument"),
    (dict(matches=None), -1, b"null argument"),
    (dict(stride=10), -1, b"stride 10 must be a multiple of 4 and >= 12"),    # 4. the stride and the alignment
    (dict(stride=8), -1, b"stride 8"),
    (dict(stride=124, dim=32), -1, b"stride 124 must be a multiple of 4 and >= 128"),
    (dict(des1=2), -1, b"4-byte aligned"),
    (dict(des2=6), -1, b"4-byte aligned"),
    (dict(offsets1=_DECREASING.ctypes.data), -1, b"offsets must not decrease"),  # 5. the offsets
    (dict(offsets2=_DECREASING2.ctypes.data), -1, b"offsets must not decrease"),
    (dict(offsets1=_HUGE.ctypes.data), -5, b"2^31"),
    (dict(offsets2=_HUGE2.ctypes.data), -5, b"2^31"),
]
