"""pcc_cluster_matching on the GPU, bit-exact against the Python restatement of the reference's cluster-matching loop
(tests/cluster_matching_util.py: candidates, gates, float32 brute-force counts in index order, acceptance) and, per searched
pair, against the length of the row Index.match_knn_batch returns.

Shapes: the padded widths' edges (dim 1, 3, 4, 5, 17, 32), query counts around the 64-query block (4, 63, 64, 65, 129),
reference counts around the 16-wave share and the 256-reference slice (4, 255, 256, 257, 513), a scene-2 cluster shared by three
scene-1 clusters, invalid records on either side, the threshold and overflow edges, duplicated references under both tie orders,
the acceptance and candidate edges, the size gate, host / device / strided descriptors, the two recorded workloads."""
import sys
from pathlib import Path

import numpy as np
import pytest

from pointcloudcomparator_amd import capi, synth

sys.path.insert(0, str(Path(__file__).resolve().parent))
import cluster_matching_util as cmu  # noqa: E402
import match_dims_util as mdu  # noqa: E402

pytestmark = pytest.mark.gpu

DIMS = (1, 3, 4, 5, 17, 32)
N_QUERIES = (4, 63, 64, 65, 129)
N_REFERENCES = (4, 255, 256, 257, 513)


@pytest.fixture(scope="module")
def ix(gpu):
    with capi.Index(np.zeros((4, 32), np.float32), auto_sync=False) as h:
        yield h


def cat(parts):
    return np.ascontiguousarray(np.concatenate(list(parts) + [np.zeros((0, 32), np.float32)]))


def offsets_of(parts):
    return np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)


def line(n, step=10.0):
    """n centroids on the x axis, `step` apart"""
    c = np.zeros((n, 3), np.float32)
    c[:, 0] = np.arange(n, dtype=np.float32) * np.float32(step)
    return c


def run(ix, parts1, parts2, centroids1, centroids2, points1=None, points2=None, threshold=0.05, dim=3, what=""):
    """the call on per-cluster descriptor arrays, held against the restatement; returns the call's dict"""
    points1 = [100] * len(parts1) if points1 is None else points1
    points2 = [100] * len(parts2) if points2 is None else points2
    args = (cat(parts1), offsets_of(parts1), cat(parts2), offsets_of(parts2), centroids1, centroids2, points1, points2)
    got = ix.cluster_matching(*args, threshold=threshold, dim=dim)
    cmu.assert_same(got, cmu.restate(*args, threshold=threshold, dim=dim), what)
    assert got["candidates"].dtype == np.int32 and got["correspondences"].dtype == np.uint32
    return got


@pytest.fixture(scope="module")
def grid_scene():
    """25 clusters a scene: scene-1 cluster (r, q) holds N_REFERENCES[r] records and lies where scene-2 cluster (r, q) with
    N_QUERIES[q] records lies; its other two candidates are the neighbours on the line.  Queries are perturbed records of the
    partner: distances on both sides of a threshold of 0.0075 a bin."""
    parts1, parts2 = [], []
    for r, nr in enumerate(N_REFERENCES):
        for q, nq in enumerate(N_QUERIES):
            a = synth.descriptor_cloud(nr, "uniform", 100 + 5 * r + q)
            parts1.append(a)
            parts2.append(synth.descriptor_queries(a, nq, "uniform", 200 + 5 * r + q))
    return parts1, parts2


@pytest.mark.parametrize("dim", DIMS)
def test_widths_query_counts_and_reference_counts(ix, grid_scene, dim):
    parts1, parts2 = grid_scene
    got = run(ix, parts1, parts2, line(25), line(25), threshold=0.0075 * dim, dim=dim, what=f"dim {dim}")
    assert (got["state"] == cmu.SEARCHED).sum() == 75  # (every cluster has three candidates, every pair passes the gates)
    nq = np.array([len(p) for p in parts2])
    corr, cand = got["correspondences"], got["candidates"]
    partial = [(i, k) for i in range(25) for k in range(3) if cand[i, k] >= 0 and 1 < corr[i, k] < nq[cand[i, k]] + 1]
    assert partial, "no pair with some queries below the threshold and some above: the counts pin nothing"
    stats = ix.stats()
    assert stats[0] == 75 and stats[1] == int(sum(nq[cand[i, k]] for i, k in zip(*np.nonzero(got["state"] == cmu.SEARCHED))))


def test_one_cluster_is_the_candidate_of_three(ix):
    shared = synth.descriptor_cloud(65, "quantised", 31)
    parts1 = [synth.descriptor_queries(shared, n, "quantised", 40 + n) for n in (4, 130, 257)]
    got = run(ix, parts1, [shared], line(3, 1.0), line(1), what="shared")
    assert got["candidates"].tolist() == [[0, -1, -1]] * 3 and got["state"].tolist() == [[3, 0, 0]] * 3
    assert ix.stats()[:2] == [3, 3 * 65]


@pytest.mark.parametrize("dim", (3, 5, 32))
def test_invalid_records(ix, dim):
    rng = np.random.default_rng(dim)
    a = rng.random((300, 32), dtype=np.float32)
    b = np.ascontiguousarray(a[:70] + np.float32(0.01))
    a[3, 0], a[17, dim - 1], a[280, dim // 2] = np.nan, np.inf, -np.inf       # invalid references, one in the second slice
    b[0, dim - 1], b[64, 0], b[69, dim // 2] = np.nan, np.inf, np.nan         # invalid queries, in both query blocks
    if dim < 32:
        a[5, dim], b[5, dim], a[6, 31], b[7, 31] = np.nan, np.nan, np.inf, np.nan  # beyond dim: ignored
    dead = np.full((8, 32), np.nan, np.float32)
    dead[:, 1:] = 0.5
    parts1 = [a, dead, a]
    parts2 = [b, b, dead]
    # cluster 0 against b, the all-invalid reference cluster against b, a against the all-invalid query cluster
    c1 = np.array([[0, 0, 0], [100, 0, 0], [200, 0, 0]], np.float32)
    c2 = np.array([[0, 0, 0], [100, 0, 0], [200, 0, 0]], np.float32)
    got = run(ix, parts1, parts2, c1, c2, threshold=0.01 * dim, dim=dim, what=f"invalid records, dim {dim}")
    corr = got["correspondences"]
    assert got["candidates"][:, 0].tolist() == [0, 1, 2] and (got["state"] == cmu.SEARCHED).all()
    assert corr[1, 0] == 1 and corr[2, 0] == 1                                  # no valid reference; no valid query
    assert 1 + 70 - 3 - 2 <= corr[0, 0] <= 1 + 70 - 3                           # 3 invalid queries; 2 valid ones lost their source
    assert (corr[1] == 1).all() and corr[2, 2] > 1


def test_a_distance_equal_to_the_threshold_is_not_counted(ix):
    a = np.zeros((6, 32), np.float32)
    b = np.zeros((5, 32), np.float32)
    b[:, 0] = 0.5
    for threshold, want in ((0.25, 1), (float(np.nextafter(np.float32(0.25), np.float32(1))), 6), (float("inf"), 6), (float("nan"), 1), (0.0, 1)):
        got = run(ix, [a], [b], line(1), line(1), threshold=threshold, dim=1, what=f"threshold {threshold}")
        assert got["correspondences"][0, 0] == want
    assert run(ix, [a], [a[:5]], line(1), line(1), threshold=0.0, dim=1)["correspondences"][0, 0] == 1  # (0 < 0 is false)


def test_an_overflowing_distance_is_no_neighbour(ix):
    a = np.full((6, 32), 3e38, np.float32)
    b = np.full((5, 32), -3e38, np.float32)
    assert run(ix, [a], [b], line(1), line(1), threshold=float("inf"), dim=1)["correspondences"][0, 0] == 1
    # 1.5e19 apart in two bins: each square is finite, their sum is not
    a[:], b[:] = 0.75e19, -0.75e19
    assert run(ix, [a], [b], line(1), line(1), threshold=float("inf"), dim=2)["correspondences"][0, 0] == 1
    assert run(ix, [a], [b], line(1), line(1), threshold=float("inf"), dim=1)["correspondences"][0, 0] == 6
    # FLT_MAX itself is "no neighbour" too (key_none), as in pcc_match_knn_batch_dims
    a[:], b[:] = 0.0, np.sqrt(np.float32(mdu.F32_MAX))
    b[0, 0] = np.float32(1.8446743e19)  # (its square rounds to FLT_MAX or below)
    run(ix, [a], [b], line(1), line(1), threshold=float("inf"), dim=1, what="around FLT_MAX")


@pytest.mark.parametrize("dim", (3, 32))
def test_duplicated_references_under_both_tie_orders(ix, dim):
    des1, des2 = mdu.tie_pair()
    tables = []
    for ties in (capi.TIES_LOWEST_INDEX, capi.TIES_FLANN):
        ix.set_tie_order(ties)
        tables.append(run(ix, [des1, des1], [des2, des2[:50]], line(2), line(2), threshold=0.001, dim=dim, what=f"ties {ties}"))
        rows = ix.match_knn_batch([(des1, des2), (des1, des2[:50])], threshold=0.001, dim=dim)
        assert tables[-1]["correspondences"][0].tolist()[:2] == [len(rows[0]), len(rows[1])]
    ix.set_tie_order(capi.TIES_LOWEST_INDEX)
    cmu.assert_same(tables[0], tables[1], "tie orders")
    assert tables[0]["correspondences"][0, 0] > 1


def copies(a, n, far=0):
    """n records: n - far copies of records of a (distance 0), then `far` records no record of a is near"""
    out = np.ascontiguousarray(a[np.arange(n) % len(a)])
    if far:
        out[n - far:] = 50.0
    return out


def test_acceptance_edges(ix):
    a = synth.descriptor_cloud(10, "uniform", 9)
    # scene 1: five clusters of 10 descriptors, 1000 apart; scene 2: the clusters each of them meets (the point counts, three times
    # as many from one cluster to the next, gate every other pair out)
    parts1 = [a] * 5
    points = [100, 300, 900, 2700, 8100]
    parts2 = [copies(a, 9),            # 0: n1 = n2 + 1, all matched: corr 10, 10 / 10 -> accepted
              copies(a, 8),            # 1: n1 = n2 + 2: corr 9 at most -> never
              copies(a, 12, far=1),    # 2: n1 <= n2, n2 - 1 matched: corr 12, 12 / 12 -> accepted
              copies(a, 12, far=2),    # 3: n2 - 2 matched: corr 11 -> not
              copies(a, 10, far=1),    # 4: two full candidates with equal corr (10) ...
              copies(a, 10, far=1),    # 5: ... the earlier one stays
              copies(a, 11, far=1)]    # 6: (a later candidate with a larger corr would replace it: 11 / 11)
    c1 = line(5, 1000.0)
    c2 = np.array([[0, 0, 0], [1000, 0, 0], [2000, 0, 0], [3000, 0, 0], [4000, 1, 0], [4000, 2, 0], [4000, 3, 0]], np.float32)
    got = run(ix, parts1, parts2, c1, c2, points1=points, points2=points + [8100, 8100], what="acceptance")
    assert (got["state"] == cmu.SEARCHED).sum() == 7
    assert got["candidates"][4].tolist() == [4, 5, 6]
    assert [int(got["correspondences"][i, 0]) for i in range(5)] == [10, 9, 12, 11, 10]
    assert got["correspondences"][4].tolist() == [10, 10, 11]
    assert got["matches"][:4].tolist() == [0, -1, 2, -1] and got["matches"][4] == 6
    # without the larger third candidate the first of the two equal ones stays
    got = run(ix, parts1, parts2[:6], c1, c2[:6], points1=points, points2=points + [8100], what="acceptance, equal corr")
    assert got["correspondences"][4].tolist()[:2] == [10, 10] and got["matches"][4] == 4


def test_candidate_edges(ix):
    a = synth.descriptor_cloud(8, "uniform", 3)
    nan = np.float32(np.nan)
    c1 = np.array([[0, 0, 0], [nan, 0, 0], [0, 0, 0]], np.float32)
    for n2 in (0, 1, 2):
        got = run(ix, [a] * 3, [a] * n2, c1, line(n2, 1.0), what=f"{n2} clusters in scene 2")
        assert got["candidates"][0].tolist() == list(range(n2)) + [-1] * (3 - n2)
        assert (got["candidates"][1] == -1).all() and (got["state"][1] == cmu.NONE).all()
    # two equidistant centroids (the lower index first), a NaN centroid in scene 2, one 2e12 away
    c2 = np.array([[0, 2, 0], [2, 0, 0], [nan, 0, 0], [2e12, 0, 0], [0, 0, 1]], np.float32)
    got = run(ix, [a] * 3, [a] * 5, c1, c2, what="candidate edges")
    assert got["candidates"].tolist() == [[4, 0, 1], [-1, -1, -1], [4, 0, 1]]
    got = run(ix, [a], [a] * 3, c1[:1], c2[1:4], what="only one within reach")
    assert got["candidates"].tolist() == [[0, -1, -1]] and got["state"].tolist() == [[3, 0, 0]]


def test_size_gate(ix):
    a = synth.descriptor_cloud(8, "uniform", 4)
    few = a[:3]
    c1 = line(4, 100.0)
    c2 = np.array([[x, y, 0] for x in (0, 100, 200, 300) for y in (1, 2, 3)][:10], np.float32)
    # cluster 0 (100 points) meets 99 / 100 / 199, cluster 1 meets 200 / 100 / 100; cluster 2 has 3 descriptors; cluster 3 no point
    got = run(ix, [a, a, few, a], [a, a, a, a, few, a, a, a, a, a], c1, c2, points1=[100, 100, 100, 0],
              points2=[99, 100, 199, 200, 100, 100, 99, 99, 99, 100], what="gates")
    assert got["state"].tolist() == [[2, 3, 3], [2, 1, 3], [1, 1, 1], [2, 2, 2]]


def test_nothing_searched_fills_the_tables(ix):
    a = synth.descriptor_cloud(3, "uniform", 4)
    got = run(ix, [a, a], [a], line(2), line(1), what="nothing searched")
    assert got["state"].tolist() == [[1, 0, 0], [1, 0, 0]] and (got["correspondences"] == 0).all() and (got["matches"] == -1).all()
    assert ix.stats()[:2] == [0, 0]


@pytest.mark.parametrize("dim", (3, 17))
def test_memory_spaces_and_strides(ix, gpu, grid_scene, dim):
    import torch
    parts1, parts2 = grid_scene[0][10:20], grid_scene[1][10:20]
    des1, des2 = cat(parts1), cat(parts2)
    args = (offsets_of(parts1), offsets_of(parts2), line(10), line(10), [100] * 10, [100] * 10)
    call = lambda d1, d2: ix.cluster_matching(d1, args[0], d2, args[1], *args[2:], threshold=0.0075 * dim, dim=dim)
    want = call(des1, des2)
    cmu.assert_same(want, cmu.restate(des1, args[0], des2, args[1], *args[2:], threshold=0.0075 * dim, dim=dim), "host")
    assert (want["state"] == cmu.SEARCHED).sum() == 30
    t1, t2 = torch.from_numpy(des1).cuda(), torch.from_numpy(des2).cuda()
    torch.cuda.synchronize()
    cmu.assert_same(call(t1, t2), want, "device tensors")
    # rows 4 * dim + 8 bytes apart, NaN between them: on the host and on the device
    wide1, wide2 = (np.full((len(d), dim + 2), np.nan, np.float32) for d in (des1, des2))
    wide1[:, :dim], wide2[:, :dim] = des1[:, :dim], des2[:, :dim]
    cmu.assert_same(call(wide1[:, :dim], wide2[:, :dim]), want, "strided host arrays")
    w1, w2 = torch.from_numpy(wide1).cuda()[:, :dim], torch.from_numpy(wide2).cuda()[:, :dim]
    torch.cuda.synchronize()
    cmu.assert_same(call(w1, w2), want, "strided device tensors")
    tight1, tight2 = torch.from_numpy(np.ascontiguousarray(des1[:, :dim])).cuda(), torch.from_numpy(np.ascontiguousarray(des2[:, :dim])).cuda()
    torch.cuda.synchronize()
    cmu.assert_same(call(tight1, tight2), want, "tight device tensors")


@pytest.mark.parametrize("dim", (3, 32))
@pytest.mark.parametrize("family", synth.DESCRIPTOR_FAMILIES)
@pytest.mark.parametrize("name,n_pairs", [("results", 7), ("cuarto2", 88)])
def test_row_lengths_on_the_recorded_workloads(ix, name, n_pairs, family, dim):
    """per searched pair the count is len(row) of Index.match_knn_batch on the same two clusters, under either tie order; the
    candidates, gates and matches are the restatement's"""
    o1, o2, c1, c2, p1, p2 = cmu.run_tables(name)
    des1, des2 = cmu.run_descriptors(name, family)
    # (the uniform family's queries lie about 0.0075 a bin from their source: the reference's 0.05 would match none on 32 bins)
    threshold = 0.0075 * dim if family == "uniform" and dim > 3 else 0.05
    got = ix.cluster_matching(des1, o1, des2, o2, c1, c2, p1, p2, threshold=threshold, dim=dim)
    want = cmu.restate(des1, o1, des2, o2, c1, c2, p1, p2, counts=False)
    np.testing.assert_array_equal(got["candidates"], want["candidates"])
    np.testing.assert_array_equal(got["state"], want["state"])
    searched = list(zip(*np.nonzero(got["state"] == cmu.SEARCHED)))
    assert len(searched) == n_pairs
    stats = ix.stats()
    pairs = [(des1[o1[i]:o1[i + 1]], des2[o2[got["candidates"][i, k]]:o2[got["candidates"][i, k] + 1]]) for i, k in searched]
    assert stats[:2] == [n_pairs, sum(len(b) for _, b in pairs)]
    for ties in (capi.TIES_LOWEST_INDEX, capi.TIES_FLANN):
        rows = ix.match_knn_batch(pairs, threshold=threshold, ties=ties, dim=dim)
        assert [int(got["correspondences"][i, k]) for i, k in searched] == [len(r) for r in rows], f"ties {ties}"
    assert (got["correspondences"][got["state"] != cmu.SEARCHED] == 0).all()
    n1, n2 = np.diff(o1), np.diff(o2)
    np.testing.assert_array_equal(got["matches"], cmu.accept(got["candidates"], got["state"], got["correspondences"], n1, n2))
    assert any(1 < int(got["correspondences"][i, k]) for i, k in searched)


def test_the_context_is_unharmed(gpu, grid_scene):
    import oracle
    ref = synth.corridor_cloud(20000, synth.SEED_A)
    qry = synth.corridor_cloud(3000, synth.SEED_B)
    parts1, parts2 = grid_scene[0][:5], grid_scene[1][:5]
    with capi.Index(ref, auto_sync=False) as h:
        h.set_tie_order(capi.TIES_FLANN)
        idx0, d0 = h.nn1(qry)
        run(h, parts1, parts2, line(5), line(5), what="on a handle that indexes a cloud")
        idx1, d1 = h.nn1(qry)
        assert h._ties == capi.TIES_FLANN and h.n_original == len(ref)
    assert np.array_equal(idx0, idx1) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
    oi, od = oracle.nn1_exhaustive(ref, qry)
    assert np.array_equal(d1.view(np.uint32), od.view(np.uint32))
