"""pcc_match_knn_batch on the GPU: every cluster pair of a comparison in one call (reference src/comparator.cpp:1296-1365,
matchRIFTFeaturesKnn at :560-588).  Every comparison is bit-exact: against the CPU oracle's FLANN-ordered answer
(oracle.match_rift_knn) under TIES_FLANN, and against the single-call path (set_input + match_knn on one handle, as the
C++ mirror does it) under both tie orders.

Workloads: the two recorded runs replayed into tests/golden/match_workloads.json (7 and 88 gated pairs, the largest
23 528 x 26 308), a seeded batch of 300 pairs with sizes drawn from the recorded descriptor counts, and edge pairs.
Descriptor contents are synthetic (pointcloudcomparator_amd.synth): "uniform" (ties rare) and "quantised" (ties in most
queries).  The whole file took 2 s on one MI355X, imports aside (the suite's step limit is 900 s)."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle
from pointcloudcomparator_amd import capi, synth

sys.path.insert(0, str(Path(__file__).resolve().parent))
import match_batch_util as mbu  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
TIES = {"lowest": capi.TIES_LOWEST_INDEX, "flann": capi.TIES_FLANN}


def single_path(ix, des1, des2):
    """what the C++ mirror's matchRIFTFeaturesKnn returns: the handle re-pointed at des1, then match_knn(des2); a cloud the
    library refuses as empty gives the dummy alone"""
    try:
        ix.set_input(des1)
        return ix.match_knn(des2)
    except capi.PccError as e:
        assert e.status == -2, e
        return np.zeros(1, np.int32)


def check_batch(ix, pairs, ties, with_oracle=True):
    ix.set_tie_order(ties)
    got = ix.match_knn_batch(pairs)
    stats = ix.stats()
    assert len(got) == len(pairs)
    assert stats[1] == sum(len(b) for _, b in pairs)
    for p, (a, b) in enumerate(pairs):
        want = single_path(ix, a, b)
        assert got[p].dtype == np.int32 and got[p][0] == 0
        assert np.array_equal(got[p], want), f"pair {p} ({len(a)} x {len(b)}): differs from the single-call path"
        if with_oracle and ties == capi.TIES_FLANN and len(a) and len(b):
            assert np.array_equal(got[p], oracle.match_rift_knn(a, b)), f"pair {p} ({len(a)} x {len(b)}): differs from the oracle"
    return got, stats


@pytest.fixture(scope="module")
def ix(gpu):
    with capi.Index(np.zeros((4, 32), np.float32), auto_sync=False) as h:
        yield h


@pytest.mark.parametrize("ties", sorted(TIES))
@pytest.mark.parametrize("family", synth.DESCRIPTOR_FAMILIES)
@pytest.mark.parametrize("workload", ["results", "cuarto2"])
def test_replayed_workloads(ix, workload, family, ties):
    sizes = mbu.workloads()[workload]["pairs"]
    if workload == "cuarto2":
        assert [23528, 26308] in [s[2:] for s in sizes]  # the largest recorded pair is part of it
    pairs = synth.descriptor_pairs(sizes, family, seed=7)
    got, stats = check_batch(ix, pairs, TIES[ties])
    assert sum(len(g) for g in got) > len(got)  # something matched
    if ties == "flann" and family == "quantised":
        # the tie path really ran: queries were flagged, and FLANN's walk named another index than the lowest somewhere
        assert stats[5] > 0 and stats[6] > 0, stats
        ix.set_tie_order(capi.TIES_LOWEST_INDEX)
        lowest = ix.match_knn_batch(pairs)
        assert any(not np.array_equal(a, b) for a, b in zip(got, lowest))
    if ties == "lowest":
        assert stats[5] == 0 and stats[6] == 0, stats


@pytest.mark.parametrize("ties", sorted(TIES))
@pytest.mark.parametrize("family", synth.DESCRIPTOR_FAMILIES)
def test_300_pairs_with_recorded_sizes(ix, family, ties):
    sizes = mbu.drawn_sizes(300)
    assert len(sizes) == 300 and min(min(s[2], s[3]) for s in sizes) > 3
    check_batch(ix, synth.descriptor_pairs(sizes, family, seed=11), TIES[ties])


def _edge_pairs(width, family):
    """pairs of (n, width) float32 arrays: every edge the entry point documents, in one batch"""
    def cloud(n, seed):
        return np.ascontiguousarray(synth.descriptor_cloud(n, family, seed)[:, :width])

    pairs = []
    ns = (0, 1, 63, 64, 65)
    for k, n1 in enumerate(ns):
        for m, n2 in enumerate(ns):
            a = cloud(n1, 100 + k)
            b = cloud(n2, 200 + 5 * k + m)
            if n1 and n2:
                b[: n2 // 2] = a[np.arange(n2 // 2) % n1]  # exact matches beside the far ones
            pairs.append((a, b))
    a = cloud(200, 300)
    nonfinite = a.copy()
    nonfinite[:, 0] = np.nan
    nonfinite[1::2, 1] = np.inf
    pairs.append((nonfinite, cloud(70, 301)))            # no finite reference at all: the dummy alone
    holes = a.copy()
    holes[::3, 2] = np.nan                                # non-finite references keep their places: indices stay original
    b = a[::-1].copy()
    b[5, 0] = np.inf                                      # non-finite queries: no match
    b[6, 1] = -np.inf
    b[7, 2] = np.nan
    pairs.append((holes, b))
    far = cloud(10, 302)
    far[:, :3] = np.float32(-3e19)
    bq = cloud(10, 303)
    bq[:, :3] = np.float32(3e19)                          # (6e19)^2 overflows: no match
    bq[3, :3] = np.float32(-3e19)                         # ... but this one is at distance 0
    pairs.append((far, bq))
    rep_a, rep_b = cloud(150, 304), cloud(90, 305)
    rep_b[:40] = rep_a[:40]
    pairs.append((rep_a, rep_b))
    pairs.append((rep_a, rep_b))                          # a pair repeated
    shared = cloud(500, 306)
    for s in range(3):                                    # three pairs sharing one des1
        q = cloud(130 + s, 307 + s)
        q[:60] = shared[s * 60:(s + 1) * 60]
        pairs.append((shared, q))
    return pairs


@pytest.mark.parametrize("ties", sorted(TIES))
@pytest.mark.parametrize("family", synth.DESCRIPTOR_FAMILIES)
@pytest.mark.parametrize("stride", [12, 16, 32, 128])
def test_edge_pairs(ix, stride, family, ties):
    pairs = _edge_pairs(stride // 4, family)
    assert all(a.strides[0] == stride or len(a) <= 1 for ab in pairs for a in ab)
    got, _ = check_batch(ix, pairs, TIES[ties])
    n = len(pairs)
    for p, (a, b) in enumerate(pairs):
        if len(a) == 0 or len(b) == 0:
            assert got[p].tolist() == [0]
    assert got[25].tolist() == [0]                                   # all references non-finite
    assert not set(got[26][1:].tolist()) & set(range(0, 200, 3))     # a non-finite reference is never named
    assert len(got[26]) <= 1 + 200 - 3                               # the three non-finite queries matched nothing
    assert got[27].tolist() == [0, 0] if ties == "lowest" else len(got[27]) == 2   # only the query at distance 0
    assert np.array_equal(got[28], got[29]) and len(got[28]) >= 41
    assert n == 33 and all(len(got[p]) >= 61 for p in (30, 31, 32))


def _check_both_entries(ix, pairs, ties):
    """pcc_match_knn_batch against the per-pair loop (and the oracle), then pcc_match_knn_batch_dims at dim = 3: the same rows,
    and beside each the squared distance the restated arithmetic gives"""
    got, _ = check_batch(ix, pairs, ties)
    rows, d2 = ix.match_knn_batch(pairs, dim=3, return_d2=True)
    for p, (a, b) in enumerate(pairs):
        assert np.array_equal(rows[p], got[p]), f"pair {p} ({len(a)} x {len(b)}): dim = 3 differs from pcc_match_knn_batch"
        assert d2[p].dtype == np.float32 and d2[p][0] == 0
        if 0 < len(a) * len(b) <= 1_000_000:   # (the distance matrix of a larger pair is left to the rows above)
            t = b[:, None, :3] - a[None, :, :3]
            t = t * t
            best = ((t[..., 0] + t[..., 1]) + t[..., 2]).min(1)
            assert np.array_equal(d2[p][1:].view(np.uint32), best[best < np.float32(0.05)].view(np.uint32)), p
    return got


@pytest.mark.parametrize("ties", sorted(TIES))
@pytest.mark.parametrize("family", synth.DESCRIPTOR_FAMILIES)
def test_slice_at_its_minimum(ix, family, ties):
    """255, 256 and 257 references in one call: far fewer than 1024 items, so the slice falls to 256 and the 257 references
    are a full slice and a slice of ONE; two pairs share one des1 (pointer and length), packed once.  Queries whose nearest
    reference is the last one have their answer in the slice of one"""
    pairs = []
    for k, (n1, n2) in enumerate(((255, 63), (256, 64), (257, 65))):
        a, b = synth.descriptor_cloud(n1, family, 400 + k), synth.descriptor_cloud(n2, family, 410 + k)
        b[:8] = a[-1]                     # the last reference, at distance 0 ...
        b[8:16] = a[n1 - 16:n1 - 8]       # ... and others of the last sixteenth
        pairs.append((a, b))
    shared = pairs[2][0]
    q = synth.descriptor_cloud(70, family, 420)
    q[:4] = shared[-1]
    pairs.append((shared, q))             # the same array: the same pointer and length as pair 2's des1
    got = _check_both_entries(ix, pairs, TIES[ties])
    if ties == "lowest" and family == "uniform":
        assert got[2][1:9].tolist() == [256] * 8 and got[3][1:5].tolist() == [256] * 4 and got[1][1:9].tolist() == [255] * 8


@pytest.mark.parametrize("ties", sorted(TIES))
@pytest.mark.parametrize("family", synth.DESCRIPTOR_FAMILIES)
def test_slice_at_its_maximum(ix, family, ties):
    """one pair of 2049 references and 32768 queries: 512 query blocks x 2 slices = 1024 items, just enough for the slice to
    stay at 2048 -- the second slice holds ONE reference, and it is the answer of some queries in every part of the table"""
    a, b = synth.descriptor_cloud(2049, family, 430), synth.descriptor_cloud(32768, family, 431)
    b[1::101] = a[2047]
    b[::97] = a[-1]
    got = _check_both_entries(ix, [(a, b)], TIES[ties])
    if ties == "lowest" and family == "uniform":
        assert (got[0][1:] == 2048).sum() >= len(b[::97])


def test_empty_batch_and_all_empty_pairs(ix):
    assert ix.match_knn_batch([]) == []
    e = np.zeros((0, 32), np.float32)
    got = ix.match_knn_batch([(e, e), (e, np.ones((5, 32), np.float32)), (np.ones((5, 32), np.float32), e)])
    assert [g.tolist() for g in got] == [[0], [0], [0]]


def test_module_level_entry_makes_its_own_context(gpu):
    sizes = mbu.workloads()["results"]["pairs"]
    pairs = synth.descriptor_pairs(sizes, "quantised", seed=7)
    got = capi.match_knn_batch(pairs, ties=capi.TIES_FLANN)
    for g, (a, b) in zip(got, pairs):
        assert np.array_equal(g, oracle.match_rift_knn(a, b))


def test_device_arrays_are_refused(ix):
    import ctypes as C
    a = np.zeros((4, 32), np.float32)
    vp, sz = (C.c_void_p * 1)(a.ctypes.data), (C.c_size_t * 1)(4)
    out, off = np.zeros(8, np.int32), np.zeros(2, np.uintp)
    st = capi.LIB.pcc_match_knn_batch(ix._h, 1, vp, sz, vp, sz, 128, capi.MEM_DEVICE, np.float32(0.05), out.ctypes.data, off.ctypes.data)
    assert st == -5 and b"host" in capi.LIB.pcc_last_error()


def test_the_context_is_unharmed(gpu):
    """the handle that lends device, stream and scratch answers afterwards as before: same nn1 bits, same cloud, same tie order"""
    ref = synth.corridor_cloud(20000, synth.SEED_A)
    qry = synth.corridor_cloud(3000, synth.SEED_B)
    pairs = synth.descriptor_pairs(mbu.workloads()["results"]["pairs"], "quantised", seed=7)
    for ties in (capi.TIES_LOWEST_INDEX, capi.TIES_FLANN):
        with capi.Index(ref, auto_sync=False) as h:
            h.set_tie_order(ties)
            i0, d0 = h.nn1(qry)
            size0 = h.size
            h.match_knn_batch(pairs)
            capi.match_knn_batch(pairs, ties=capi.TIES_FLANN, ctx=h)   # (another tie order for the call only)
            i1, d1 = h.nn1(qry)
            assert h.size == size0
            assert np.array_equal(i0, i1) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
            assert h._ties == ties


def test_cpp_mirror_and_report(gpu):
    """tests/cpp/test_match_batch.cpp: matchRIFTFeaturesKnnBatch against a loop of matchRIFTFeaturesKnn, and clusterSections
    on two small scenes with descriptors against the results.txt / stdout recorded before the batch call went in"""
    exe = ROOT / "build" / "test_match_batch"
    if not exe.exists():
        subprocess.check_call(["make", "hosttest"], cwd=ROOT)
    r = subprocess.run([str(exe), str(ROOT / "tests" / "golden")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "match batch ok" in r.stdout
