"""pcc_match_fpfh_batch on the GPU: the reference's matchFPFH (src/comparator.cpp:877-910) on the 33 bins of an FPFH descriptor,
from host and from device memory.  Every comparison is bit-exact against the NumPy restatement in match_dims_util at dim = 33
(float32 running sum in index order, lowest index among equals), whose sensitivity tests/test_match_fpfh_cpu.py asserts on the
same inputs."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from pointcloudcomparator_amd import capi

sys.path.insert(0, str(Path(__file__).resolve().parent))
import fpfh_util  # noqa: E402
import match_dims_util as mdu  # noqa: E402
import match_fpfh_util as mfu  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
TIES = {"lowest": capi.TIES_LOWEST_INDEX, "flann": capi.TIES_FLANN}
INF = np.float32(np.inf)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same(got, want, what=""):
    """(rows, d2 rows) from the library against [(row, d2, tied)] from the restatement: indices and distance bits"""
    rows, d2 = got
    assert len(rows) == len(d2) == len(want)
    for p, (w_row, w_d2, _tied) in enumerate(want):
        assert isinstance(rows[p], np.ndarray) and rows[p].dtype == np.int32 and d2[p].dtype == np.float32
        assert rows[p][0] == 0 and bits(d2[p][:1])[0] == 0, f"{what} pair {p}: the dummy"
        assert np.array_equal(rows[p], w_row), f"{what} pair {p}: indices differ from the restatement"
        assert np.array_equal(bits(d2[p]), bits(w_d2)), f"{what} pair {p}: distance bits differ from the restatement"


@pytest.fixture(scope="module")
def ix(gpu):
    with capi.Index(np.zeros((4, 3), np.float32)) as h:
        yield h


@pytest.fixture(scope="module")
def parity():
    """the 35 pairs, their threshold (the batch's median minimum distance) and the restatement's rows, computed once"""
    pairs = mfu.parity_pairs()
    free = [mdu.restate(a, b, 33, INF) for a, b in pairs]
    thr = np.float32(np.median(np.concatenate([w[1][1:] for w in free])))
    want = [mdu.restate(a, b, 33, thr) for a, b in pairs]
    kept = sum(len(w[0]) - 1 for w in want)
    n_queries = sum(len(b) for _, b in pairs)
    assert 0 < kept < sum(len(w[0]) - 1 for w in free) <= n_queries          # rows are kept AND dropped
    return pairs, thr, want, n_queries


@pytest.fixture(scope="module")
def host_parity(ix, parity):
    """the parity batch from host memory at stride 132, for the device test to compare with"""
    pairs, thr, _want, _n = parity
    got = ix.match_fpfh_batch(pairs, threshold=thr, return_d2=True)
    return got, list(ix.stats())


@pytest.mark.parametrize("stride", mfu.STRIDES)
def test_parity_with_the_restatement(ix, parity, stride):
    """35 pairs (n1 x n2 around the wave share, the slice and the query block; both families) in one call, per row stride
    (floats behind bin 32 are NaN): indices, distance bits, offsets and dummies, the stats, and the rows without out_d2"""
    pairs, thr, want, n_queries = parity
    memo = {}
    strided = [(mfu.with_stride(a, stride, memo), mfu.with_stride(b, stride, memo)) for a, b in pairs]
    assert all(x.shape[1] == 33 and (len(x) < 2 or x.strides[0] == stride) for ab in strided for x in ab)
    assert strided[0][0] is strided[2][0]                                     # shared des1 arrays stay shared
    for ties in TIES.values():
        ix.set_tie_order(ties)
        got = ix.match_fpfh_batch(strided, threshold=thr, return_d2=True)
        st = ix.stats()
        same(got, want, f"stride {stride}")
        assert st[1] == n_queries and st[5] == sum(w[2] for w in want) and st[6] == 0, st
    rows_only = ix.match_fpfh_batch(strided, threshold=thr)                   # out_d2 = NULL
    assert all(np.array_equal(r, w[0]) for r, w in zip(rows_only, want))
    ix.set_tie_order(capi.TIES_LOWEST_INDEX)


def test_bin_32_decides(ix):
    """300 references equal in bins 0 ... 31 and distinct in bin 32: 33 bins see the permutation, the 32-wide search sees one
    point -- a forward to pcc_match_knn_batch_dims(dim = 32) fails here"""
    a, b, perm = mfu.bin32_pair()
    want = mdu.restate(a, b, 33, 0.25)
    assert np.array_equal(want[0][1:], perm)
    got = ix.match_fpfh_batch([(a, b)], return_d2=True)
    same(got, [want])
    assert np.array_equal(got[0][0][1:], perm)
    ix.set_tie_order(capi.TIES_LOWEST_INDEX)
    assert np.array_equal(ix.match_knn_batch([(a, b)], threshold=0.25, dim=32)[0], np.zeros(131, np.int32))


@pytest.mark.parametrize("ties", sorted(TIES))
def test_ties_and_slices(ix, ties):
    """duplicates in another slice than their originals, and two distinct records at one distance (made by bin 32): the lowest
    index wins and [5] counts the tied queries, under either tie order of the handle"""
    a, b = mfu.tie_pair()
    want = mdu.restate(a, b, 33, 0.25)
    assert want[2] == 80 and len(a) > 256
    ix.set_tie_order(TIES[ties])
    got = ix.match_fpfh_batch([(a, b)], return_d2=True)
    st = ix.stats()
    ix.set_tie_order(capi.TIES_LOWEST_INDEX)
    same(got, [want], ties)
    assert got[0][0][1:].tolist() == list(range(100))
    assert st[1] == 100 and st[5] == 80 and st[6] == 0, st


def test_invalid_and_overflow(ix):
    clean = mfu.fpfh_cloud(60, "fpfh-like", 91)
    a = clean.copy()
    a[7, 32] = np.nan            # invalid in bin 32 alone: never returned
    a[9, 32] = np.inf
    a[11, 32] = -np.inf
    a[13, 0] = np.nan            # invalid in bin 0 alone
    a[15, 0] = -np.inf
    b = clean[[7, 9, 11, 13, 15, 20, 30, 31, 32]].copy()
    b[6, 32] = np.nan            # invalid queries: no row entry
    b[7, 0] = np.inf
    b[8, 32] = -np.inf
    none_valid = clean.copy()
    none_valid[:, 32] = np.nan
    none_valid[::2, 0] = np.inf
    empty = np.zeros((0, 33), np.float32)
    # +-3e19: every distance from the first query overflows to +inf (no neighbour); the second finds its own record
    far_a, far_b = np.zeros((3, 33), np.float32), np.zeros((2, 33), np.float32)
    far_a[:, 31:] = np.float32(3e19)
    far_b[0, 31:] = np.float32(-3e19)
    far_b[1, 31:] = np.float32(3e19)
    pairs = [(a, b), (none_valid, b), (empty, b), (a, empty), (far_a, far_b), (a, b)]
    with np.errstate(over="ignore", invalid="ignore"):
        want = [mdu.restate(x, y, 33, INF) for x, y in pairs]
        assert np.isinf(mdu.d2_chain(far_a, far_b, 33)[0]).all()
    assert want[0][0].tolist()[-1] == 20 and len(want[0][0]) == 7 and not {7, 9, 11, 13, 15} & set(want[0][0].tolist())
    assert all(len(want[p][0]) == 1 for p in (1, 2, 3))                     # the dummy alone
    assert want[4][0].tolist() == [0, 0] and want[4][1].tolist() == [0.0, 0.0]
    got = ix.match_fpfh_batch(pairs, threshold=INF, return_d2=True)
    same(got, want)
    assert ix.stats()[1] == sum(len(y) for _, y in pairs)                   # (a pair without references still has queries)
    for p in (2, 3):
        assert got[0][p].tolist() == [0] and got[1][p].tolist() == [0.0]
    # a batch of nothing to search, and no pair at all
    rows, d2 = ix.match_fpfh_batch([(empty, b), (a, empty)], return_d2=True)
    assert [r.tolist() for r in rows] == [[0], [0]] and [d.tolist() for d in d2] == [[0.0], [0.0]]
    assert ix.match_fpfh_batch([]) == []


def test_device_memory_equals_host_memory(ix, parity, host_parity):
    """the parity pairs at stride 132 as CUDA tensors, the shared des1 tensors included: rows, d2 and stats of the host call"""
    import torch
    pairs, thr, want, n_queries = parity
    (h_rows, h_d2), h_stats = host_parity
    dev = {}

    def up(x):
        if id(x) not in dev:
            dev[id(x)] = torch.from_numpy(x).cuda()
        return dev[id(x)]

    dpairs = [(up(a), up(b)) for a, b in pairs]
    assert dpairs[0][0] is dpairs[2][0] and all(t.is_cuda and t.stride(0) == 33 for ab in dpairs for t in ab if t.shape[0] > 1)
    rows, d2 = ix.match_fpfh_batch(dpairs, threshold=thr, return_d2=True)
    st = list(ix.stats())
    same((rows, d2), want, "device memory")
    for p in range(len(pairs)):
        assert np.array_equal(rows[p], h_rows[p]) and np.array_equal(bits(d2[p]), bits(h_d2[p])), p
    assert [st[k] for k in (1, 5, 6)] == [h_stats[k] for k in (1, 5, 6)] == [n_queries, sum(w[2] for w in want), 0]
    rows_only = ix.match_fpfh_batch(dpairs, threshold=thr)
    assert all(np.array_equal(r, w[0]) for r, w in zip(rows_only, want))
    with pytest.raises(ValueError):
        ix.match_fpfh_batch([(dpairs[0][0], pairs[0][1])])
    # the tensors were only read
    torch.cuda.synchronize()
    assert all(np.array_equal(bits(up(x).cpu().numpy()), bits(x)) for ab in pairs for x in ab)


@pytest.fixture(scope="module")
def end_to_end(gpu):
    """clouds A and B indexed from CUDA tensors, their descriptors left on the device and matched there at the reference's 0.25:
    (row, descriptors of A, descriptors of B) with the descriptors downloaded afterwards"""
    import torch
    a, b = mfu.scene_clouds()
    with capi.Index(torch.from_numpy(a).cuda(), engine=capi.ENGINE_GRID, device=0) as ia, \
            capi.Index(torch.from_numpy(b).cuda(), engine=capi.ENGINE_GRID, device=0) as ib:
        ha, _ = ia.fpfh_descriptors()
        hb, _ = ib.fpfh_descriptors()
        assert ha.is_cuda and hb.is_cuda and ha.shape[1] == 33 and hb.shape[1] == 33
        row = ia.match_fpfh_batch([(ha, hb)])[0]
        torch.cuda.synchronize()
        return row, ha.cpu().numpy(), hb.cpu().numpy()


def test_end_to_end_on_the_device(end_to_end):
    """volume300 (300 points) and the same cloud without the 15 points within 0.05 of its corner: descriptors far from the cut are
    unchanged and match at distance 0, those near it change.  On the CPU mirror (build/fpfh_host) 171 of B's 285 descriptors find
    a descriptor of A below 0.25, 45 of them at distance 0."""
    row, ha, hb = end_to_end
    assert len(ha) > 250 and 200 < len(hb) < len(ha)
    want = mdu.restate(ha, hb, 33, 0.25)
    assert np.array_equal(row, want[0])
    kept = len(row) - 1
    assert 0 < kept < len(hb), (kept, len(hb))
    assert (want[1][1:] == 0).any() and (want[1][1:] > 0).any()


def test_cpp_mirror(end_to_end, tmp_path):
    """tests/cpp/fpfh_match_driver.cpp: pcc::processFPFH on both clouds, then pcc::matchFPFH, against the Python row"""
    exe = ROOT / "build" / "fpfh_match_driver"
    if not exe.exists():
        subprocess.check_call(["make", "build/fpfh_match_driver"], cwd=ROOT)
    row, ha, hb = end_to_end
    a, b = mfu.scene_clouds()
    fa, fb, fout = tmp_path / "a.in", tmp_path / "b.in", tmp_path / "match.out"
    fpfh_util.write_cloud(fa, a)
    fpfh_util.write_cloud(fb, b)
    r = subprocess.run([str(exe), str(fa), str(fb), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    raw = np.fromfile(fout, np.int32)
    assert raw[0] == len(raw) - 1
    assert np.array_equal(raw[1:], row)
    assert f"fpfh_match_driver des1={len(ha)} des2={len(hb)} kept={len(row) - 1}\n" in r.stdout
    assert "Found NaN in FPFH descriptors" not in r.stdout                   # (every descriptor of these clouds is finite)
