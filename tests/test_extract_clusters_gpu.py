"""pcc_extract_clusters / Index.extract_clusters against np.argsort(kind="stable") restricted to labels >= 0 (the order
`for i: clusters[labels[i]].push_back(i)` gives, reference src/segmentation.cpp:133-152 and :290-318).  Everything is integer or
byte-exact.  The shapes straddle a tile of the scatter (256), a workgroup's chunk (2048 entries from 4097 points on: two
workgroups) and the one-pass limit of 255 clusters (256 and 300 take two 8-bit passes)."""
import numpy as np
import pytest

from plane_removal_util import three_planes
from pointcloudcomparator_amd import capi
from segment_util import stable_partition, to_numpy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu):
    with capi.Index(np.zeros((1, 3), np.float32)) as ix:
        yield ix


def _labels(n, n_clusters, seed):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, n_clusters, n).astype(np.int32)
    labels[rng.random(n) < 0.2] = -1
    return labels


def _records(n, cols=12, seed=0):
    """input stride 48: every word of a record is its own"""
    return np.random.default_rng(seed).random((n, cols)).astype(np.float32)


def _check(got, records, labels, n_clusters, record_bytes=None):
    want_index, want_offsets = stable_partition(labels, n_clusters)
    index, offsets = got[0], got[1]
    np.testing.assert_array_equal(offsets, want_offsets)
    np.testing.assert_array_equal(index, want_index)
    if len(got) > 2:
        words = (record_bytes or records.shape[1] * 4) // 4
        assert got[2].shape == (len(want_index), words)
        assert (got[2].view(np.uint32) == records[want_index, :words].view(np.uint32)).all()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025, 4097])
@pytest.mark.parametrize("n_clusters", [1, 2, 255, 256, 300])
def test_extract_equals_the_stable_argsort(ctx, n, n_clusters):
    labels = _labels(n, n_clusters, 1000 * n_clusters + n)
    records = _records(n)
    _check(ctx.extract_clusters(records, labels, n_clusters), records, labels, n_clusters)


def test_single_cases(ctx):
    records = _records(700)
    # all left out
    labels = np.full(700, -1, np.int32)
    index, offsets, out = ctx.extract_clusters(records, labels, 3)
    assert len(index) == 0 and len(out) == 0 and (offsets == 0).all() and len(offsets) == 4
    # cluster ids that no point carries: empty slices, in front, in between and behind
    labels = _labels(700, 3, 7) * 2 + 1
    labels[labels < 0] = -1
    got = ctx.extract_clusters(records, labels, 8)
    _check(got, records, labels, 8)
    assert (np.diff(got[1])[[0, 2, 4, 6, 7]] == 0).all() and (np.diff(got[1])[[1, 3, 5]] > 0).all()
    # one cluster holds everything
    labels = np.zeros(700, np.int32)
    index, offsets, out = ctx.extract_clusters(records, labels, 1)
    np.testing.assert_array_equal(index, np.arange(700))
    np.testing.assert_array_equal(offsets, [0, 700])
    assert (out.view(np.uint32) == records.view(np.uint32)).all()
    # nothing to do
    index, offsets = ctx.extract_clusters(records[:0], labels[:0], 3, with_records=False)
    assert len(index) == 0 and (offsets == 0).all()
    index, offsets = ctx.extract_clusters(records, np.full(700, -1, np.int32), 0, with_records=False)
    assert len(index) == 0 and list(offsets) == [0]


@pytest.mark.parametrize("record_bytes,out_stride", [(12, 12), (16, 32), (32, 32)])
def test_record_lengths_and_untouched_slot_bytes(ctx, record_bytes, out_stride):
    n, n_clusters = 1025, 5
    records, labels = _records(n), _labels(n, n_clusters, 3)
    want_index, want_offsets = stable_partition(labels, n_clusters)
    m = len(want_index)
    for device in (False, True):
        out = np.full((n, out_stride // 4), 0x5A5A5A5A, np.uint32)
        index = np.full(n, -7, np.int32)
        offsets = np.zeros(n_clusters + 1, np.uintp)
        if device:
            import torch
            d_rec, d_lab, d_out, d_idx = (torch.from_numpy(a).cuda() for a in (records, labels, out.view(np.int32), index))
            torch.cuda.synchronize()
            args = (d_rec.data_ptr(), n, 48, record_bytes, d_lab.data_ptr(), n_clusters, capi.MEM_DEVICE, d_out.data_ptr(), out_stride,
                    d_idx.data_ptr(), offsets.ctypes.data)
        else:
            args = (records.ctypes.data, n, 48, record_bytes, labels.ctypes.data, n_clusters, capi.MEM_HOST, out.ctypes.data, out_stride,
                    index.ctypes.data, offsets.ctypes.data)
        assert capi.LIB.pcc_extract_clusters(ctx._h, *args) == 0, capi.LIB.pcc_last_error()
        if device:
            ctx.sync()
            out, index = d_out.cpu().numpy().view(np.uint32), d_idx.cpu().numpy()
        np.testing.assert_array_equal(offsets.astype(np.int64), want_offsets)
        np.testing.assert_array_equal(index[:m], want_index)
        words = record_bytes // 4
        assert (out[:m, :words] == records.view(np.uint32)[want_index, :words]).all()
        assert (out[:m, words:] == 0x5A5A5A5A).all() and (out[m:] == 0x5A5A5A5A).all()  # beyond record_bytes, beyond the clusters


def test_device_memory_leaves_host_arrays_alone_and_equals_host(ctx):
    import torch
    n, n_clusters = 4097, 300
    records, labels = _records(n), _labels(n, n_clusters, 11)
    host = ctx.extract_clusters(records, labels, n_clusters, record_bytes=16)
    keep = (records.copy(), labels.copy())
    dev = ctx.extract_clusters(torch.from_numpy(records).cuda(), torch.from_numpy(labels).cuda(), n_clusters, record_bytes=16)
    assert dev[0].is_cuda and dev[2].is_cuda and isinstance(dev[1], np.ndarray)
    np.testing.assert_array_equal(dev[0].cpu().numpy(), host[0])
    np.testing.assert_array_equal(dev[1], host[1])
    assert (dev[2].cpu().numpy().view(np.uint32) == host[2].view(np.uint32)).all()
    assert (records.view(np.uint32) == keep[0].view(np.uint32)).all() and (labels == keep[1]).all()
    _check(host, records, labels, n_clusters, 16)


def test_two_calls_give_identical_bytes(ctx):
    n, n_clusters = 4097, 255
    records, labels = _records(n), _labels(n, n_clusters, 5)
    a = ctx.extract_clusters(records, labels, n_clusters)
    b = ctx.extract_clusters(records, labels, n_clusters)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("bad", [3, 7, -2, 2 ** 31 - 1])
def test_a_label_outside_the_range_is_an_input_error(ctx, bad):
    """found on the device, where no table is indexed by the label itself: PCC_ERR_INVALID, and the handle works on"""
    n = 1025
    records, labels = _records(n), _labels(n, 3, 2)
    labels[600] = bad
    with pytest.raises(capi.PccError) as e:
        ctx.extract_clusters(records, labels, 3)
    assert e.value.status == -1 and "label" in str(e.value)
    import torch
    with pytest.raises(capi.PccError) as e:
        ctx.extract_clusters(torch.from_numpy(records).cuda(), torch.from_numpy(labels).cuda(), 3)
    assert e.value.status == -1
    labels[600] = 2
    _check(ctx.extract_clusters(records, labels, 3), records, labels, 3)


def test_device_chain_of_the_euclidean_path(gpu):
    """plane_removal -> set_input -> euclidean_clusters -> extract_clusters, everything in device memory, against the same four
    steps on host arrays"""
    import torch
    pts = np.zeros((700, 4), np.float32)
    pts[:, :3] = three_planes()
    pts[:, 3] = np.arange(700)

    def chain(cloud, device):
        with capi.Index(np.zeros((1, 3), np.float32)) as ix:
            rest = ix.plane_removal(cloud, stop_fraction=0.3, with_points=True)[-1]
            assert rest.is_cuda if device else isinstance(rest, np.ndarray)
            n_rest = len(rest)
            ix.set_input(rest)
            labels, ncl, sizes = ix.euclidean_clusters(0.5, 3, 250000, device_out=rest if device else None)
            index, offsets, records = ix.extract_clusters(rest, labels[:n_rest], ncl)
            return [to_numpy(a) for a in (rest, labels[:n_rest], index, offsets, records)] + [ncl, sizes]

    host = chain(pts, False)
    dev = chain(torch.from_numpy(pts).cuda(), True)
    assert host[5] == dev[5] == 11 and len(host[0]) == 96  # (oracle.euclidean_clusters over the 96 remaining points: 11 clusters of 7 ... 3)
    for h, d in zip(host[:5], dev[:5]):
        assert h.shape == d.shape and h.tobytes() == d.tobytes()
    np.testing.assert_array_equal(np.diff(host[3]), host[6][:host[5]])  # the clusters' sizes
    want_index, want_offsets = stable_partition(host[1], host[5])
    np.testing.assert_array_equal(host[2], want_index)
    assert (host[4].view(np.uint32) == host[0][want_index].view(np.uint32)).all()
