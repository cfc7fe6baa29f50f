"""pcc_region_growing_rgb_batch without a GPU (the reference's two color_growing_segmentation calls per accepted match,
src/comparator.cpp:1456-1495 and src/segmentation.cpp:161-216, for every match at once): the entry point and its option are
declared, exported and bound; every argument is refused before the handle or any device is looked at; no cloud at all is
PCC_OK; the host half cuts a concatenation's segments and pairs per cloud as the single path would; the new source is part of
the library and shares its kernels instead of copying them."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "pointcloudcomparator_amd" / "csrc"


def test_entry_point_and_option_are_declared_exported_and_bound():
    from pointcloudcomparator_amd import capi
    text = (ROOT / "include" / "pcc_nn.h").read_text()
    assert re.search(r"\bint\s+pcc_region_growing_rgb_batch\s*\(\s*pcc_index \*ctx, size_t n_clouds,", text)
    comment = text[:text.index("int pcc_region_growing_rgb_batch(")].rsplit("/*", 1)[1]
    assert "src/comparator.cpp:1456-1495" in comment and "src/segmentation.cpp:161-216" in comment
    assert "PCC_ERR_EMPTY" in comment and "split" in comment and "PCC_OPT_RGB_BATCH_BRUTE_MAX" in comment
    assert re.search(r"\bPCC_OPT_SIFT_BATCH_BRUTE_MAX = 27,", text)  # the one before it keeps its number
    assert re.search(r"\bPCC_OPT_RGB_BATCH_BRUTE_MAX = 28\b", text)
    assert capi.OPT_RGB_BATCH_BRUTE_MAX == 28 and capi.OPT_SIFT_BATCH_BRUTE_MAX == 27
    assert "PCC_RGB_BATCH_BRUTE_MAX" in (CSRC / "api.hip").read_text()
    assert "pcc_region_growing_rgb_batch" in capi.SYMBOLS
    fn = capi.LIB.pcc_region_growing_rgb_batch  # (raises when the library does not export it)
    assert fn.restype is C.c_int and len(fn.argtypes) == 17
    assert callable(capi.Index.region_growing_rgb_batch) and callable(capi.region_growing_rgb_batch)
    stats = text[:text.index("int pcc_index_stats(")].rsplit("/*", 1)[1]
    assert "pcc_region_growing_rgb_batch" in stats and "[3] points of the" in stats


def test_arguments_are_refused_without_a_device():
    """every refusal below happens with a NULL handle: nothing of it can have looked at a device"""
    from pointcloudcomparator_amd import capi
    L = capi.LIB
    rec = np.zeros((8, 8), np.float32)  # pcl::PointXYZRGB records: the colour word 16 bytes into each
    rec[:, :3] = np.arange(24, dtype=np.float32).reshape(8, 3) * 0.01
    one_p, one_c, one_n = (C.c_void_p * 1)(rec.ctypes.data), (C.c_void_p * 1)(rec.ctypes.data + 16), (C.c_size_t * 1)(8)
    nulls = (C.c_void_p * 1)(None)
    labels, ncl = np.full(8, 77, np.int32), np.full(1, 77, np.int32)
    f32 = C.c_float

    def call(k=1, p=one_p, n=one_n, stride=32, c=one_c, cstride=32, mem=0, dist=10.0, p2p=6.0, r2r=5.0, mn=200, mx=2 ** 31 - 1, nn=30, rnn=100,
             o_l=labels.ctypes.data, o_n=ncl.ctypes.data, ctx=None):
        return L.pcc_region_growing_rgb_batch(ctx, k, p, n, stride, c, cstride, mem, f32(dist), f32(p2p), f32(r2r), mn, mx, nn, rnn, o_l, o_n)

    def err():
        return L.pcc_last_error()

    assert call(mem=7) == -1 and b"mem space" in err()
    assert call(mem=capi.MEM_DEVICE) == -5 and b"PCC_MEM_HOST" in err()
    for kw in (dict(p=None), dict(n=None), dict(c=None), dict(o_l=None), dict(o_n=None)):
        assert call(**kw) == -1 and b"null" in err() and b"null index" not in err(), kw
    assert call(p=nulls) == -1 and b"null point pointer" in err()
    assert call(c=nulls) == -1 and b"null colour pointer" in err()
    for stride in (0, 8, 10, 30):
        assert call(stride=stride) == -1 and b"stride" in err(), stride
    for kw in (dict(cstride=0), dict(cstride=6), dict(c=(C.c_void_p * 1)(rec.ctypes.data + 18)), dict(p=(C.c_void_p * 1)(rec.ctypes.data + 2)),
               dict(o_l=labels.ctypes.data + 2), dict(o_n=ncl.ctypes.data + 2)):
        assert call(**kw) == -1 and b"4-byte aligned" in err(), kw
    # the thresholds and neighbour counts, with the single call's messages
    for name in ("dist", "p2p", "r2r"):
        for bad in (-1.0, float("nan"), float("inf")):
            assert call(**{name: bad}) == -1 and b"bad threshold" in err(), (name, bad)
    for kw in (dict(nn=0), dict(rnn=0), dict(rnn=capi.KNN_MAX_K + 1)):
        assert call(**kw) == -5 and b"both must be at least 1, the region neighbours at most" in err(), kw
    # totals from 2^31 on (nothing is read: the sizes alone decide)
    two_p = (C.c_void_p * 2)(rec.ctypes.data, rec.ctypes.data)
    two_c = (C.c_void_p * 2)(rec.ctypes.data + 16, rec.ctypes.data + 16)
    assert call(k=2, p=two_p, c=two_c, n=(C.c_size_t * 2)(2 ** 30, 2 ** 30)) == -5 and b"2^31" in err()
    assert call(n=(C.c_size_t * 1)(2 ** 31)) == -5 and b"2^31" in err()
    # an empty cloud needs neither pointer
    assert call(k=2, p=(C.c_void_p * 2)(None, rec.ctypes.data), c=(C.c_void_p * 2)(None, rec.ctypes.data + 16), n=(C.c_size_t * 2)(0, 8)) == -1 \
        and b"null index" in err()
    assert call() == -1 and b"null index" in err()  # all arguments good: the handle is looked at last
    assert (labels == 77).all() and (ncl == 77).all()  # nothing was written by any refused call
    # no cloud at all: PCC_OK, no device, no array needed
    assert call(k=0) == 0
    assert call(k=0, p=None, n=None, c=None, o_l=None, o_n=None) == 0
    assert (labels == 77).all() and (ncl == 77).all()


def test_the_split_gives_every_cloud_what_it_gets_alone():
    """tests/cpp/test_rgb_batch_split.cpp compiles csrc/rgb_batch_split.hpp, the header region_rgb_batch.hip cuts its segments and
    pairs with: clouds of one segment, without a pair and without a segment in the middle of a shuffled concatenation"""
    subprocess.check_call(["make", "build/test_rgb_batch_split"], cwd=ROOT)
    r = subprocess.run([str(ROOT / "build" / "test_rgb_batch_split")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "rgb batch split ok" in r.stdout
    mixed = [ln for ln in r.stdout.splitlines() if ln.startswith("mixed-min1 ")]
    assert mixed and all("8 clouds" in ln and "2 without a segment" in ln and "2 clouds of one segment" in ln for ln in mixed)
    src = (ROOT / "tests" / "cpp" / "test_rgb_batch_split.cpp").read_text()
    for what in ("the split differs from the cloud alone", "a pair between two clouds was accepted", "short id ranges accepted"):
        assert what in src
    header = (CSRC / "rgb_batch_split.hpp").read_text()
    assert "#include <hip" not in header and "hip_runtime" not in header and "pcc_internal.hpp" not in header
    assert '#include "rgb_batch_split.hpp"' in (CSRC / "region_rgb_batch.hip").read_text()


def test_new_source_and_binaries_are_in_the_makefile():
    mk = (ROOT / "Makefile").read_text()
    hip_srcs = re.search(r"^HIP_SRCS\s*:=(.*)$", mk, flags=re.M).group(1)
    assert "region_rgb_batch.hip" in hip_srcs
    assert re.search(r"^hosttest:.*build/test_rgb_batch_split", mk, flags=re.M)
    assert re.search(r"^asan:.*build/asan/test_rgb_batch_split", mk, flags=re.M)
    # the stage kernels, the merge network and the work items are shared, not copied
    batch = (CSRC / "region_rgb_batch.hip").read_text()
    single = (CSRC / "region_rgb.hip").read_text()
    assert "rgb_stages(" in batch and "rift_batch_plan(" in batch and "topk_merge<KR>" in batch
    for kernel in ("k_rgb_prepare", "k_rgb_link", "k_rgb_flatten", "k_rgb_sweep", "k_rgb_seed_flags", "k_rgb_segment_ids", "k_rgb_stats",
                   "k_rgb_pairs", "k_rgb_compact_pairs", "k_rgb_label"):
        assert kernel in single and kernel not in batch, kernel
    knn = (CSRC / "knn.hip").read_text()
    assert '#include "knn_merge.hpp"' in knn and '#include "knn_merge.hpp"' in batch
    assert "void topk_merge(" not in knn and "void topk_merge(" in (CSRC / "knn_merge.hpp").read_text()
    assert "struct RiftBatchItem {" not in batch
