"""pcc_rift_descriptors_batch without a GPU (the reference's per-cluster descriptor loop, src/comparator.cpp:1224-1272, each
turn processRIFT, :590-684): the entry point is declared, exported and bound; every argument is refused before the handle or
any device is looked at; the host-built table of work items covers every (cloud, query) exactly once; the new source is part
of the library."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def test_entry_point_is_declared_exported_bound_and_cites_the_reference():
    from pointcloudcomparator_amd import capi
    text = (ROOT / "include" / "pcc_nn.h").read_text()
    assert re.search(r"\bint\s+pcc_rift_descriptors_batch\s*\(\s*pcc_index \*ctx, size_t n_clouds,", text)
    comment = text[:text.index("int pcc_rift_descriptors_batch(")].rsplit("/*", 1)[1]
    assert "src/comparator.cpp:1224-1272" in comment and ":590-684" in comment
    assert "pcc_rift_descriptors_batch" in capi.SYMBOLS
    fn = capi.LIB.pcc_rift_descriptors_batch
    assert fn.restype is C.c_int and len(fn.argtypes) == 16
    assert callable(capi.rift_descriptors_batch) and callable(capi.Index.rift_descriptors_batch)
    # the option: its number in the header and in the binding; the one before it keeps its line
    assert re.search(r"\bPCC_OPT_SIFT_LAYOUT = 25,", text)
    assert re.search(r"\bPCC_OPT_RIFT_BATCH_BRUTE_MAX = 26\b", text)
    assert capi.OPT_RIFT_BATCH_BRUTE_MAX == 26 and capi.OPT_SIFT_LAYOUT == 25
    assert "PCC_RIFT_BATCH_BRUTE_MAX" in (ROOT / "pointcloudcomparator_amd" / "csrc" / "api.hip").read_text()
    stats = text[:text.index("int pcc_index_stats(")].rsplit("/*", 1)[1]
    assert "pcc_rift_descriptors_batch" in stats and "work handle" in stats
    mirror = (ROOT / "include" / "pcc" / "rift.hpp").read_text()
    assert "processRIFTBatch(const std::vector<PointCloud<PointXYZRGB>::Ptr>& clouds" in mirror and "src/comparator.cpp:1224-1272" in mirror


def test_arguments_are_refused_without_a_device():
    """every refusal below happens with a NULL handle: nothing of it can have looked at a device"""
    from pointcloudcomparator_amd import capi
    L = capi.LIB
    rec = np.zeros((8, 8), np.float32)  # pcl::PointXYZRGB records: the colour word 16 bytes into each
    one_p, one_c, one_n = (C.c_void_p * 1)(rec.ctypes.data), (C.c_void_p * 1)(rec.ctypes.data + 16), (C.c_size_t * 1)(8)
    nulls = (C.c_void_p * 1)(None)
    hist, idx, off = np.zeros((8, 32), np.float32), np.zeros(8, np.int32), np.full(2, 99, np.uintp)

    def call(k=1, p=one_p, n=one_n, stride=32, c=one_c, cstride=32, mem=0, rn=0.03, rg=0.03, rr=0.05, nd=4, ng=8, h=hist.ctypes.data,
             i=idx.ctypes.data, o=off.ctypes.data, ctx=None):
        return L.pcc_rift_descriptors_batch(ctx, k, p, n, stride, c, cstride, mem, rn, rg, rr, nd, ng, h, i, o)

    def err():
        return L.pcc_last_error()

    assert call(mem=7) == -1 and b"mem space" in err()
    assert call(mem=capi.MEM_DEVICE) == -5 and b"PCC_MEM_HOST" in err()
    for kw in (dict(p=None), dict(n=None), dict(c=None), dict(h=None), dict(i=None), dict(o=None)):
        assert call(**kw) == -1 and b"null" in err() and b"null index" not in err(), kw
    assert call(p=nulls) == -1 and b"null point pointer" in err()
    assert call(c=nulls) == -1 and b"null colour pointer" in err()
    for stride in (0, 8, 10, 30):
        assert call(stride=stride) == -1 and b"stride" in err(), stride
    for kw in (dict(cstride=0), dict(cstride=6), dict(c=(C.c_void_p * 1)(rec.ctypes.data + 18)), dict(p=(C.c_void_p * 1)(rec.ctypes.data + 2))):
        assert call(**kw) == -1 and b"4-byte aligned" in err(), kw
    for kw in (dict(rn=0.0), dict(rg=-0.03), dict(rr=float("nan")), dict(rr=float("inf"))):
        assert call(**kw) == -1 and b"bad radius" in err(), kw
    for nd, ng in ((8, 4), (4, 4), (2, 16), (1, 32), (0, 8), (5, 8)):  # nd * ng == 32 included
        assert call(nd=nd, ng=ng) == -5 and b"only 4 distance x 8 gradient bins" in err(), (nd, ng)
    # totals from 2^31 on (nothing is read: the sizes alone decide)
    two_p = (C.c_void_p * 2)(rec.ctypes.data, rec.ctypes.data)
    two_c = (C.c_void_p * 2)(rec.ctypes.data + 16, rec.ctypes.data + 16)
    assert call(k=2, p=two_p, c=two_c, n=(C.c_size_t * 2)(2 ** 30, 2 ** 30)) == -5 and b"2^31" in err()
    assert call(n=(C.c_size_t * 1)(2 ** 31)) == -5 and b"2^31" in err()
    assert call() == -1 and b"null index" in err()  # all arguments good: the handle is looked at last
    assert off.tolist() == [99, 99] and not hist.any() and not idx.any()  # nothing was written by any refused call
    # no cloud at all: PCC_OK, one offset, no device -- no array but the offsets is needed
    assert call(k=0) == 0 and off.tolist() == [0, 99]
    off[:] = 99
    assert call(k=0, p=None, n=None, c=None, h=None, i=None) == 0 and off.tolist() == [0, 99]
    assert call(k=0, o=None) == -1 and b"null out_offsets" in err()


def test_work_item_table_covers_every_query_once():
    """tests/cpp/test_rift_batch_plan.cpp compiles csrc/rift_batch_plan.hpp, the header rift_batch.hip builds its table with:
    sizes around the largest query block and the 2048-point LDS tile, empty clouds in front and in the middle; batches small
    and large enough for every choice of the block"""
    subprocess.check_call(["make", "build/test_rift_batch_plan"], cwd=ROOT)
    exe = str(ROOT / "build" / "test_rift_batch_plan")
    # (sizes, the query block the table must choose: 64 halved while fewer than 1024 items would come of it)
    for sizes, block in (([0, 1, 64, 65, 2048, 2049, 0, 700], 4), ([300] * 60, 16), ([700] * 100, 64), ([0, 65536, 1, 0], 64),
                         ([3] * 7, 4)):
        r = subprocess.run([exe] + [str(v) for v in sizes], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        items = sum((v + block - 1) // block for v in sizes)
        assert f"rift batch plan ok: {len(sizes)} clouds, {sum(sizes)} points, {items} items of up to {block} queries, tile 2048" in r.stdout
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)  # its own default: the first set above
    assert r.returncode == 0 and "8 clouds, 4927 points" in r.stdout
    src = (ROOT / "tests" / "cpp" / "test_rift_batch_plan.cpp").read_text()
    for what in ("not covered exactly once", "cross the end of its cloud", "not the prefix sum"):
        assert what in src
    assert '#include "rift_batch_plan.hpp"' in (ROOT / "pointcloudcomparator_amd" / "csrc" / "rift_batch.hip").read_text()


def test_new_source_and_binaries_are_in_the_makefile():
    mk = (ROOT / "Makefile").read_text()
    hip_srcs = re.search(r"^HIP_SRCS\s*:=(.*)$", mk, flags=re.M).group(1)
    assert "rift_batch.hip" in hip_srcs
    assert re.search(r"^hosttest:.*build/sift_driver.*build/test_rift_batch_plan.*build/rift_batch_driver", mk, flags=re.M)
