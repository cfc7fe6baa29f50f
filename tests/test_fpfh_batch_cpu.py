"""pcc_fpfh_descriptors_batch without a GPU (processFPFH, reference src/comparator.cpp:824-875, for every cluster in one call):
the entry point and its option are declared, exported and bound; every argument is refused, in the header's order, before the
handle or any device is looked at; the host side of the call (routes, bases, work items, the output splice, the offsets'
refusals: csrc/range_batch_plan.hpp and csrc/fpfh_batch_plan.hpp) holds on the CPU; the new source and binaries are part of the build."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
INVALID, UNSUPPORTED = -1, -5  # enum pcc_status


def test_entry_point_and_option_are_declared_exported_and_bound():
    from pointcloudcomparator_amd import capi
    text = (ROOT / "include" / "pcc_nn.h").read_text()
    assert re.search(r"\bint\s+pcc_fpfh_descriptors_batch\s*\(\s*pcc_index \*ctx,\s*const void \*pts, size_t stride_bytes,", text)
    assert text.index("int pcc_fpfh_descriptors(") < text.index("int pcc_fpfh_descriptors_batch(") < text.index("int pcc_sift_keypoints(")
    comment = text[:text.index("int pcc_fpfh_descriptors_batch(")].rsplit("/*", 1)[1]
    for what in ("a bad memory space", "offsets that decrease", "a null handle\n *     last", "writes nothing", "ONE CSR", "pcc_match_fpfh_batch"):
        assert what in comment, what
    assert re.search(r"\bPCC_OPT_FPFH_LAYOUT = 29,", text) and re.search(r"\bPCC_OPT_FPFH_BATCH_BRUTE_MAX = 30\b", text)
    assert capi.OPT_FPFH_BATCH_BRUTE_MAX == 30 and capi.OPT_FPFH_LAYOUT == 29
    api = (ROOT / "pointcloudcomparator_amd" / "csrc" / "api.hip").read_text()
    assert '{PCC_OPT_FPFH_BATCH_BRUTE_MAX, "PCC_FPFH_BATCH_BRUTE_MAX", &Options::fpfh_batch_brute_max' in api
    assert "PCC_FPFH_BATCH_BRUTE_MAX" in (ROOT / "README.md").read_text()
    assert "pcc_fpfh_descriptors_batch" in capi.SYMBOLS
    fn = capi.LIB.pcc_fpfh_descriptors_batch  # (the library exports it: ctypes resolves the symbol here)
    assert fn.restype is C.c_int and len(fn.argtypes) == 14
    assert callable(capi.fpfh_descriptors_batch) and callable(capi.Index.fpfh_descriptors_batch)
    mirror = (ROOT / "include" / "pcc" / "fpfh.hpp").read_text()
    assert "processFPFHBatch(const std::vector<PointCloud<PointXYZRGB>::Ptr>& clouds" in mirror


def test_arguments_are_refused_in_order_without_a_device():
    """every refusal happens with a NULL handle -- nothing of it can have looked at a device -- and each call carries, besides
    the fault it is refused for, every fault that comes LATER in the order: the earlier one is the one reported"""
    from pointcloudcomparator_amd import capi
    L = capi.LIB
    rec = np.zeros((8, 8), np.float32)
    offs = (C.c_size_t * 3)(0, 5, 8)
    hist, idx, out = np.zeros((8, 33), np.float32), np.zeros(8, np.int32), np.full(3, 99, np.uintp)

    def call(p=rec.ctypes.data, stride=32, o=offs, k=2, mem=0, rn=0.03, rf=0.05, bins=(11, 11, 11), h=hist.ctypes.data, i=idx.ctypes.data,
             oo=out.ctypes.data, ctx=None):
        return L.pcc_fpfh_descriptors_batch(ctx, p, stride, o, k, mem, rn, rf, bins[0], bins[1], bins[2], h, i, oo)

    def err():
        return L.pcc_last_error()

    decreasing = (C.c_size_t * 3)(0, 5, 4)
    later = dict(bins=(11, 11, 12), rn=0.0)  # faults 5, beside a null handle (6)
    # 1. the memory space, in front of everything else
    assert call(mem=7, p=None, stride=10, o=decreasing, **later) == INVALID and b"mem space" in err()
    # 2. null arrays, in front of the stride, the offsets and the parameters
    for kw in (dict(o=None), dict(oo=None), dict(p=None), dict(h=None), dict(i=None)):
        assert call(stride=10, **later, **kw) == INVALID and b"null argument" in err(), kw
    assert call(p=None, o=decreasing, stride=10) == INVALID and b"null argument" in err()
    # 3. the stride and the alignment, in front of the offsets and the parameters
    for stride in (0, 8, 10, 30):
        assert call(stride=stride, o=decreasing, **later) == INVALID and b"stride" in err(), stride
    for kw in (dict(p=rec.ctypes.data + 2), dict(h=hist.ctypes.data + 1), dict(i=idx.ctypes.data + 2)):
        assert call(o=decreasing, **later, **kw) == INVALID and b"4-byte aligned" in err(), kw
    for mem in (capi.MEM_HOST, capi.MEM_DEVICE):  # (either space: nothing is read)
        assert call(mem=mem, stride=10) == INVALID and b"stride" in err()
    # 4. the offsets: a decrease (in front of the size), then 2^31 points -- in front of the parameters
    assert call(o=decreasing, **later) == INVALID and b"offsets must not decrease (cluster 1)" in err()
    assert call(o=(C.c_size_t * 3)(0, 2 ** 31, 2 ** 31 - 1), **later) == INVALID and b"must not decrease" in err()
    assert call(o=(C.c_size_t * 3)(0, 2 ** 30, 2 ** 31), **later) == UNSUPPORTED and b"2^31" in err()
    assert call(o=(C.c_size_t * 3)(7, 7, 7 + 2 ** 31), rn=0.0) == UNSUPPORTED and b"2^31" in err()
    # 5. the radii, then the bins, with pcc_fpfh_descriptors' messages
    for kw in (dict(rn=0.0), dict(rf=-0.05), dict(rf=float("nan")), dict(rn=float("inf"))):
        assert call(bins=(11, 11, 12), **kw) == INVALID and b"bad radius" in err(), kw
    for bins in ((11, 11, 12), (33, 0, 0), (10, 11, 11), (0, 0, 0)):
        assert call(bins=bins) == UNSUPPORTED and b"only 11 + 11 + 11 bins are built" in err(), bins
    # 6. all arguments good: the handle is looked at last
    assert call() == INVALID and b"null index" in err()
    assert out.tolist() == [99, 99, 99] and not hist.any() and not idx.any()  # nothing was written by any refused call
    # no cluster at all: PCC_OK, one offset, no device -- no array but the offsets is needed; its parameters are still checked
    assert call(k=0) == 0 and out.tolist() == [0, 99, 99]
    out[:] = 99
    assert call(k=0, p=None, h=None, i=None) == 0 and out.tolist() == [0, 99, 99]
    out[:] = 99
    assert call(k=0, rn=0.0) == INVALID and b"bad radius" in err() and out.tolist() == [99, 99, 99]
    # clusters without a point need no arrays either, but they do need a handle
    assert call(o=(C.c_size_t * 3)(4, 4, 4), p=None, h=None, i=None) == INVALID and b"null index" in err()


def test_host_side_of_the_call_holds_on_the_cpu():
    """tests/cpp/test_fpfh_batch_plan.cpp compiles csrc/fpfh_batch_plan.hpp, the header fpfh_batch.hip plans its call with"""
    subprocess.check_call(["make", "build/test_fpfh_batch_plan"], cwd=ROOT)
    r = subprocess.run([str(ROOT / "build" / "test_fpfh_batch_plan")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "fpfh batch plan ok: 13 cases" in r.stdout, r.stdout + r.stderr
    src = (ROOT / "tests" / "cpp" / "test_fpfh_batch_plan.cpp").read_text()
    for what in ("limit - 1, limit, limit + 1", "is on the wrong route", "not the prefix sum", "an output row is written twice",
                 "not copied exactly once", "not in cluster order", "2^31 points are not refused", "{0, 0, 5, 0, 0, 64, 65, 0}"):
        assert what in src, what
    csrc = ROOT / "pointcloudcomparator_amd" / "csrc"
    hip = (csrc / "fpfh_batch.hip").read_text()
    assert '#include "fpfh_batch_plan.hpp"' in hip
    # the routes and the offsets' check moved to the range-batch scaffold: each name is followed to where it is used now
    for used in ("range_batch_plan(", "fpfh_batch_splice(", "check_range_batch("):
        assert used in hip, used
    assert '#include "range_batch_plan.hpp"' in (csrc / "fpfh_batch_plan.hpp").read_text()
    assert "check_cluster_offsets(" in (csrc / "range_batch.hip").read_text()  # check_range_batch's fourth check
    assert "check_scene_offsets(" in (csrc / "entry.hpp").read_text() and "check_range_offsets(" in (csrc / "range_batch_plan.hpp").read_text()


def test_new_source_and_binaries_are_in_the_makefile():
    mk = (ROOT / "Makefile").read_text()
    hip_srcs = re.search(r"^HIP_SRCS\s*:=(.*)$", mk, flags=re.M).group(1)
    assert "fpfh_batch.hip" in hip_srcs
    assert re.search(r"^hosttest:.*build/test_fpfh_batch_plan.*build/fpfh_batch_driver", mk, flags=re.M)
    assert re.search(r"^asan:.*build/asan/test_fpfh_batch_plan", mk, flags=re.M)
    assert "ASAN_OPTIONS=detect_leaks=1 build/asan/test_fpfh_batch_plan" in mk
