"""pcc_vfh_descriptors_batch without a GPU (processVHF, reference src/comparator.cpp:482-516, for every cluster in one call):
the entry point and its option are declared, exported and bound; every argument is refused, in the header's order, before the
handle or any device is looked at; the host side of the call (routes, bases, vote items, the caller's bounds, the copy runs,
the offsets' refusals: csrc/range_batch_plan.hpp and csrc/vfh_batch_plan.hpp) holds on the CPU; the new source and binaries are part of the build."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "pointcloudcomparator_amd" / "csrc"
INVALID, UNSUPPORTED = -1, -5  # enum pcc_status


def test_entry_point_and_option_are_declared_exported_and_bound():
    from pointcloudcomparator_amd import capi
    text = (ROOT / "include" / "pcc_nn.h").read_text()
    assert re.search(r"\bint\s+pcc_vfh_descriptors_batch\s*\(\s*pcc_index \*ctx,\s*const void \*pts, size_t stride_bytes,", text)
    assert text.index("int pcc_match_vfh(") < text.index("int pcc_vfh_descriptors_batch(") < text.index("int pcc_sift_keypoints(")
    comment = text[:text.index("int pcc_vfh_descriptors_batch(")].rsplit("/*", 1)[1]
    for what in ("a bad memory space", "offsets that decrease", "a null handle\n *     last", "writes nothing", "never read", "non-finite",
                 "pcc_match_vfh", "before\n *     anything is launched"):
        assert what in comment, what
    assert "After pcc_vfh_descriptors_batch on the handle" in text  # the stats comment
    assert re.search(r"\bPCC_OPT_FPFH_BATCH_BRUTE_MAX = 30,", text) and re.search(r"\bPCC_OPT_VFH_BATCH_BRUTE_MAX = 31\b", text)
    assert capi.OPT_VFH_BATCH_BRUTE_MAX == 31 and capi.OPT_FPFH_BATCH_BRUTE_MAX == 30
    api = (CSRC / "api.hip").read_text()
    assert '{PCC_OPT_VFH_BATCH_BRUTE_MAX, "PCC_VFH_BATCH_BRUTE_MAX", &Options::vfh_batch_brute_max, nullptr, 0, 1073741824' in api
    assert re.search(r"int vfh_batch_brute_max = 8192;", (CSRC / "pcc_internal.hpp").read_text())
    assert "PCC_VFH_BATCH_BRUTE_MAX" in (ROOT / "README.md").read_text()
    assert "pcc_vfh_descriptors_batch" in capi.SYMBOLS
    fn = capi.LIB.pcc_vfh_descriptors_batch  # (the library exports it: ctypes resolves the symbol here)
    assert fn.restype is C.c_int and len(fn.argtypes) == 9
    assert callable(capi.vfh_descriptors_batch) and callable(capi.Index.vfh_descriptors_batch)
    mirror = (ROOT / "include" / "pcc" / "vfh.hpp").read_text()
    assert "processVHFBatch(const std::vector<PointCloud<PointXYZRGB>::Ptr>& clouds" in mirror
    assert re.search(r"std::vector<double> matchVHF\(const std::vector<PointCloud<VFHSignature308>::Ptr>& d1,", mirror)


def test_arguments_are_refused_in_order_without_a_device():
    """every refusal happens with a NULL handle -- nothing of it can have looked at a device -- and each call carries, besides
    the fault it is refused for, every fault that comes LATER in the order: the earlier one is the one reported"""
    from pointcloudcomparator_amd import capi
    L = capi.LIB
    rec = np.zeros((8, 8), np.float32)
    offs = (C.c_size_t * 3)(0, 5, 8)
    hist, out = np.zeros((2, 308), np.float32), np.full(3, 99, np.uintp)

    def call(p=rec.ctypes.data, stride=32, o=offs, k=2, mem=0, rn=0.03, h=hist.ctypes.data, oo=out.ctypes.data, ctx=None):
        return L.pcc_vfh_descriptors_batch(ctx, p, stride, o, k, mem, rn, h, oo)

    def err():
        return L.pcc_last_error()

    decreasing = (C.c_size_t * 3)(0, 5, 4)
    later = dict(rn=0.0)  # fault 5, beside a null handle (6)
    # 1. the memory space, in front of everything else
    assert call(mem=7, p=None, stride=10, o=decreasing, **later) == INVALID and b"mem space" in err()
    # 2. null arrays, in front of the stride, the offsets and the radius
    for kw in (dict(o=None), dict(oo=None), dict(p=None), dict(h=None)):
        assert call(stride=10, **later, **kw) == INVALID and b"null argument" in err(), kw
    assert call(p=None, o=decreasing, stride=10) == INVALID and b"null argument" in err()
    # 3. the stride and the alignment, in front of the offsets and the radius
    for stride in (0, 8, 10, 30):
        assert call(stride=stride, o=decreasing, **later) == INVALID and b"stride" in err(), stride
    for kw in (dict(p=rec.ctypes.data + 2), dict(h=hist.ctypes.data + 1)):
        assert call(o=decreasing, **later, **kw) == INVALID and b"4-byte aligned" in err(), kw
    for mem in (capi.MEM_HOST, capi.MEM_DEVICE):  # (either space: nothing is read)
        assert call(mem=mem, stride=10) == INVALID and b"stride" in err()
    # 4. the offsets: a decrease (in front of the size), then 2^31 points -- in front of the radius
    assert call(o=decreasing, **later) == INVALID and b"offsets must not decrease (cluster 1)" in err()
    assert call(o=(C.c_size_t * 3)(0, 2 ** 31, 2 ** 31 - 1), **later) == INVALID and b"must not decrease" in err()
    assert call(o=(C.c_size_t * 3)(0, 2 ** 30, 2 ** 31), **later) == UNSUPPORTED and b"2^31" in err()
    assert call(o=(C.c_size_t * 3)(7, 7, 7 + 2 ** 31), rn=0.0) == UNSUPPORTED and b"2^31" in err()
    # 5. the radius
    for rn in (0.0, -0.03, float("nan"), float("inf")):
        assert call(rn=rn) == INVALID and b"bad radius" in err(), rn
    # 6. all arguments good: the handle is looked at last
    assert call() == INVALID and b"null index" in err()
    assert out.tolist() == [99, 99, 99] and not hist.any()  # nothing was written by any refused call
    # no cluster at all: PCC_OK, one offset, no device -- no array but the offsets is needed; the radius is still checked
    assert call(k=0) == 0 and out.tolist() == [0, 99, 99]
    out[:] = 99
    assert call(k=0, p=None, h=None) == 0 and out.tolist() == [0, 99, 99]
    out[:] = 99
    assert call(k=0, rn=0.0) == INVALID and b"bad radius" in err() and out.tolist() == [99, 99, 99]
    # clusters without a point need no arrays either, but they do need a handle
    assert call(o=(C.c_size_t * 3)(4, 4, 4), p=None, h=None) == INVALID and b"null index" in err()
    assert out.tolist() == [99, 99, 99]


def test_host_side_of_the_call_holds_on_the_cpu():
    """tests/cpp/test_vfh_batch_plan.cpp compiles csrc/vfh_batch_plan.hpp, the header vfh_batch.hip plans its call with"""
    subprocess.check_call(["make", "build/test_vfh_batch_plan"], cwd=ROOT)
    r = subprocess.run([str(ROOT / "build" / "test_vfh_batch_plan")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "vfh batch plan ok: 17 cases" in r.stdout, r.stdout + r.stderr
    src = (ROOT / "tests" / "cpp" / "test_vfh_batch_plan.cpp").read_text()
    for what in ("limit - 1, limit, limit + 1", "sizes 0, 1, 2", "alternating routes", "is on the wrong route", "not the prefix sum of (n >= 2)",
                 "not in exactly one vote item", "a vote item crosses its cluster", "not copied exactly once", "not in cluster order",
                 "limit 0", "2^31 points are not refused"):
        assert what in src, what
    hip = (CSRC / "vfh_batch.hip").read_text()
    assert '#include "vfh_batch_plan.hpp"' in hip
    # (the offsets' check moved to the range-batch scaffold: the name is followed to where it is used now)
    for used in ("vfh_batch_plan(", "check_range_batch(", "plan.copies", "plan.votes", "plan.route", "plan.out_offsets"):
        assert used in hip, used
    assert "check_cluster_offsets(" in (CSRC / "range_batch.hip").read_text()  # check_range_batch's fourth check
    assert "check_scene_offsets(" in (CSRC / "entry.hpp").read_text() and "check_range_offsets(" in (CSRC / "range_batch_plan.hpp").read_text()
    for name in ("vfh_batch_plan.hpp", "range_batch_plan.hpp"):
        plan = (CSRC / name).read_text()
        assert "hip_runtime" not in plan and "__global__" not in plan, name  # plain C++


def test_one_chain_body_and_no_float_atomic():
    """the single call and the batch call run ONE body of the centroid chains; the new kernels add integers only"""
    dev = (CSRC / "vfh_device.hpp").read_text()
    assert dev.count("void vfh_centroid_chains(") == 1 and "VFH_CENT_ROWS = 8" in dev and "VFH_CENT_TILE = 64 * VFH_CENT_ROWS" in dev
    for name in ("vfh.hip", "vfh_batch.hip"):
        text = (CSRC / name).read_text()
        assert '#include "vfh_device.hpp"' in text and text.count("vfh_centroid_chains(") >= 1, name
        assert "park[" not in text, f"{name} keeps a copy of the chain body"
    batch = (CSRC / "vfh_batch.hip").read_text()
    for kernel in ("k_vfh_batch_centroids", "k_vfh_batch_votes", "k_vfh_batch_finish"):
        assert kernel in batch
    assert "vfh_vote(" in batch and "vfh_bin_value(" in batch
    shared = (CSRC / "range_batch.hip").read_text()  # the pack kernel and its flag word live with the range-batch scaffold
    assert "stage_ranges(" in batch and "atomicMin(" in shared and "k_range_pack" in shared
    code = re.sub(r"//.*", "", batch)
    assert "atomicAdd(" in code and not re.search(r"atomicAdd\([^;]*\b\d*\.\d*f\b", code) and "unsafeAtomicAdd" not in code
    shared_code = re.sub(r"//.*", "", shared)  # no float atomic there either: the one atomic is the integer minimum
    assert "atomicAdd(" not in shared_code and "unsafeAtomic" not in shared_code and shared_code.count("atomic") == 1
    assert "VFH_BATCH_VOTE_POINTS = 1024" in (CSRC / "vfh_batch_plan.hpp").read_text()


def test_new_source_and_binaries_are_in_the_makefile():
    mk = (ROOT / "Makefile").read_text()
    hip_srcs = re.search(r"^HIP_SRCS\s*:=(.*)$", mk, flags=re.M).group(1)
    assert "vfh_batch.hip" in hip_srcs
    assert re.search(r"^hosttest:.*build/test_vfh_batch_plan.*build/vfh_batch_driver", mk, flags=re.M)
    assert re.search(r"^asan:.*build/asan/test_vfh_batch_plan", mk, flags=re.M)
    assert "ASAN_OPTIONS=detect_leaks=1 build/asan/test_vfh_batch_plan" in mk
    assert re.search(r"^build/vfh_batch_driver: tests/cpp/vfh_batch_driver.cpp include/pcc/vfh.hpp", mk, flags=re.M)
