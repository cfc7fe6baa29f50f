"""The host scaffold the three "every cloud at once" calls share (csrc/cloud_batch.hpp, the lease and the argument checks in
csrc/entry.hpp, capi._cloud_batch), without a GPU: the header's own test binary; the pieces that used to be copied exist once;
the three Python methods go through the one helper; and a call with TWO bad arguments still returns the status of the check
that came first before the checks were shared."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "pointcloudcomparator_amd" / "csrc"


def test_cloud_batch_header_on_the_cpu():
    """tests/cpp/test_cloud_batch.cpp compiles csrc/cloud_batch.hpp alone: route split, pack, finiteness, upload layouts"""
    subprocess.check_call(["make", "build/test_cloud_batch"], cwd=ROOT)
    r = subprocess.run([str(ROOT / "build" / "test_cloud_batch")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "cloud batch ok" in r.stdout
    header = (CSRC / "cloud_batch.hpp").read_text()
    assert "#include <hip" not in header and "hip_runtime" not in header and "pcc_internal.hpp" not in header
    assert "isfinite" not in header and "(x - x) == 0.0f && (y - y) == 0.0f && (z - z) == 0.0f" in header
    mk = (ROOT / "Makefile").read_text()
    assert re.search(r"^hosttest:.*build/test_cloud_batch", mk, flags=re.M)
    assert re.search(r"^asan:.*build/asan/test_cloud_batch", mk, flags=re.M)
    assert "build/asan/test_cloud_batch: " in mk and "$(SANFLAGS)" in mk.split("build/asan/test_cloud_batch: ", 1)[1].split("\n\n", 1)[0]


def test_the_copied_pieces_exist_once():
    sources = {p.name: p.read_text() for p in sorted(CSRC.iterdir()) if p.suffix in (".hip", ".hpp")}

    def defined(pattern):
        return [name for name, text in sources.items() for _ in re.finditer(pattern, text, flags=re.M)]

    assert defined(r"^\s*(?:static\s+|inline\s+)*size_t\s+align_up\s*\(") == ["cloud_batch.hpp"]
    assert defined(r"\bbool\s+(?:cloud_)?any_finite\s*\(") == ["cloud_batch.hpp"]
    assert len(defined(r"\bstruct\s+Borrow\b")) <= 1
    assert defined(r"\bbool\s+finite3\s*\(") == ["cloud_batch.hpp"]
    # the batch files and the host packs no longer write the test out (the k = 1 kernels of small.hip and flann_order.hip keep theirs)
    open_coded = set(defined(r"\(\s*(\w+(?:\[\d\])?)\s*-\s*\1\s*\)\s*==\s*0(?:\.0?f)?\s*&&"))
    assert "cloud_batch.hpp" in open_coded
    assert not open_coded & {"rift_batch.hip", "sift_batch.hip", "region_rgb_batch.hip", "match_batch.hip", "pack.hip"}
    for name in ("rift_batch.hip", "sift_batch.hip", "region_rgb_batch.hip"):
        text = sources[name]
        assert "check_cloud_batch(" in text and "WorkLease" in text and "batch_routes(" in text and ": BatchStaging" in text, name
    assert "WorkLease" in sources["sift.hip"]


def test_python_batch_methods_share_one_helper():
    from pointcloudcomparator_amd import capi
    src = (ROOT / "pointcloudcomparator_amd" / "capi.py").read_text()
    assert src.count("def _cloud_batch(") == 1
    for fn in ("pcc_rift_descriptors_batch", "pcc_sift_keypoints_batch", "pcc_region_growing_rgb_batch"):
        assert f'_cloud_batch(clouds, rgbs, "{fn}")' in src
    assert src.count("every cloud of a batch must have the same row stride") == 1
    # two row strides in one batch: the same assertion from each method, before the handle is used at all
    wide, narrow = np.zeros((4, 8), np.float32), np.zeros((4, 6), np.float32)
    ix = capi.Index.__new__(capi.Index)  # (no handle: the helper runs first)
    for method in (capi.Index.rift_descriptors_batch, capi.Index.sift_keypoints_batch, capi.Index.region_growing_rgb_batch):
        with pytest.raises(AssertionError, match="every cloud of a batch must have the same row stride, and so every colour array"):
            method(ix, [wide, narrow])
        with pytest.raises(AssertionError, match="one colour array per cloud"):
            method(ix, [wide], [])
        with pytest.raises(AssertionError, match="one colour per point"):
            method(ix, [wide], [np.zeros(3, np.uint32)])


def _entry_points():
    """the three entry points with good default arguments (NULL handle), every argument overridable by keyword"""
    from pointcloudcomparator_amd import capi
    L = capi.LIB
    rec = np.zeros((8, 8), np.float32)  # pcl::PointXYZRGB records: the colour word 16 bytes into each
    rec[:, :3] = np.arange(24, dtype=np.float32).reshape(8, 3) * 0.01
    keep = dict(rec=rec, hist=np.zeros((8, 32), np.float32), idx=np.zeros(8, np.int32), off=np.zeros(2, np.uintp), kp=np.zeros((8, 4), np.float32),
                snap=np.zeros(8, np.int32), labels=np.zeros(8, np.int32), ncl=np.zeros(1, np.int32))
    one_p, one_c, one_n = (C.c_void_p * 1)(rec.ctypes.data), (C.c_void_p * 1)(rec.ctypes.data + 16), (C.c_size_t * 1)(8)
    f32 = C.c_float

    def rift(k=1, p=one_p, n=one_n, stride=32, c=one_c, cstride=32, mem=0, rn=0.03, rg=0.03, rr=0.05, nd=4, ng=8, o1=keep["hist"].ctypes.data,
             o2=keep["idx"].ctypes.data, off=keep["off"].ctypes.data):
        return L.pcc_rift_descriptors_batch(None, k, p, n, stride, c, cstride, mem, rn, rg, rr, nd, ng, o1, o2, off)

    def sift(k=1, p=one_p, n=one_n, stride=32, c=one_c, cstride=32, mem=0, ms=0.005, no=5, ns=5, mc=0.001, r=0.05, o1=keep["kp"].ctypes.data,
             o2=keep["snap"].ctypes.data, cap=8, off=keep["off"].ctypes.data):
        return L.pcc_sift_keypoints_batch(None, k, p, n, stride, c, cstride, mem, ms, no, ns, mc, r, o1, o2, cap, off)

    def rgb(k=1, p=one_p, n=one_n, stride=32, c=one_c, cstride=32, mem=0, dist=10.0, p2p=6.0, r2r=5.0, nn=30, rnn=100, o1=keep["labels"].ctypes.data,
            o2=keep["ncl"].ctypes.data):
        return L.pcc_region_growing_rgb_batch(None, k, p, n, stride, c, cstride, mem, f32(dist), f32(p2p), f32(r2r), 200, 2 ** 31 - 1, nn, rnn, o1, o2)

    nulls = (C.c_void_p * 1)(None)
    big = (C.c_size_t * 1)(2 ** 31)
    return keep, dict(rift=rift, sift=sift, rgb=rgb), nulls, big


# (entry point, two bad arguments) -> the status libpcc_nn returned before the three entry points shared their checks (recorded
# from that library, not from this one).  -1 PCC_ERR_INVALID, -5 PCC_ERR_UNSUPPORTED.  "nulls": one cloud of 8 points whose
# colour pointer is NULL; "big": one cloud of 2^31 points.
TWO_FAULTS = [
    ("rift", dict(mem=1, stride=10), -5),
    ("rift", dict(cstride=6, k=2 ** 31), -1),
    ("rift", dict(off=None, k=2 ** 31), -1),
    ("rift", dict(k=2 ** 31, p=None), -5),
    ("rift", dict(nd=8, c="nulls"), -5),
    ("rift", dict(rr=-1.0, n="big"), -1),
    ("rift", dict(k=0, nd=8), -5),
    ("rift", dict(c="nulls", n="big"), -5),
    ("sift", dict(mem=1, stride=10), -5),
    ("sift", dict(cstride=6, k=2 ** 31), -5),
    ("sift", dict(off=None, k=2 ** 31), -1),
    ("sift", dict(k=2 ** 31, p=None), -5),
    ("sift", dict(ns=14, c="nulls"), -5),
    ("sift", dict(ms=-1.0, n="big"), -1),
    ("sift", dict(ns=14, ms=0.0), -1),
    ("sift", dict(r=-1.0, ns=14), -5),
    ("sift", dict(k=0, ns=14), -5),
    ("sift", dict(c="nulls", n="big"), -5),
    ("rgb", dict(mem=1, stride=10), -5),
    ("rgb", dict(cstride=6, k=2 ** 31), -5),
    ("rgb", dict(o1=None, k=2 ** 31), -5),
    ("rgb", dict(cstride=6, p=None), -1),
    ("rgb", dict(rnn=0, c="nulls"), -5),
    ("rgb", dict(dist=-1.0, n="big"), -1),
    ("rgb", dict(rnn=0, dist=-1.0), -1),
    ("rgb", dict(k=0, rnn=0), -5),
    ("rgb", dict(c="nulls", n="big"), -5),
]


def two_fault_statuses():
    keep, fns, nulls, big = _entry_points()
    named = dict(nulls=nulls, big=big)
    out = []
    for entry, kw, _ in TWO_FAULTS:
        out.append(fns[entry](**{k: named.get(v, v) if isinstance(v, str) else v for k, v in kw.items()}))
    return out


def test_two_bad_arguments_return_the_status_they_always_did():
    got = two_fault_statuses()
    for (entry, kw, want), status in zip(TWO_FAULTS, got):
        assert status == want, (entry, kw, status, want)
    assert {want for _, _, want in TWO_FAULTS} == {-1, -5}
