"""pcc_region_growing_rgb without a GPU (reference src/segmentation.cpp:161-216, color_growing_segmentation): the entry point
is declared, exported and bound; its arguments are refused before any device is touched; the host half (csrc/rgb_merge.hpp)
agrees with the oracle, plain and under ASan + UBSan (make test-rgb-merge); and the order-free statement the kernels rest on
-- the segment of a point is the lowest index that reaches it along valid edges -- reproduces the oracle's queue."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle
import rgb_device_util as util

ROOT = Path(__file__).resolve().parent.parent


def test_entry_point_is_declared_exported_bound_and_cites_the_reference():
    from pointcloudcomparator_amd import capi
    text = (ROOT / "include" / "pcc_nn.h").read_text()
    assert re.search(r"\bint pcc_region_growing_rgb\(pcc_index \*index, const void \*rgb, size_t rgb_stride_bytes, int mem,", text)
    comment = text[:text.index("int pcc_region_growing_rgb(")].rsplit("/*", 1)[1]
    assert "src/segmentation.cpp:161-216" in comment and "RegionGrowingRGB" in comment
    assert "pcc_region_growing_rgb" in capi.SYMBOLS and hasattr(capi.LIB, "pcc_region_growing_rgb")
    assert callable(capi.Index.region_growing_rgb)
    mk = (ROOT / "Makefile").read_text()
    hip_srcs = re.search(r"^HIP_SRCS\s*:=(.*)$", mk, flags=re.M).group(1)
    assert "region_rgb.hip" in hip_srcs
    merge = (ROOT / "pointcloudcomparator_amd" / "csrc" / "rgb_merge.hpp").read_text()
    assert not any("hip" in inc.lower() for inc in re.findall(r"#include\s*[<\"]([^>\"]+)", merge)), "the host half includes no HIP header"
    mirror = (ROOT / "include" / "pcc" / "region_growing_rgb.hpp").read_text()
    assert "setDeviceSegmentation(bool" in mirror and "color_growing_segmentation_device" in mirror


def test_arguments_are_refused_without_a_device():
    """every refusal below happens with a NULL handle: nothing of it can have looked at a device; nothing is written"""
    from pointcloudcomparator_amd import capi
    L = capi.LIB
    rgb = np.zeros(8, np.uint32)
    labels = np.full(8, 77, np.int32)
    ncl = ctypes.c_int32(77)

    def call(rgb_p=rgb.ctypes.data, stride=4, mem=0, dist=10.0, p2p=6.0, r2r=5.0, mn=200, mx=2**31 - 1, nn=30, rnn=100,
             lab=labels.ctypes.data, nc=ctypes.byref(ncl)):
        return L.pcc_region_growing_rgb(None, rgb_p, stride, mem, dist, p2p, r2r, mn, mx, nn, rnn, lab, nc)

    assert call(mem=7) == -1 and b"mem space" in L.pcc_last_error()
    for kw in (dict(rgb_p=None), dict(lab=None), dict(nc=None)):
        assert call(**kw) == -1 and b"null argument" in L.pcc_last_error(), kw
    for kw in (dict(stride=0), dict(stride=6), dict(rgb_p=rgb.ctypes.data + 2)):
        assert call(**kw) == -1 and b"4-byte aligned" in L.pcc_last_error(), kw
    for kw in (dict(dist=-1.0), dict(p2p=-0.5), dict(r2r=float("nan")), dict(dist=float("inf")), dict(p2p=float("nan")),
               dict(r2r=-float("inf"))):
        assert call(**kw) == -1 and b"bad threshold" in L.pcc_last_error(), kw
    for kw in (dict(nn=0), dict(rnn=0), dict(rnn=65537)):
        assert call(**kw) == -5 and b"neighbours" in L.pcc_last_error(), kw
    assert call() == -1 and b"null index" in L.pcc_last_error()  # all arguments good: the handle is looked at last
    assert (labels == 77).all() and ncl.value == 77


def test_host_half_against_the_oracle_plain_and_sanitized():
    """tests/cpp/test_rgb_merge.cpp, a stand-alone program: few colours with min_size 1 / 7 / 200 (the folds), colour noise,
    distance threshold 0.05, 3 region neighbours (the (d, t) cut) -- built twice, plain and with ASan + UBSan, both run"""
    r = subprocess.run(["make", "test-rgb-merge"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("rgb merge ok") == 2 and "FAILED" not in r.stdout
    assert (ROOT / "build" / "test_rgb_merge").exists() and (ROOT / "build" / "asan" / "test_rgb_merge").exists()


@pytest.mark.parametrize("scene", range(6))
def test_order_free_segments_are_the_oracles(scene):
    """region_colour = 0 and min_size = 1: nothing merges, nothing folds, nothing is dropped -- the oracle's clusters ARE the
    grown segments of its queue, in seed order.  The fixpoint of "push the lowest index along directed valid edges" must
    give the same ids."""
    name, pts, rgb = util.fixpoint_scenes()[scene]
    K = min(100, len(pts))
    ki, kd = oracle.knn_exhaustive(pts, pts, K)
    want, want_n = oracle.region_growing_rgb(pts, rgb, neighbours=ki, neighbour_d2=kd, region_colour=0.0, min_size=1)
    got, sweeps = util.order_free_segments(rgb, ki)
    print(f"{name:12s} {len(pts):5d}  segments oracle {want_n} free {got.max() + 1} equal {(got == want).all()}  jacobi sweeps {sweeps}")
    assert got.max() + 1 == want_n and (got == want).all()
    if name == "cascade":
        assert want_n < 6, "the dense clumps must be reached from the sparse ones (one-way edges), or the scene shows nothing"
    if name == "cascade_rev":
        assert want_n == 6, "in reversed order every clump is seeded before a sparser one reaches it"
