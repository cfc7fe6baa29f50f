"""pcc_rift_descriptors without a GPU (reference src/comparator.cpp:590-684, processRIFT): the entry point is declared,
exported and bound; its arguments are refused before any device is touched; the host mirror of the pipeline
(build/rift_host: csrc/rift_math.hpp + csrc/plane_fit.hpp, the headers the kernels are compiled from) agrees with an
independent NumPy restatement in float64 (tests/rift_ref.py); lm_acosf carries the host libm's bits.

The bound on the host mirror: per bin, at most MARGIN x the largest deviation of the FLOAT32 run of the restatement from
its float64 run on the same scene (F32_VS_F64 below; measured with tests/rift_ref.py, table and method in EXPERIMENTS.md,
"RIFT descriptors").  MARGIN is 8: the C++ solve is a hand-written column-pivoted Householder QR where the restatement
calls LAPACK's SVD, and the near-plane scene pushes the condition number of the 3 x 3 system to 5e6.
The restatement takes every stage in the run's dtype, the normal included (PCL's single-pass covariance E[xx] - E[x]E[x]):
in float32 that stage alone moves a bin by up to 8e-4 (an isotropic neighbourhood has no preferred normal), which is why
the figures are larger than with a float64 normal in both runs.  GIVEN_NORMALS holds the same measurement with the normal
stage taken out (both runs and the mirror get oracle.normals_radius' normals): the gradient and histogram stages alone."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle
import rift_ref
import rift_util

ROOT = Path(__file__).resolve().parent.parent
MARGIN = 8.0
# max |float32 restatement - float64 restatement| per bin, every stage in the run's dtype (EXPERIMENTS.md)
F32_VS_F64 = {"volume": 5.43e-05, "volume300": 6.59e-05, "slab": 1.18e-05, "near-plane": 7.99e-04, "isolated": 7.89e-05,
              "non-finite": 5.83e-05}
# the same with the normals given (oracle.normals_radius) to both runs: gradient + histogram stages only.  The near-plane
# scene is not in this table: there the mirror's QR differs from the float64 run by 6.2e-4, 33 x the 1.9e-5 of the float32
# SVD run -- with pivots at the rank threshold column pivoting sets an AXIS unknown to zero where the SVD removes the
# singular direction; end to end (above) the scene is held at 0.87 x.
GIVEN_NORMALS = {"volume": 8.07e-07, "volume300": 1.79e-06, "slab": 3.52e-06, "isolated": 1.51e-06, "non-finite": 3.11e-06}
# descriptors that survive both compactions, of the scene's points (float64 restatement)
KEPT = {"volume": (600, 600), "volume300": (300, 300), "slab": (600, 600), "near-plane": (600, 600), "isolated": (500, 536),
        "non-finite": (487, 500)}


@pytest.fixture(scope="module")
def tools():
    subprocess.check_call(["make", "build/rift_host", "build/test_acosf"], cwd=ROOT)


def test_entry_point_is_declared_exported_bound_and_cites_the_reference():
    from pointcloudcomparator_amd import capi
    text = (ROOT / "include" / "pcc_nn.h").read_text()
    assert re.search(r"\bint pcc_rift_descriptors\(pcc_index \*index, const void \*rgb, size_t rgb_stride_bytes, int mem", text)
    comment = text[:text.index("int pcc_rift_descriptors(")].rsplit("/*", 1)[1]
    assert "src/comparator.cpp:590-684" in comment and "processRIFT" in comment
    assert "pcc_rift_descriptors" in capi.SYMBOLS and hasattr(capi.LIB, "pcc_rift_descriptors")
    assert callable(capi.Index.rift_descriptors)
    assert capi.OPT_RIFT_LAYOUT == 24
    mirror = (ROOT / "include" / "pcc" / "rift.hpp").read_text()
    assert "processRIFT(const PointCloud<PointXYZRGB>::Ptr& cloud" in mirror and "src/comparator.cpp:590-684" in mirror


def test_arguments_are_refused_without_a_device():
    """every refusal below happens with a NULL handle: nothing of it can have looked at a device"""
    from pointcloudcomparator_amd import capi
    L = capi.LIB
    rgb = np.zeros(8, np.uint32)
    hist = np.zeros((8, 32), np.float32)
    idx = np.zeros(8, np.int32)
    n_out = ctypes.c_size_t(0)

    def call(rgb_p=rgb.ctypes.data, stride=4, mem=0, rn=0.03, rg=0.03, rr=0.05, nd=4, ng=8, h=hist.ctypes.data, i=idx.ctypes.data,
             no=ctypes.byref(n_out)):
        return L.pcc_rift_descriptors(None, rgb_p, stride, mem, rn, rg, rr, nd, ng, h, i, no)

    assert call(mem=7) == -1 and b"mem space" in L.pcc_last_error()
    for kw in (dict(rgb_p=None), dict(h=None), dict(i=None), dict(no=None)):
        assert call(**kw) == -1 and b"null argument" in L.pcc_last_error(), kw
    for kw in (dict(stride=0), dict(stride=6), dict(rgb_p=rgb.ctypes.data + 2)):
        assert call(**kw) == -1 and b"4-byte aligned" in L.pcc_last_error(), kw
    for kw in (dict(rn=0.0), dict(rg=-0.03), dict(rr=float("nan")), dict(rr=float("inf"))):
        assert call(**kw) == -1 and b"bad radius" in L.pcc_last_error(), kw
    for nd, ng in ((8, 4), (4, 4), (2, 16), (1, 32), (0, 8), (5, 8)):  # nd * ng == 32 included
        assert call(nd=nd, ng=ng) == -5, (nd, ng)
        assert b"only 4 distance x 8 gradient bins" in L.pcc_last_error()
    assert call() == -1 and b"null index" in L.pcc_last_error()  # all arguments good: the handle is looked at last


def _pipeline(name, tmp_path, normals=None):
    p, rgb = rift_util.scene(name)
    h64, i64, info = rift_ref.rift_pipeline(p, rgb, np.float64, normals=normals)
    hh, ih, _ = rift_util.run_tool(rift_util.HOST, p, rgb, tmp_path)
    return p, h64, i64, info, hh, ih


@pytest.mark.parametrize("name", list(rift_util.SMALL))
def test_scenes_meet_the_input_condition(name):
    """no test below compares empty sets: >= 90 % of the points keep a finite descriptor in the float64 restatement and the
    median r = 0.03 row holds >= 10 entries (the scene built to have isolated points: what it was built to lose, exactly)"""
    p, rgb = rift_util.scene(name)
    h64, i64, info = rift_ref.rift_pipeline(p, rgb, np.float64)
    assert (len(i64), len(p)) == KEPT[name]
    assert np.median(info["rows_normal"]) >= 10
    assert len(i64) >= 0.9 * len(p)
    assert np.isfinite(h64).all() and h64.shape == (len(i64), 32)
    if name == "isolated":
        assert len(i64) < len(p)  # 30 points without a normal (first compaction), 6 hubs with a NaN gradient (second)
    if name == "non-finite":
        assert np.isfinite(p[i64]).all() and not np.isfinite(p).all()


@pytest.mark.parametrize("name", list(rift_util.SMALL))
def test_host_mirror_against_float64_restatement(tools, tmp_path, name):
    p, h64, i64, info, hh, ih = _pipeline(name, tmp_path)
    assert np.array_equal(ih, i64), "kept point indices differ"
    assert hh.shape == h64.shape and np.isfinite(hh).all()  # every descriptor takes part
    dev = np.abs(hh.astype(np.float64) - h64).max()
    print(f"{name}: host mirror vs float64 restatement {dev:.3g}, float32 restatement {F32_VS_F64[name]:.3g}, "
          f"ratio {dev / F32_VS_F64[name]:.2f} (bound {MARGIN:g}); largest condition number {info['cond'].max():.1e}")
    assert dev <= MARGIN * F32_VS_F64[name]


@pytest.mark.parametrize("name", list(GIVEN_NORMALS))
def test_gradient_and_histogram_stages_alone(tools, tmp_path, name):
    """the float64 restatement is handed the float32 normals the mirror computes (oracle.normals_radius returns the bits of
    pcc_normals_radius, tests/test_normals_gpu.py): what remains is the error of the new stages, held to 8 x the float32
    restatement's with the same normals"""
    p, rgb = rift_util.scene(name)
    nr = oracle.normals_radius(np.ascontiguousarray(p), 0.03)[:, :3]
    p, h64, i64, info, hh, ih = _pipeline(name, tmp_path, normals=nr)
    assert np.array_equal(ih, i64)
    dev = np.abs(hh.astype(np.float64) - h64).max()
    print(f"{name}: given normals, host mirror vs float64 {dev:.3g}, float32 restatement {GIVEN_NORMALS[name]:.3g}")
    assert dev <= MARGIN * GIVEN_NORMALS[name]


def test_big_scene_meets_the_input_condition(tools, tmp_path):
    """the 20 000-point cluster of the GPU test and of tools/exp_rift.py (too large for the O(n^2) restatement): rows counted
    on a sample, kept descriptors from the host mirror"""
    p, rgb = rift_util.scene("volume20000")
    sample = p[::10]
    d = sample[:, None, :] - p[None, :, :]
    rows = ((d * d).sum(-1) < np.float32(0.03 * 0.03)).sum(1)
    assert np.median(rows) >= 10
    hh, ih, _ = rift_util.run_tool(rift_util.HOST, p, rgb, tmp_path)
    assert len(ih) >= 0.9 * len(p) and np.isfinite(hh).all()


def test_restated_acosf_against_the_host_libm(tools):
    """every float of [-1, 1], the non-finite and the out-of-range arguments; the largest ulp distance is printed and must
    not exceed the one recorded in tests/cpp/test_acosf.cpp when lm_acosf was written (0: all bits equal)"""
    r = subprocess.run([str(ROOT / "build" / "test_acosf")], capture_output=True, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0 and "acosf ok" in r.stdout, r.stdout[-2000:]
    assert re.search(r"acosf 2\d{9} arguments: \d+ mismatches, max ulp distance \d+", r.stdout)


def test_library_does_not_link_the_host_mirror():
    mk = (ROOT / "Makefile").read_text()
    hip_srcs = re.search(r"^HIP_SRCS\s*:=(.*)$", mk, flags=re.M).group(1)
    assert "rift.hip" in hip_srcs and "rift_host" not in hip_srcs
    assert re.search(r"^hosttest:.*build/rift_host.*build/rift_driver", mk, flags=re.M)
    assert re.search(r"^asan:.*build/asan/rift_host", mk, flags=re.M)
