"""pcc_sift_keypoints without a GPU (reference src/comparator.cpp:435-469, processSift): the entry point is declared,
exported and bound; its arguments are refused before any device is touched; the host mirror of the detector
(build/sift_host: csrc/sift_math.hpp, the header the kernels are compiled from) agrees with an independent NumPy
restatement in float64 (tests/sift_ref.py); lm_expf carries the host libm's bits.

The bound on the host mirror: per octave, max |dog_mirror - dog64| <= MARGIN x the largest deviation of the FLOAT32 run of
the restatement from its float64 run on the same scene (F32_VS_F64 below; measured with tools/exp_sift_ref.py, table and
method in EXPERIMENTS.md, "SIFT keypoints").  MARGIN is 4: the mirror differs from the float32 restatement only in the order
of its running sums (row order against index order) and in expf's last bit, both float32 rounding.  The restatement's sums
are RUNNING sums (one addition after the other, as PCL's loop and the mirror add): with ndarray.sum's pairwise additions the
float32 run is 3-4 x closer to float64 (4.5e-5 / 5.8e-5 / 5.9e-5) than any running float32 sum over rows of hundreds of
entries can be, the mirror's (1.8e-4 / 2.6e-4 / 3.1e-4) included.
The DoG columns are differences of mean intensities on the scale 0 .. 255."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sift_ref
import sift_util

ROOT = Path(__file__).resolve().parent.parent
MARGIN = 4.0
# max |float32 restatement - float64 restatement| over the DoG columns of every octave (EXPERIMENTS.md)
F32_VS_F64 = {"sift300": 1.57e-04, "sift600": 1.98e-04, "sift2000": 2.54e-04}
# every voxel grid's output size, why the loop ended, keypoints (float64 restatement)
EXPECT = {"sift300": ([293, 268, 169, 27, 8], "gate", 33), "sift600": ([581, 495, 199, 27, 8], "gate", 59),
          "sift2000": ([1957, 1700, 689, 125, 27], "count", 196)}


@pytest.fixture(scope="module")
def tools():
    subprocess.check_call(["make", "build/sift_host", "build/test_expf"], cwd=ROOT)


@pytest.fixture(scope="module")
def ref64():
    """name -> the float64 restatement's result, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            p, rgb = sift_util.scene(name)
            cache[name] = sift_ref.sift_pipeline(p, rgb, np.float64)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def mirror(tools, tmp_path_factory):
    """name -> build/sift_host's result with every octave dumped, computed once"""
    tmp = tmp_path_factory.mktemp("sift_host")
    cache = {}

    def get(name):
        if name not in cache:
            p, rgb = sift_util.scene(name)
            cache[name] = sift_util.run_host(p, rgb, tmp, tag=name.replace("-", "_"), dump=True)
        return cache[name]
    return get


def test_entry_point_is_declared_exported_bound_and_cites_the_reference():
    from pointcloudcomparator_amd import capi
    text = (ROOT / "include" / "pcc_nn.h").read_text()
    assert re.search(r"\bint pcc_sift_keypoints\(pcc_index \*ctx, const void \*pts, size_t n, size_t stride_bytes, const void \*rgb,\s+"
                     r"size_t rgb_stride_bytes, int mem, float min_scale, int nr_octaves, int nr_scales_per_octave,\s+float min_contrast, "
                     r"float \*out_keypoints", text)
    comment = text[:text.index("int pcc_sift_keypoints(")].rsplit("/*", 1)[1]
    assert "src/comparator.cpp:435-469" in comment and "processSift" in comment and "[recalled]" in comment
    assert "PCC_OPT_SIFT_LAYOUT = 25" in text
    assert "pcc_sift_keypoints" in capi.SYMBOLS and hasattr(capi.LIB, "pcc_sift_keypoints")
    assert callable(capi.Index.sift_keypoints)
    assert capi.OPT_SIFT_LAYOUT == 25 and capi.OPT_RIFT_LAYOUT == 24
    surface = (ROOT / "include" / "pcc" / "sift.hpp").read_text()
    assert "processSift(const PointCloud<PointXYZRGB>::Ptr& cloud" in surface and "src/comparator.cpp:435-469" in surface
    assert "processRIFTwithSIFT(const PointCloud<PointXYZRGB>::Ptr& cloud" in surface and ":686-822" in surface
    assert "struct alignas(16) PointWithScale" in (ROOT / "include" / "pcc" / "point_types.hpp").read_text()


def test_arguments_are_refused_without_a_device():
    """every refusal below happens with a NULL handle: nothing of it can have looked at a device"""
    from pointcloudcomparator_amd import capi
    L = capi.LIB
    pts = np.zeros((8, 8), np.float32)
    out = np.zeros((8, 4), np.float32)
    n_out = ctypes.c_size_t(0)
    nan, inf = float("nan"), float("inf")

    def call(p=pts.ctypes.data, n=8, stride=32, rgb=pts.ctypes.data + 16, rgb_stride=32, mem=0, min_scale=0.005, octaves=5, nspo=5,
             contrast=0.001, o=out.ctypes.data, cap=8, no=ctypes.byref(n_out)):
        return L.pcc_sift_keypoints(None, p, n, stride, rgb, rgb_stride, mem, min_scale, octaves, nspo, contrast, o, cap, no)

    assert call(mem=7) == -1 and b"mem space" in L.pcc_last_error()
    assert call(p=None) == -1 and b"null point pointer" in L.pcc_last_error()
    for kw in (dict(rgb=None), dict(o=None), dict(no=None)):
        assert call(**kw) == -1 and b"null argument" in L.pcc_last_error(), kw
    for kw in (dict(stride=8), dict(stride=14)):
        assert call(**kw) == -1 and b"stride" in L.pcc_last_error(), kw
    for kw in (dict(rgb_stride=0), dict(rgb_stride=6), dict(rgb=pts.ctypes.data + 18), dict(p=pts.ctypes.data + 2), dict(o=out.ctypes.data + 1)):
        assert call(**kw) == -1 and b"4-byte aligned" in L.pcc_last_error(), kw
    for v in (0.0, -0.005, nan, inf):
        assert call(min_scale=v) == -1 and b"min_scale" in L.pcc_last_error(), v
    for v in (-0.001, nan):
        assert call(contrast=v) == -1 and b"min_contrast" in L.pcc_last_error(), v
    for v in (0, -3):
        assert call(octaves=v) == -1 and b"nr_octaves" in L.pcc_last_error(), v
    for v in (0, -1, 14, 100):
        assert call(nspo=v) == -5 and b"1 to 13 scales per octave are built" in L.pcc_last_error(), v
    for v in (1, 13):
        assert call(nspo=v) == -1 and b"null index" in L.pcc_last_error(), v
    assert call() == -1 and b"null index" in L.pcc_last_error()  # all arguments good: the handle is looked at last


@pytest.mark.parametrize("name", list(sift_util.SMALL))
def test_scenes_meet_the_input_condition(ref64, name):
    """no test below compares empty sets: the float64 restatement finds at least 20 keypoints in at least two octaves; the
    loop ends at the 25-point gate on sift300 / sift600 and after the last octave on sift2000"""
    r = ref64(name)
    sizes, stop, n_kp = EXPECT[name]
    assert (r["sizes"], r["stop"], len(r["keypoints"])) == (sizes, stop, n_kp)
    assert len(r["keypoints"]) >= 20
    assert len({k[0] for k in r["keypoints"]}) >= 2
    assert r["stop"] == ("count" if name == "sift2000" else "gate")
    assert len(r["octaves"]) == (5 if name == "sift2000" else 4)
    assert min(o["rows"].min() for o in r["octaves"]) >= 1
    assert any(o["rows"].max() == len(o["cloud"]) for o in r["octaves"])  # some rows hold a whole octave cloud
    assert np.mean(r["octaves"][0]["rows"]) >= 20
    assert all(o["k"] == 25 for o in r["octaves"])


@pytest.mark.parametrize("name", list(sift_util.SMALL))
def test_host_mirror_against_float64_restatement(ref64, mirror, name):
    r, h = ref64(name), mirror(name)
    assert len(h["octaves"]) == len(r["octaves"]) and h["info"]["stop"] == r["stop"]
    assert [int(x) for x in h["info"]["sizes"].split("/")] == r["sizes"]
    worst = 0.0
    for o, (a, b) in enumerate(zip(h["octaves"], r["octaves"])):
        assert np.array_equal(a["cloud"], b["cloud"]), f"octave {o}: the voxel grids differ"
        # (numpy's float32 power and the host libm's powf may round the last bit differently)
        assert (np.abs(a["scales"] - b["scales"]) <= np.spacing(b["scales"])).all(), f"octave {o}: the scales differ"
        dev = float(np.abs(a["dog"].astype(np.float64) - b["dog"]).max())
        print(f"{name} octave {o} ({len(a['cloud'])} points): host mirror vs float64 restatement {dev:.3g}, float32 restatement "
              f"{F32_VS_F64[name]:.3g} on the scene, ratio {dev / F32_VS_F64[name]:.2f} (bound {MARGIN:g})")
        assert np.isfinite(a["dog"]).all()
        assert dev <= MARGIN * F32_VS_F64[name]
        worst = max(worst, dev)
    # keypoint sets, as (octave, point, column): nothing the float64 run does not have; what is missing sat on a margin
    got = [tuple(int(v) for v in k) for k in h["ids"]]
    want = r["keypoints"]
    assert got == sorted(got) and len(set(got)) == len(got)  # the detector's order
    assert set(got) <= set(want), sorted(set(got) - set(want))
    margin = dict(zip(want, r["margins"]))
    missing = [k for k in want if k not in set(got)]
    print(f"{name}: {len(got)} of {len(want)} keypoints, {len(missing)} left out; smallest float64 margin {r['margins'].min():.3g}, "
          f"largest DoG deviation {worst:.3g}")
    assert all(margin[k] < 2 * worst for k in missing), [(k, margin[k]) for k in missing]
    assert len(missing) <= 0.02 * len(want)
    # and the keypoints are the octave cloud's points with the column's scale
    for (o, i, c), kp in zip(got, h["keypoints"]):
        assert np.array_equal(kp[:3], h["octaves"][o]["cloud"][i]) and kp[3] == h["octaves"][o]["scales"][c]


def test_tiny_clouds_at_the_gate(ref64, mirror):
    """24 points in 24 voxels: no octave is processed; 25: one octave, every row and every k-NN row is the whole cloud"""
    h = mirror("tiny24")
    assert h["info"]["sizes"] == "24" and h["info"]["stop"] == "gate" and h["info"]["octaves"] == "0" and len(h["keypoints"]) == 0
    assert ref64("tiny24")["sizes"] == [24] and ref64("tiny24")["keypoints"] == []
    h, r = mirror("tiny25"), ref64("tiny25")
    assert h["info"]["sizes"] == "25/7" and h["info"]["stop"] == "gate" and h["info"]["octaves"] == "1"
    assert h["info"]["rows_min"] == "25" and h["info"]["rows_max"] == "25"
    assert r["sizes"] == [25, 7] and r["octaves"][0]["k"] == 25 and (r["octaves"][0]["rows"] == 25).all()
    assert [tuple(int(v) for v in k) for k in h["ids"]] == r["keypoints"]
    # a running float32 sum of 25 terms is within 25 u of the exact one (u = 2^-24), num and den each; a response is at most
    # 255, a DoG column the difference of two
    assert np.abs(h["octaves"][0]["dog"].astype(np.float64) - r["octaves"][0]["dog"]).max() <= 2 * 2 * 25 * 2.0 ** -24 * 255


def test_duplicates_and_non_finite_points_leave_in_the_first_voxel_grid(mirror):
    p, _ = sift_util.scene("dups")
    assert len(p) == 330
    assert mirror("dups")["info"]["sizes"].split("/")[0] == mirror("sift300")["info"]["sizes"].split("/")[0]  # same voxels occupied
    assert len(mirror("dups")["keypoints"]) > 0
    h = mirror("non-finite")
    p, _ = sift_util.scene("non-finite")
    assert int(h["info"]["sizes"].split("/")[0]) <= np.isfinite(p).all(1).sum() < len(p)
    assert len(h["keypoints"]) > 0 and np.isfinite(h["keypoints"]).all()


def test_restated_expf_against_the_host_libm(tools):
    """every float of [-4.5, 0], a stride sample of [-104, 89], the non-finite arguments; the largest ulp distance is printed
    and must not exceed the one recorded in tests/cpp/test_expf.cpp when lm_expf was written (0: all bits equal)"""
    r = subprocess.run([str(ROOT / "build" / "test_expf")], capture_output=True, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0 and "expf ok" in r.stdout, r.stdout[-2000:]
    assert re.search(r"expf 1\d{9} arguments: \d+ mismatches, max ulp distance \d+", r.stdout)


def test_library_does_not_link_the_host_mirror():
    mk = (ROOT / "Makefile").read_text()
    hip_srcs = re.search(r"^HIP_SRCS\s*:=(.*)$", mk, flags=re.M).group(1)
    assert "sift.hip" in hip_srcs and "sift_host" not in hip_srcs
    assert re.search(r"^hosttest:.*build/rift_driver.*build/test_expf.*build/sift_host.*build/sift_driver", mk, flags=re.M)
    assert re.search(r"^asan:.*build/asan/rift_host.*build/asan/sift_host", mk, flags=re.M)
