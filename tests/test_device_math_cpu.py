"""tests/cpp/test_device_math.hip on the CPU: the program must cross-compile for gfx950 with the library's flags, and its
`--host` run (no HIP call) must find the host pass of every lm_* function equal to this machine's libm, bit for bit, on the
sets the device run uses -- which pins the reference of tests/test_device_math_gpu.py to what test_libm_cpu, test_rift_cpu and
test_sift_cpu pin.  It also prints, per family of the composite functions' case sets, how many cases ended in each observable
class; every class a family is there for must be non-empty, so that a change to the generators cannot quietly stop reaching
the branches.  No GPU."""
import re
import subprocess
from pathlib import Path

import pytest

from device_math_util import FUNCTIONS

ROOT = Path(__file__).resolve().parent.parent

# (function, family) -> the classes that family aims at
EXPECTED = {
    # covariances from the nine sums of 3, 4, 5, 10 and 50 points
    ("plane_from_sums", "blob"): ["finite_normal", "cubic_path"],
    # the single-pass covariance cancels; the cubic's smallest root comes out <= 0 and pf_roots2 replaces the roots
    ("plane_from_sums", "offset1000"): ["nonpositive_variance", "finite_normal", "nan_normal", "cubic_fallback"],
    ("plane_from_sums", "plane"): ["curvature0", "finite_normal", "roots2_path"],
    ("plane_from_sums", "line"): ["nan_normal", "curvature0"],
    ("plane_from_sums", "identical"): ["nan_normal", "curvature0", "nonpositive_variance"],  # the zero matrix: scale <= FLT_MIN
    # the same covariances times 2^-100 and 2^+100, and matrices given directly
    ("plane_from_covariance", "blob"): ["finite_normal", "cubic_path"],
    ("plane_from_covariance", "offset1000"): ["finite_normal", "nan_normal", "cubic_fallback"],
    ("plane_from_covariance", "plane"): ["curvature0", "finite_normal"],
    ("plane_from_covariance", "line"): ["nan_normal", "curvature0"],
    ("plane_from_covariance", "identical"): ["nan_normal", "curvature0"],
    ("plane_from_covariance", "isotropic"): ["nan_normal", "cubic_path"],     # a triple root: A - lambda I = 0
    ("plane_from_covariance", "two_equal"): ["finite_normal", "nan_normal"],  # the smallest root single, or double
    ("plane_from_covariance", "denormal"): ["curvature0", "nan_normal", "finite_normal"],
    ("plane_from_covariance", "nonfinite"): ["nan_normal"],
    # |c0| either side of +-FLT_EPSILON; beyond -FLT_EPSILON the smallest root is negative: the fallback
    ("plane_from_covariance", "c0_edge"): ["roots2_path", "cubic_path", "cubic_fallback", "finite_normal"],
    ("rift_solve3", "random"): ["rank3"],
    ("rift_solve3", "rank0"): ["rank0"],
    ("rift_solve3", "rank1"): ["rank1"],
    ("rift_solve3", "rank2"): ["rank2"],
    ("rift_solve3", "diagonal"): ["rank0", "rank1", "rank2", "rank3"],
    ("rift_solve3", "equal_norms"): ["rank1", "rank3"],
    ("rift_solve3", "tail0_step0"): ["rank3"],
    ("rift_solve3", "tail0_step1"): ["rank3"],
    ("rift_solve3", "pivot_edge"): ["rank1", "rank2", "rank3"],  # second and third pivot either side of the threshold
    ("rift_solve3", "extreme"): ["rank0", "rank3"],              # squares that underflow to 0; everything else
    ("rift_vote", "random"): ["kept"],
    ("rift_vote", "self"): ["angle_reset"],           # 0 / 0
    ("rift_vote", "zero_gradient"): ["angle_reset"],  # x / 0
    ("rift_vote", "parallel"): ["angle_reset", "kept"],  # the cosine rounds beyond +-1, or does not
    ("rift_vote", "d2_edge"): ["kept"],
    ("rigid_from_sums", "rotation"): ["finite_transform"],
    ("rigid_from_sums", "identity"): ["finite_transform"],
    ("rigid_from_sums", "half_turn"): ["finite_transform"],
    ("rigid_from_sums", "coplanar"): ["finite_transform"],
    ("rigid_from_sums", "collinear"): ["finite_transform"],
    ("rigid_from_sums", "few"): ["refused"],
    ("rigid_from_sums", "zero"): ["refused", "finite_transform"],  # no pairs; pairs that are all the origin
    ("rigid_from_sums", "far_centre"): ["finite_transform"],
    ("rigid_from_sums", "huge"): ["inf_transform"],  # (products overflow: N is NaN, the sweep ends at once; T holds Inf, no NaN)
    ("sift_is_keypoint", "pool"): ["keypoint", "not_keypoint"],
}


@pytest.fixture(scope="module")
def host_run():
    subprocess.check_call(["make", "build/test_device_math"], cwd=ROOT)
    r = subprocess.run([str(ROOT / "build" / "test_device_math"), "--host"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    return r.stdout


def test_host_pass_carries_the_host_libms_bits(host_run):
    assert host_run.rstrip().endswith("host math: 0 mismatches against libm"), host_run[-2000:]
    for fn in FUNCTIONS:
        m = re.search(rf"^{fn}: (\d+) cases, host pass", host_run, re.M)
        assert m and int(m.group(1)) > 0, fn
    for fn in FUNCTIONS[:6]:
        m = re.search(rf"^{fn} against libm: (\d+) cases, 0 mismatches$", host_run, re.M)
        assert m and int(m.group(1)) > 0, fn


def test_every_family_reaches_the_classes_it_aims_at(host_run):
    seen = {}
    for m in re.finditer(r"^class (\w+) (\w+): (.*)$", host_run, re.M):
        words = m.group(3).split()
        seen[(m.group(1), m.group(2))] = {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}
    assert set(seen) == set(EXPECTED), set(seen) ^ set(EXPECTED)
    empty = [(key, cls) for key, classes in EXPECTED.items() for cls in classes if seen[key].get(cls, 0) == 0]
    assert not empty, empty
    m = re.search(r"^rift_vote: (\d+) votes had the angle reset to 0$", host_run, re.M)
    assert m and int(m.group(1)) > 0
