"""csrc/libm_f64.hpp without a GPU: lm_acos and lm_atan2 -- pcc_shot_descriptors' own definition of acos and atan2 in double,
fdlibm's e_acos.c / s_atan.c / e_atan2.c restated from + - * / sqrt and bit operations -- against the host's libm (math.acos,
math.atan2: the C library's own, never a vectorised substitute), through build/shot_host --libm.

Bound: at most 2 ulp apart.  fdlibm and glibc each document an error of at most 1 ulp for these functions, so two correct
implementations cannot differ by more.  Special values are exact.  The largest difference found is printed (EXPERIMENTS.md,
"SHOT descriptors")."""
import math
import subprocess

import numpy as np
import pytest

import shot_util

ULP_BOUND = 2


@pytest.fixture(scope="module")
def tools():
    subprocess.check_call(["make", "build/shot_host"], cwd=shot_util.ROOT)


def _ordered(x):
    """float64 -> int64, monotone in the value (+0 and -0 coincide): differences are distances in ulp"""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
    return np.where(b < 0, np.int64(-2**63) - b, b)


def _ulp_apart(a, b):
    assert not np.isnan(a).any() and not np.isnan(b).any()
    return np.abs(_ordered(a) - _ordered(b))


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _acos_arguments():
    rng = np.random.default_rng(5)
    dense = np.linspace(-1.0, 1.0, 200001)
    parts = [dense, rng.uniform(-1, 1, 100000),
             np.nextafter(dense[::500], 2.0).clip(-1, 1), np.nextafter(dense[::500], -2.0).clip(-1, 1),
             1.0 - np.logspace(-17, -1, 2000), -1.0 + np.logspace(-17, -1, 2000),         # towards +-1
             np.logspace(-320, -1, 3000), -np.logspace(-320, -1, 3000),                    # towards 0, subnormals included
             np.array([0.5, -0.5]), np.nextafter([0.5, 0.5, -0.5, -0.5], [1, 0, -1, 0]),  # the branch points
             np.array([5e-324, -5e-324, 2.2250738585072014e-308, 2.0**-57, 2.0**-56, 0.0, -0.0])]
    return np.concatenate(parts)


def _atan2_arguments():
    rng = np.random.default_rng(6)
    parts = []
    ang = rng.uniform(-np.pi, np.pi, 150000)                      # all four quadrants, every ratio
    rad = 10.0 ** rng.uniform(-12, 12, len(ang))
    parts.append(np.stack([rad * np.sin(ang), rad * np.cos(ang)], -1))
    mag = 10.0 ** rng.uniform(-300, 300, (50000, 2))              # far apart in magnitude: the k > 60 and k < -60 branches too
    parts.append(mag * rng.choice([-1.0, 1.0], mag.shape))
    for t in (7 / 16, 11 / 16, 19 / 16, 39 / 16, 2.0**-29, 1.0, 2.0**60, 2.0**-60, 2.0**66):   # fdlibm's reduction breakpoints
        r = t * (1.0 + np.concatenate([np.arange(-600, 601) * 2.0**-52, rng.uniform(-1e-6, 1e-6, 800)]))
        x = 10.0 ** rng.uniform(-3, 3, len(r))
        for sy in (1.0, -1.0):
            for sx in (1.0, -1.0):
                parts.append(np.stack([sy * r * x, sx * x], -1))
                parts.append(np.stack([sy * r, sx * np.ones_like(r)], -1))     # x == +-1: the ratio itself
    sub = np.array([5e-324, 1e-320, 1e-310, 2.2250738585072014e-308])          # subnormals and the smallest normal
    other = np.array([5e-324, 1e-310, 1e-300, 1.0, 1e300])
    for a in sub:
        for b in other:
            for sa in (1.0, -1.0):
                for sb in (1.0, -1.0):
                    parts.append(np.array([[sa * a, sb * b], [sb * b, sa * a]]))
    return np.concatenate(parts)


def test_acos_is_within_two_ulp_of_the_host_libm(tools, tmp_path):
    x = _acos_arguments()
    got = shot_util.run_libm("acos", x, tmp_path, "acos")
    want = np.array([math.acos(v) for v in x])
    d = _ulp_apart(got, want)
    print(f"lm_acos: {len(x)} arguments, largest difference {int(d.max())} ulp ({int((d > 0).sum())} differ at all), bound {ULP_BOUND}")
    assert d.max() <= ULP_BOUND, x[np.argmax(d)]


def test_atan2_is_within_two_ulp_of_the_host_libm(tools, tmp_path):
    yx = _atan2_arguments()
    got = shot_util.run_libm("atan2", yx, tmp_path, "atan2")
    want = np.array([math.atan2(y, x) for y, x in yx])
    d = _ulp_apart(got, want)
    print(f"lm_atan2: {len(yx)} pairs, largest difference {int(d.max())} ulp ({int((d > 0).sum())} differ at all), bound {ULP_BOUND}")
    assert d.max() <= ULP_BOUND, yx[np.argmax(d)]


def test_special_values_are_exact(tools, tmp_path):
    x = np.array([1.0, -1.0, 0.0, -0.0])
    got = shot_util.run_libm("acos", x, tmp_path, "acos_special")
    assert np.array_equal(_bits(got), _bits([0.0, math.pi, math.pi / 2, math.pi / 2]))
    assert np.isnan(shot_util.run_libm("acos", np.array([1.0000000000000002, -2.0, np.nan]), tmp_path, "acos_nan")).all()
    pairs, want = [], []
    for xv in (1.0, 3.5, 1e-310, 1e300, math.inf):       # atan2(+-0, +x) = +-0 and atan2(+-0, -x) = +-pi
        pairs += [(0.0, xv), (-0.0, xv), (0.0, -xv), (-0.0, -xv)]
        want += [0.0, -0.0, math.pi, -math.pi]
    for yv in (1.0, 3.5, 1e-310, 1e300, math.inf):       # atan2(+-y, +-0) = +-pi/2
        pairs += [(yv, 0.0), (yv, -0.0), (-yv, 0.0), (-yv, -0.0)]
        want += [math.pi / 2, math.pi / 2, -math.pi / 2, -math.pi / 2]
    pairs += [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0)]   # the zeros against each other, as C's Annex F has them
    want += [0.0, -0.0, math.pi, -math.pi]
    got = shot_util.run_libm("atan2", np.array(pairs), tmp_path, "atan2_special")
    assert np.array_equal(_bits(got), _bits(want))        # signs of zero included
    assert np.array_equal(_bits(want), _bits([math.atan2(y, x) for y, x in pairs]))
