"""tests/voxel_ref.py (float64 sums, rounded once) against oracle.voxel_grid (PCL's float running sums) on every cloud of the
exact GPU tests: two independent restatements of pcl::VoxelGrid.  Voxels, order and colours agree exactly; the centroids agree
to the bit where a float sum is exact, and within a float running sum's bound elsewhere -- the reason the oracle cannot serve
as the reference for the kernel's centroids.  Also csrc/voxel_plan.hpp, the lattice derivation, compiled on its own."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import oracle  # noqa: E402
import voxel_util as vu  # noqa: E402
from voxel_ref import ulp_distance, voxel_grid_ref  # noqa: E402

# dyadic clouds with at most 2^(24 - bits of a coordinate) points in a voxel: PCL's float sums are exact there as well
FLOAT_EXACT = ["faces-2^-4", "faces-0.025", "far-0.025", "non-finite", "one-point", "one-voxel-257"]
COORDINATE_BITS = {"faces-2^-4": 11, "faces-0.025": 11, "far-0.025": 23, "non-finite": 11, "one-point": 24, "one-voxel-257": 9}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", list(vu.CASES))
def test_reference_and_oracle_agree(name):
    rec, leaf = vu.cloud(name), vu.leaf_of(name)
    rows, counts = vu.reference(name)
    orows, nv = oracle.voxel_grid(rec, leaf, has_rgb=True)
    assert nv == len(rows) == len(counts) and counts.sum() == np.isfinite(rec[:, :3]).all(axis=1).sum()
    if name == "all-non-finite":
        assert nv == 0
        return
    assert nv > 0 and (_bits(orows[:, 3]) == 0x3F800000).all() and (_bits(rows[:, 3]) == 0x3F800000).all()
    assert (_bits(orows[:, 4]) == _bits(rows[:, 4])).all()          # colour words, and with them the order of the rows
    assert (_bits(rows[:, 4]) >> 24 == 0).all() and (_bits(rec[:, 4]) >> 24).max() > 0
    ulps = ulp_distance(rows[:, :3], orows[:, :3])
    bound = counts.max() * 2.0 ** -24 * np.abs(rec[np.isfinite(rec[:, :3]).all(axis=1), :3]).max()
    print(f"{name}: {nv} voxels, at most {counts.max()} points in one, oracle up to {ulps.max()} float ulps from the float64 mean, "
          f"|difference| <= {np.abs(rows[:, :3].astype(np.float64) - orows[:, :3]).max():.3g} (bound {bound:.3g})")
    if name in FLOAT_EXACT:
        assert counts.max() <= 2 ** (24 - COORDINATE_BITS[name]), name
        assert (_bits(rows[:, :3]) == _bits(orows[:, :3])).all()
    else:
        assert (np.abs(rows[:, :3].astype(np.float64) - orows[:, :3].astype(np.float64)) <= bound).all()


def test_reference_properties():
    """what the GPU cases rely on: the clouds are what their names say"""
    inv = np.float32(16.0)
    faces = vu.cloud("faces-2^-4")
    on_face = (np.floor(faces[:, :3] * inv) == faces[:, :3] * inv)
    assert 0.03 < on_face.any(axis=1).mean() < 0.06   # a coordinate in 64 is a multiple of the leaf
    assert (faces[:, :3] < 0).any() and (faces[:, :3] > 0).any()
    rows, counts = vu.reference("heavy-white")
    assert counts.max() >= 60000 and counts.max() <= 65793 and len(counts) > 100
    assert (_bits(rows[np.argmax(counts), 4]) == 0x00FFFFFF)
    nf = vu.cloud("non-finite")
    assert np.isnan(nf[0, 0]) and np.isinf(nf[-1, 2]) and np.isinf(nf[2000:2064, 0]).all() and np.isnan(nf[::97, 1]).all()
    assert vu.reference("one-point")[1].tolist() == [1] and vu.reference("one-voxel-257")[1].tolist() == [257]
    for name in ("general", "general-y+1000"):
        assert vu.reference(name)[1].max() <= 2 ** 10   # the premise of the 1-ulp bound of the GPU test
    # without colour: the same voxels and centroids, four columns
    rows4, counts4 = voxel_grid_ref(vu.cloud("far-0.25"), 0.25, False)
    rows5, counts5 = vu.reference("far-0.25")
    assert rows4.shape[1] == 4 and (counts4 == counts5).all() and (_bits(rows4) == _bits(rows5[:, :4])).all()
    # a lattice beyond int32 is not the reference's to decide
    wide = vu.records(np.array([[3000.0, 0, 0], [3000.001, 1e-4, 1e-4]], np.float32), np.random.default_rng(1))
    with pytest.raises(AssertionError):
        voxel_grid_ref(wide, 1e-6, True)


def test_input_layouts_of_the_gpu_helper():
    """voxel_util.input_bytes: every stride carries the fields the call reads, and the trimmed view ends with the last of them"""
    rec = vu.cloud("one-voxel-257")
    for stride in (12, 16, 20, 32):
        for rgb in (False, True):
            if rgb and stride < 20:
                continue
            whole = vu.input_bytes(rec, stride, rgb, True).reshape(257, stride)
            assert (np.ascontiguousarray(whole[:, :12]).view(np.float32) == rec[:, :3]).all()
            if stride >= 20:
                assert (np.ascontiguousarray(whole[:, 16:20]).view(np.uint32)[:, 0] == _bits(rec[:, 4])).all()
            cut = vu.input_bytes(rec, stride, rgb, False)
            assert len(cut) == 256 * stride + (20 if rgb else 12) and (cut == whole.reshape(-1)[:len(cut)]).all()


def test_lattice_plan_header_alone():
    """tests/cpp/test_voxel_plan.cpp compiles csrc/voxel_plan.hpp, the lattice derivation voxel.hip and sift_batch.hip (host
    check and kernel) share, on its own: hand-written lattices, both signs, bounds around 2^24 and 2^31, Inf and NaN products"""
    subprocess.check_call(["make", "build/test_voxel_plan"], cwd=ROOT)
    r = subprocess.run([str(ROOT / "build" / "test_voxel_plan")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_voxel_plan: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    csrc = ROOT / "pointcloudcomparator_amd" / "csrc"
    for user, uses in (("voxel.hip", 1), ("sift_batch.hip", 2)):
        text = (csrc / user).read_text()
        assert '#include "voxel_plan.hpp"' in text and text.count("voxel_plan(") == uses, user
        assert not re.search(r"\(int\)\s*(std::)?floorf?\((lo|hi|l|h)\b", text), user   # no conversion of a bound of its own
    mk = (ROOT / "Makefile").read_text()
    assert re.search(r"^hosttest:.*build/test_voxel_plan\b", mk, flags=re.M)
    assert re.search(r"^asan:.*build/asan/test_voxel_plan\b", mk, flags=re.M)
    assert re.search(r"^build/asan/test_voxel_plan:.*\n.*\n\t\$\(CXX\).*\$\(SANFLAGS\).*float-cast-overflow", mk, flags=re.M)
    assert "build/asan/test_voxel_plan\n" in mk
