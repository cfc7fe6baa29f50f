"""pcc_fpfh_descriptors without a GPU (reference src/comparator.cpp:824-875, processFPFH): the entry point is declared,
exported and bound; its arguments are refused before any device is touched, in the documented order; the host mirror of the
pipeline (build/fpfh_host: csrc/fpfh_math.hpp + csrc/plane_fit.hpp, the headers the kernels are compiled from) agrees with an
independent NumPy restatement in float64 (tests/fpfh_ref.py), stage by stage:

  pair features   per feature at most MARGIN x the largest deviation of the restatement's FLOAT32 run from its float64 run on
                  the same pairs (PAIR_F32_VS_F64: f1, f2, f3, f4 and the gap acos|a1| - acos|a2| of the swap decision);
  SPFH            the normals GIVEN (oracle.normals_radius' float32 normals to both sides): the 33 integer vote counts of every
                  point are EQUAL, except for the points the restatement flags -- a pair in their row within EDGE = MARGIN x
                  the table's figure of a bin boundary or of a tie in the swap decision; at most 5 % of a scene may be flagged;
  weighting       the SPFH GIVEN (the mirror's table and rows): every bin within MARGIN x the deviation of the restatement's
                  own float32 weighting from its float64 weighting (WEIGHT_F32_VS_F64); no point is left out.

MARGIN is 8, as for RIFT: the mirror uses lm_acosf / lm_atan2f and unfused operations in one fixed order where NumPy calls
libm and sums as it likes.  Both tables are measured with tests/fpfh_ref.py run as a script (method and figures in
EXPERIMENTS.md, "FPFH descriptors"), from the restatement alone, never from the mirror."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fpfh_ref
import fpfh_util
import oracle

ROOT = Path(__file__).resolve().parent.parent
MARGIN = 8.0
# max |float32 restatement - float64 restatement| over the scene's 1250 pairs: f1 (as an angle), f2, f3, f4, swap gap
PAIR_F32_VS_F64 = {"volume300": (1.09e-06, 1.32e-07, 1.81e-07, 4.69e-09, 8.94e-07), "volume": (1.59e-06, 1.01e-06, 1.83e-07, 4.59e-09, 9.28e-06),
                   "slab": (3.02e-08, 1.99e-08, 9.41e-08, 4.85e-09, 2.57e-07), "near-plane": (4.74e-11, 3.35e-11, 8.11e-10, 4.48e-09, 1.17e-07),
                   "isolated": (6.47e-07, 5.9e-07, 1.49e-07, 5.38e-09, 5.36e-06), "non-finite": (1.36e-06, 2.1e-07, 1.68e-07, 3.89e-09, 4.22e-06),
                   "duplicates": (1.26e-06, 5.98e-07, 1.57e-07, 4.94e-09, 2.95e-06), "short-rows": (5.47e-08, 3.27e-08, 4.61e-08, 4.4e-09, 1.48e-07)}
# max |float32 weighting - float64 weighting| per bin over one SPFH table (bins are percentages: 0 .. 100)
WEIGHT_F32_VS_F64 = {"volume300": 4.44e-05, "volume": 7.71e-05, "slab": 0.000161, "near-plane": 7.63e-06, "isolated": 6.81e-05,
                     "non-finite": 9.01e-05, "duplicates": 4.93e-05, "short-rows": 2.34e-05}
# The vote counts are compared on every scene but near-plane: there every normal is the plane's and every connecting line lies
# in it, so a1 and a2 are both ~ 0, the swap decision of most pairs is a tie within rounding and the restatement flags 73 % of
# the points.  No seed changes that; the scene stays in every other test (and in the GPU test, bit for bit).
COUNT_SCENES = [s for s in fpfh_util.SMALL if s != "near-plane"]
LEFT_OUT_MAX = 0.05


@pytest.fixture(scope="module")
def tools():
    subprocess.check_call(["make", "build/fpfh_host"], cwd=ROOT)


@pytest.fixture(scope="module")
def given(tools, tmp_path_factory):
    """name -> what the stage tests share, computed once: the scene, oracle.normals_radius' normals, the float64 restatement over
    them (flags with EDGE = MARGIN x the scene's pair table) and the mirror's run over the same normals"""
    tmp = tmp_path_factory.mktemp("fpfh_given")
    cache = {}

    def get(name):
        if name not in cache:
            pts = fpfh_util.scene(name)
            nrm = oracle.normals_radius(np.ascontiguousarray(pts), 0.03)[:, :3]
            edge = MARGIN * np.array(PAIR_F32_VS_F64[name])[[0, 1, 2, 4]]
            ref = fpfh_ref.fpfh_pipeline(pts, np.float64, normals_given=nrm, edge=edge)
            hist, index, _, counts = fpfh_util.run_host(pts, tmp, tag=name.replace("-", "_"), normals=nrm, counts=True)
            cache[name] = {"pts": pts, "nrm": nrm, "ref": ref, "hist": hist, "index": index, "counts": counts}
        return cache[name]
    return get


@pytest.fixture(scope="module")
def mirror(tools, tmp_path_factory):
    """name -> (hist, index) of the whole pipeline in build/fpfh_host, its own normals"""
    tmp = tmp_path_factory.mktemp("fpfh_host")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = fpfh_util.run_host(fpfh_util.scene(name), tmp, tag=name.replace("-", "_"))[:2]
        return cache[name]
    return get


# ---- 1. declaration and binding ---------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_bound_and_cites_the_reference():
    from pointcloudcomparator_amd import capi
    text = (ROOT / "include" / "pcc_nn.h").read_text()
    assert re.search(r"\bint pcc_fpfh_descriptors\(pcc_index \*index, int mem, double normal_radius, double fpfh_radius,", text)
    comment = text[:text.index("int pcc_fpfh_descriptors(")].rsplit("/*", 1)[1]
    assert "replaces:" in comment and "src/comparator.cpp:824-875" in comment and "processFPFH" in comment
    assert "[recalled]" in comment and "unpinned" in comment
    assert "pcc_fpfh_descriptors" in capi.SYMBOLS and hasattr(capi.LIB, "pcc_fpfh_descriptors")
    assert callable(capi.Index.fpfh_descriptors)
    assert capi.OPT_FPFH_LAYOUT == 29 and re.search(r"\bPCC_OPT_FPFH_LAYOUT = 29\b", text)
    mirror_hpp = (ROOT / "include" / "pcc" / "fpfh.hpp").read_text()
    assert "processFPFH(const PointCloud<PointXYZRGB>::Ptr& cloud" in mirror_hpp and "src/comparator.cpp:824-875" in mirror_hpp
    assert "struct FPFHSignature33" in mirror_hpp
    assert '"PCC_FPFH_LAYOUT"' in (ROOT / "pointcloudcomparator_amd" / "csrc" / "api.hip").read_text()


def test_library_does_not_link_the_host_mirror():
    mk = (ROOT / "Makefile").read_text()
    hip_srcs = re.search(r"^HIP_SRCS\s*:=(.*)$", mk, flags=re.M).group(1)
    assert "fpfh.hip" in hip_srcs and "fpfh_host" not in hip_srcs
    assert re.search(r"^hosttest:.*build/fpfh_host.*build/fpfh_driver", mk, flags=re.M)
    assert re.search(r"^asan:.*build/asan/fpfh_host", mk, flags=re.M)


# ---- 2. refusals --------------------------------------------------------------------------------------------------------------
def test_arguments_are_refused_without_a_device_in_the_documented_order():
    """every refusal below happens with a NULL handle: nothing of it can have looked at a device.  Each call is wrong in the
    way under test AND in every way that is checked later, so the message shows which check came first."""
    from pointcloudcomparator_amd import capi
    L = capi.LIB
    hist = np.full((8, 33), 7.0, np.float32)
    idx = np.full(8, 7, np.int32)
    n_out = ctypes.c_size_t(77)

    def call(mem=0, rn=0.03, rf=0.05, bins=(11, 11, 11), h=hist.ctypes.data, i=idx.ctypes.data, no=ctypes.byref(n_out)):
        return L.pcc_fpfh_descriptors(None, mem, rn, rf, bins[0], bins[1], bins[2], h, i, no)

    assert call(mem=7, h=None, rn=0.0, bins=(5, 5, 5)) == -1 and b"mem space" in L.pcc_last_error()
    for kw in (dict(h=None), dict(i=None), dict(no=None)):
        assert call(rn=0.0, bins=(5, 5, 5), **kw) == -1 and b"null argument" in L.pcc_last_error(), kw
    for kw in (dict(rn=0.0), dict(rn=-0.03), dict(rf=float("nan")), dict(rf=float("inf")), dict(rf=0.0)):
        assert call(bins=(5, 5, 5), **kw) == -1 and b"bad radius" in L.pcc_last_error(), kw
    for bins in ((11, 11, 10), (33, 0, 0), (0, 0, 0), (10, 11, 11), (11, 12, 11)):
        assert call(bins=bins) == -5, bins
        assert b"only 11 + 11 + 11 bins" in L.pcc_last_error()
    assert call() == -1 and b"null index" in L.pcc_last_error()  # all arguments good: the handle is looked at last
    assert (hist == 7.0).all() and (idx == 7).all() and n_out.value == 77  # a refused call writes nothing


# ---- 3. the input condition -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fpfh_util.SMALL))
def test_scenes_meet_the_input_condition(name):
    """no test below compares empty sets (float64 restatement, its own normals)"""
    pts = fpfh_util.scene(name)
    r = fpfh_ref.fpfh_pipeline(pts, np.float64)
    n2 = int(r["in2"].sum())
    if name == "isolated":
        assert n2 == len(pts) - 30  # the singles, the pairs and the spokes: what it was built to lose
    else:
        assert n2 >= 0.9 * len(pts)
    rows = r["row_len"][r["in2"]]
    if name == "short-rows":
        assert 5 <= rows.min() and rows.max() <= 20  # all below one chunk
    else:
        assert np.median(rows) >= 10
    if name == "volume":
        assert np.median(rows) > 64 and rows.max() > 128  # crosses every chunk size
    h = r["hist"]
    assert h.shape == (n2, 33) and np.isfinite(h).all()
    sums = h.reshape(n2, 3, 11).sum(2)
    assert np.abs(sums[rows > 1] - 100.0).max() < 1e-3
    if name == "duplicates":
        assert len(fpfh_util.duplicate_pairs(pts)) == 20
    if name == "non-finite":
        assert np.isfinite(pts[r["index"]]).all() and not np.isfinite(pts).all()


# ---- 4. pair features -----------------------------------------------------------------------------------------------------------
def test_pair_features_against_the_float64_restatement(tools, tmp_path):
    total = 0
    for name in fpfh_util.SMALL:
        pts = fpfh_util.scene(name)
        nrm = oracle.normals_radius(np.ascontiguousarray(pts), 0.03)[:, :3]
        a, b = fpfh_util.scene_pairs(pts, nrm)
        total += len(a)
        table = np.array(PAIR_F32_VS_F64[name])
        p0 = np.where(np.isfinite(pts), pts, 0)
        measured = fpfh_ref.pair_deviation(p0, nrm, a, b)
        assert np.allclose(measured, table, rtol=0.02), f"{name}: the table is not what tests/fpfh_ref.py measures: {measured}"
        r64 = fpfh_ref.pair_features(p0, nrm, a, b, np.float64)
        f, ok, swapped = fpfh_util.run_pairs(pts, nrm, np.stack([a, b], -1), tmp_path, tag=name.replace("-", "_"))
        flagged = fpfh_ref.near_edge(r64, MARGIN * table[[0, 1, 2, 4]])
        assert np.array_equal(ok[~flagged], r64["ok"][~flagged]), f"{name}: 'no pair' differs on an unflagged pair"
        assert np.array_equal(swapped[~flagged], r64["swapped"][~flagged]), f"{name}: the swap decision differs on an unflagged pair"
        both = ok & r64["ok"] & (swapped == r64["swapped"])
        assert both.sum() >= 0.95 * len(a)
        d = np.abs(f.astype(np.float64) - r64["f"])[both]
        d[:, 0] = fpfh_ref.circular(f[both, 0].astype(np.float64) - r64["f"][both, 0])
        dev = d.max(0)
        print(f"{name}: {len(a)} pairs ({int(flagged.sum())} flagged), mirror vs float64 f1 .. f4 " + " ".join(f"{x:.3g}" for x in dev) +
              "; ratio to the float32 restatement " + " ".join(f"{x:.2f}" for x in dev / table[:4]) + f" (bound {MARGIN:g})")
        assert (dev <= MARGIN * table[:4]).all(), name
    assert 9000 <= total <= 11000  # about 10^4 pairs


# ---- 5. SPFH counts, the normals given ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", COUNT_SCENES)
def test_spfh_vote_counts_equal_the_restatements(given, name):
    g = given(name)
    ref = g["ref"]
    in2 = ref["in2"]
    assert np.array_equal(g["index"], ref["index"])
    left_out = ref["flagged"][in2].mean()
    compare = in2 & ~ref["flagged"]
    differ = (g["counts"][compare] != ref["counts"][compare]).any(1)
    print(f"{name}: {100 * left_out:.2f} % of cloud2 left out (at most {100 * LEFT_OUT_MAX:g}), {int(compare.sum())} points compared, "
          f"{int(differ.sum())} differ")
    assert left_out <= LEFT_OUT_MAX  # (the restatement alone decides this)
    assert not differ.any()
    assert (g["counts"][~in2] == 0).all()
    # every vote is one count in each of the three groups
    per_group = g["counts"].reshape(len(in2), 3, 11).sum(2)
    assert (per_group[:, 0] == per_group[:, 1]).all() and (per_group[:, 0] == per_group[:, 2]).all()
    assert (per_group[in2, 0] <= ref["row_len"][in2] - 1).all()


# ---- 6. weighting, the SPFH given ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fpfh_util.SMALL))
def test_weighting_against_the_float64_restatement_over_the_mirrors_spfh(given, name):
    g = given(name)
    ref = g["ref"]
    in2 = ref["in2"]
    spfh = fpfh_ref.spfh_table(g["counts"].astype(np.int64), ref["row_len"], np.float32)  # the mirror's table: its counts, its increments
    w64 = fpfh_ref.weighting(spfh, ref["rows"], ref["d2"], in2, np.float64)[in2]
    assert g["hist"].shape == w64.shape and np.isfinite(g["hist"]).all()
    dev = np.abs(g["hist"].astype(np.float64) - w64).max()
    print(f"{name}: mirror vs float64 weighting {dev:.3g}, float32 restatement {WEIGHT_F32_VS_F64[name]:.3g}, "
          f"ratio {dev / WEIGHT_F32_VS_F64[name]:.2f} (bound {MARGIN:g})")
    assert dev <= MARGIN * WEIGHT_F32_VS_F64[name]


def test_weighting_table_is_what_the_restatement_measures(given):
    for name in fpfh_util.SMALL:
        ref = given(name)["ref"]
        t32 = fpfh_ref.spfh_table(ref["counts"], ref["row_len"], np.float32)
        w32 = fpfh_ref.weighting(t32, ref["rows"], ref["d2"], ref["in2"], np.float32)
        w64 = fpfh_ref.weighting(t32, ref["rows"], ref["d2"], ref["in2"], np.float64)
        assert np.isclose(np.abs(w32 - w64).max(), WEIGHT_F32_VS_F64[name], rtol=0.02), name


# ---- 7. exact cases ----------------------------------------------------------------------------------------------------------------
def test_isolated_hubs_have_an_all_zero_descriptor(mirror):
    pts = fpfh_util.scene("isolated")
    hist, index = mirror("isolated")
    r = fpfh_ref.fpfh_pipeline(pts, np.float64)
    hubs = np.nonzero(r["in2"] & (r["row_len"] == 1))[0]
    assert len(hubs) == 6
    rows = np.searchsorted(index, hubs)
    assert np.array_equal(index[rows], hubs)
    assert (hist[rows].view(np.uint32) == 0).all()  # +0.0 in every bin: incr = inf was never added
    assert (hist[np.setdiff1d(np.arange(len(index)), rows)].sum(1) > 0).all()


def test_copies_of_a_point_carry_equal_descriptors(mirror):
    pts = fpfh_util.scene("duplicates")
    hist, index = mirror("duplicates")
    assert np.array_equal(index, np.arange(len(pts)))
    pairs = fpfh_util.duplicate_pairs(pts)
    assert len(pairs) == 20
    for a, b in pairs:
        assert np.array_equal(hist[a].view(np.uint32), hist[b].view(np.uint32)), (a, b)


@pytest.mark.parametrize("name", list(fpfh_util.SMALL))
def test_kept_indices_are_the_points_with_a_finite_normal(mirror, name):
    pts = fpfh_util.scene(name)
    nrm = oracle.normals_radius(np.ascontiguousarray(pts), 0.03)[:, :3]
    assert np.array_equal(mirror(name)[1], np.nonzero(np.isfinite(nrm).all(1))[0])


def test_big_scene_meets_the_input_condition():
    """the 20 000-point cluster of the GPU test and of tools/exp_fpfh.py (too large for the O(n^2) restatement): rows counted on a sample"""
    p = fpfh_util.scene("volume20000")
    sample = p[::20]
    d = sample[:, None, :] - p[None, :, :]
    rows = ((d * d).sum(-1) < np.float32(0.05 * 0.05)).sum(1)
    assert np.median(rows) >= 10 and rows.max() > 128


# ---- 8. the stand-alone tool under ASan and UBSan ------------------------------------------------------------------------------------
def test_host_mirror_is_clean_under_the_sanitizers(tmp_path):
    subprocess.check_call(["make", "build/asan/fpfh_host"], cwd=ROOT)
    r = subprocess.run([str(ROOT / "build" / "asan" / "fpfh_host"), "--self", str(tmp_path / "self.bin")], capture_output=True, text=True,
                       timeout=300, env={"ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0 and "fpfh_host n=240" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    hist, index = fpfh_util.read_result(tmp_path / "self.bin")
    assert 200 <= len(index) < 240 and np.isfinite(hist).all()
