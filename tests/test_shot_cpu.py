"""pcc_shot_descriptors without a GPU (reference src/comparator.cpp:941-986, the deterministic part of processSHOT): the entry
point is declared, exported and bound; its arguments are refused before any device is touched, in the documented order; the host
mirror of the pipeline (build/shot_host: csrc/shot_math.hpp + csrc/libm_f64.hpp + csrc/plane_fit.hpp, the headers the kernels
are compiled from) agrees with an independent NumPy restatement in float64 (tests/shot_ref.py), stage by stage:

  Jacobi       shot_jacobi3 alone on >= 10^4 symmetric matrices: residuals and orthogonality within 64 x 2^-52, eigenvalues
               equal to eigh's within the same bound, exact zeros within the sweep cap on all of them;
  frames       the normals GIVEN (oracle.normals_radius' float32 normals to both sides): same NaN pattern everywhere; on the
               points the restatement does not flag -- an adjacent eigenvalue gap below GAP of the trace, or a sign vote that
               rests on entries with |v . axis| < EDGE = MARGIN x LRF_DOT_F32_VS_F64 -- the same signs and an axis angle of at
               most MARGIN x LRF_F32_VS_F64; at most 5 % of a scene may be flagged;
  descriptors  the frames GIVEN too (the mirror's own, to both sides): every bin of every finite row within MARGIN x
               DESC_F32_VS_F64, the same NaN rows, every finite row of norm 1 within the same figure; no point is left out (the
               interpolation is continuous across every routing boundary).

MARGIN is 8, as for RIFT and FPFH.  The tables are the largest deviation of the restatement's FLOAT32 run from its float64 run,
measured with tests/shot_ref.py run as a script (method and figures in EXPERIMENTS.md, "SHOT descriptors"), from the
restatement alone, never from the mirror."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle
import shot_ref
import shot_util

ROOT = Path(__file__).resolve().parent.parent
MARGIN = 8.0
# the largest angle (rad) between the float32 and the float64 restatement's x or z axis over the points with a gap >= shot_ref.GAP
LRF_F32_VS_F64 = {"volume300": 3.13e-06, "volume": 1.9e-05, "slab": 1.21e-05, "near-plane": 2.67e-05, "isolated": 4.84e-06,
                  "non-finite": 1.66e-05, "duplicates": 4.96e-06, "short-rows": 1.24e-05, "five-rule": 3.24e-07}
# the largest |v . axis in float32 - v . axis in float64| over the same points' valid entries: EDGE = MARGIN x this
LRF_DOT_F32_VS_F64 = {"volume300": 1.06e-07, "volume": 7.45e-07, "slab": 4.74e-07, "near-plane": 1.06e-06, "isolated": 1.81e-07,
                      "non-finite": 5.8e-07, "duplicates": 1.61e-07, "short-rows": 4.28e-07, "five-rule": 2.58e-09}
# the largest |bin in float32 - bin in float64|, the frames given (bins of a unit-norm descriptor: 0 .. 1)
DESC_F32_VS_F64 = {"volume300": 1.29e-07, "volume": 1.3e-07, "slab": 9.99e-08, "near-plane": 1.18e-07, "isolated": 1.32e-07,
                   "non-finite": 9.34e-08, "duplicates": 1.85e-07, "short-rows": 1.65e-07, "five-rule": 1.87e-07}
# The share of flagged frames is bounded on every scene but near-plane: there every neighbourhood lies in one plane, every v . z
# is ~ 0, and the sign vote of z rests on entries within EDGE for 88 % of the points.  No seed changes that; the scene's
# unflagged points are still compared, and it stays in every other test (and in the GPU test, bit for bit).
SHARE_SCENES = [s for s in shot_util.SMALL if s != "near-plane"]
DENSE = ["volume300", "volume", "slab", "near-plane", "isolated", "non-finite", "duplicates"]
LEFT_OUT_MAX = 0.05
JACOBI_BOUND = 64 * 2.0**-52


@pytest.fixture(scope="module")
def tools():
    subprocess.check_call(["make", "build/shot_host"], cwd=ROOT)


@pytest.fixture(scope="module")
def given(tools, tmp_path_factory):
    """name -> what the stage tests share, computed once: the scene, oracle.normals_radius' normals at 0.05, the float64
    restatement over them, and the mirror's run over the same normals with the frames of all points"""
    tmp = tmp_path_factory.mktemp("shot_given")
    cache = {}

    def get(name):
        if name not in cache:
            pts = shot_util.scene(name)
            nrm = oracle.normals_radius(np.ascontiguousarray(pts), 0.05)[:, :3]
            ref = shot_ref.shot_pipeline(pts, np.float64, normals_given=nrm)
            desc, rf, index, _, lrf = shot_util.run_host(pts, tmp, tag=name.replace("-", "_"), normals=nrm, lrf_out=True)
            cache[name] = {"pts": pts, "nrm": nrm, "ref": ref, "desc": desc, "rf": rf, "index": index, "lrf": lrf}
        return cache[name]
    return get


@pytest.fixture(scope="module")
def mirror(tools, tmp_path_factory):
    """name -> (desc, rf, index) of the whole pipeline in build/shot_host, its own normals"""
    tmp = tmp_path_factory.mktemp("shot_host")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = shot_util.run_host(shot_util.scene(name), tmp, tag=name.replace("-", "_"))[:3]
        return cache[name]
    return get


# ---- 1. declaration and binding ---------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_bound_and_cites_the_reference():
    from pointcloudcomparator_amd import capi
    text = (ROOT / "include" / "pcc_nn.h").read_text()
    assert re.search(r"\bint pcc_shot_descriptors\(pcc_index \*index, int mem, double normal_radius, double shot_radius,", text)
    comment = text[:text.index("int pcc_shot_descriptors(")].rsplit("/* ----", 1)[1]
    assert "replaces:" in comment and "src/comparator.cpp:941-986" in comment and "processSHOT" in comment
    assert "915-939" in comment and "[recalled]" in comment and "unpinned" in comment
    assert "pcc_shot_descriptors" in capi.SYMBOLS and hasattr(capi.LIB, "pcc_shot_descriptors")
    assert callable(capi.Index.shot_descriptors)
    mirror_hpp = (ROOT / "include" / "pcc" / "shot.hpp").read_text()
    assert "processSHOT(const PointCloud<PointXYZRGB>::Ptr& cloud" in mirror_hpp and "src/comparator.cpp:941-986" in mirror_hpp
    assert "struct SHOT352" in mirror_hpp and "915-939" in mirror_hpp
    assert "pcc_sift_keypoints" in mirror_hpp and "pcc_first_within" in mirror_hpp


def test_library_does_not_link_the_host_mirror():
    mk = (ROOT / "Makefile").read_text()
    hip_srcs = re.search(r"^HIP_SRCS\s*:=(.*)$", mk, flags=re.M).group(1)
    assert "shot.hip" in hip_srcs and "shot_host" not in hip_srcs
    assert re.search(r"^hosttest:.*build/shot_host.*build/shot_driver", mk, flags=re.M)
    assert re.search(r"^asan:.*build/asan/shot_host", mk, flags=re.M)
    assert "build/asan/shot_host --self" in mk


# ---- 2. refusals --------------------------------------------------------------------------------------------------------------
def test_arguments_are_refused_without_a_device_in_the_documented_order():
    """every refusal below happens with a NULL handle: nothing of it can have looked at a device.  Each call is wrong in the
    way under test AND in every way that is checked later, so the message shows which check came first."""
    from pointcloudcomparator_amd import capi
    L = capi.LIB
    desc = np.full((8, 352), 7.0, np.float32)
    rf = np.full((8, 9), 7.0, np.float32)
    idx = np.full(8, 7, np.int32)
    n_out = ctypes.c_size_t(77)

    def call(mem=0, rn=0.05, rs=0.04, d=desc.ctypes.data, r=rf.ctypes.data, i=idx.ctypes.data, no=ctypes.byref(n_out)):
        return L.pcc_shot_descriptors(None, mem, rn, rs, d, r, i, no)

    assert call(mem=7, d=None, rn=0.0) == -1 and b"mem space" in L.pcc_last_error()
    for kw in (dict(d=None), dict(i=None), dict(no=None)):
        assert call(rn=0.0, **kw) == -1 and b"null argument" in L.pcc_last_error(), kw
    for kw in (dict(rn=0.0), dict(rn=-0.05), dict(rs=float("nan")), dict(rs=float("inf")), dict(rs=0.0), dict(rn=float("nan"))):
        assert call(**kw) == -1 and b"bad radius" in L.pcc_last_error(), kw
    assert call() == -1 and b"null index" in L.pcc_last_error()          # all arguments good: the handle is looked at last
    assert call(r=None) == -1 and b"null index" in L.pcc_last_error()    # out_rf may be NULL
    assert (desc == 7.0).all() and (rf == 7.0).all() and (idx == 7).all() and n_out.value == 77  # a refused call writes nothing


# ---- 3. the input condition -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(shot_util.SMALL))
def test_scenes_meet_the_input_condition(given, name):
    """no test below compares empty sets (float64 restatement alone)"""
    g = given(name)
    r, pts = g["ref"], g["pts"]
    in2, f = r["in2"], r["lrf"]
    rows = r["row_len"][in2]
    valid = f["valid"]
    if name in DENSE:
        assert in2.sum() >= 0.9 * len(pts) and np.median(rows) >= 10
    if name == "volume":
        assert rows.max() > 64  # more than one chunk
    if name == "five-rule":
        rl = r["row_len"]
        assert (in2 & (rl == 4)).sum() >= 5
        assert (in2 & (rl == 5) & (valid == 4)).sum() >= 5
        assert (in2 & (rl >= 6) & (valid >= 5)).sum() >= 5
        assert (in2 & (valid < rl - 1)).sum() >= 1  # a copy of p is in the row and not in `valid`
        assert (in2 & (rl >= 5) & (valid == 4)).sum() > (in2 & (rl == 5) & (valid == 4)).sum()  # row 6, valid 4: a copy alone decides
        assert len(shot_util.fpfh_util.duplicate_pairs(pts)) == 4
    if name == "short-rows":
        median_clause = sum(1 for i in np.nonzero(in2)[0] if f["dots"][i] is not None and (f["s"][i] == 0).any())
        assert median_clause >= 10
    if name == "isolated":
        assert (in2 & (r["row_len"] == 4)).sum() >= 4
    fin = np.isfinite(r["desc"]).all(1)
    assert fin.sum() >= 0.5 * len(r["index"])
    assert np.abs(np.sqrt((r["desc"][fin] ** 2).sum(1)) - 1).max() < 1e-12


# ---- 4. Jacobi alone ------------------------------------------------------------------------------------------------------------
def _jacobi_matrices(given):
    rng = np.random.default_rng(41)
    mats = []
    for name in shot_util.SMALL:  # the scenes' own covariances
        cov = given(name)["ref"]["lrf"]["cov"]
        mats.append(cov[np.isfinite(cov).all(1)])

    def sym(q, d):
        m = (q * d[:, None, :]) @ q.transpose(0, 2, 1)
        m = (m + m.transpose(0, 2, 1)) / 2
        return m[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]

    m = 2000
    q = np.linalg.qr(rng.normal(size=(m, 3, 3)))[0]
    scale = 10.0 ** rng.uniform(-12, 6, (m, 1))
    ev = rng.uniform(0, 1, (m, 3)) * scale
    mats.append(sym(q, ev))                                                      # general
    diag = np.zeros((m, 6))
    diag[:, [0, 3, 5]] = ev * (rng.uniform(0, 1, (m, 3)) > 0.2)
    mats.append(diag)                                                            # diagonal, zeros among the entries
    v = rng.normal(size=(m, 3)) * np.sqrt(scale)
    w = rng.normal(size=(m, 3)) * np.sqrt(scale)
    outer = lambda a: (a[:, :, None] * a[:, None, :])[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]
    mats.append(outer(v))                                                        # rank 1
    mats.append(outer(v) + outer(w))                                             # rank 2
    mats.append(sym(q, np.stack([ev[:, 0], ev[:, 0], ev[:, 2]], -1)))            # two equal eigenvalues, rotated
    mats.append(sym(q, np.stack([ev[:, 1], ev[:, 1], ev[:, 1]], -1)))            # three equal, up to rounding
    two = np.zeros((m, 6))
    two[:, [0, 3, 5]] = np.stack([ev[:, 0], ev[:, 0], ev[:, 2]], -1)
    two[:, 1] = ev[:, 1] * 0.5
    mats.append(two)                                                             # exactly equal diagonal entries: 45 degree rotations
    return np.concatenate(mats)


def test_jacobi_against_eigh(given, tmp_path):
    a6 = _jacobi_matrices(given)
    assert len(a6) >= 10**4
    ev, V, sweeps = shot_util.run_jacobi(a6, tmp_path)
    A = np.zeros((len(a6), 3, 3))
    A[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]] = a6
    A[:, [1, 2, 2], [0, 0, 1]] = a6[:, [1, 2, 4]]
    fro = np.sqrt((A * A).sum((1, 2)))
    assert sweeps.max() <= 32, "the sweep cap was hit"      # exact zeros within the cap on all of them
    res = np.sqrt((((A @ V) - V * ev[:, None, :]) ** 2).sum(1))   # per pair: column k
    orth = np.abs(V.transpose(0, 2, 1) @ V - np.eye(3))
    want = np.linalg.eigvalsh(A)
    dev = np.abs(np.sort(ev, 1) - want)
    nz = fro > 0
    print(f"shot_jacobi3: {len(a6)} matrices, sweeps max {int(sweeps.max())}, largest residual {np.max(res[nz] / fro[nz, None]) / 2.0**-52:.2f} x 2^-52 ||A||, "
          f"orthogonality {orth.max() / 2.0**-52:.2f} x 2^-52, eigenvalues vs eigh {np.max(dev[nz] / fro[nz, None]) / 2.0**-52:.2f} x 2^-52 ||A|| (bound 64)")
    assert (res <= JACOBI_BOUND * fro[:, None]).all()
    assert orth.max() <= JACOBI_BOUND
    assert (dev <= JACOBI_BOUND * fro[:, None]).all()


# ---- 5. frames, the normals given -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(shot_util.SMALL))
def test_frames_against_the_float64_restatement(given, name):
    g = given(name)
    ref = g["ref"]
    in2, f = ref["in2"], ref["lrf"]
    assert np.array_equal(g["index"], ref["index"])
    got, want = g["lrf"].astype(np.float64), ref["rf_all"]
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN in other words"  # (valid < 5 is an integer rule: no point is left out)
    assert np.isnan(got[~in2]).all()
    have = np.array([d is not None for d in f["dots"]])
    flagged = shot_ref.lrf_flags(f, MARGIN * LRF_DOT_F32_VS_F64[name])
    left_out = flagged[have].mean() if have.any() else 0.0
    compare = have & ~flagged
    worst, flips = 0.0, 0
    for i in np.nonzero(compare)[0]:
        for a in (0, 6):
            flips += bool(got[i, a:a + 3] @ want[i, a:a + 3] < 0)
            worst = max(worst, shot_ref._unit_angle(got[i, a:a + 3], want[i, a:a + 3]))
    print(f"{name}: {100 * left_out:.2f} % of the frames left out (at most {100 * LEFT_OUT_MAX:g}), {int(compare.sum())} compared, {flips} sign "
          f"differences, largest axis angle {worst:.3g}, float32 restatement {LRF_F32_VS_F64[name]:.3g} (bound x {MARGIN:g})")
    if name in SHARE_SCENES:
        assert left_out <= LEFT_OUT_MAX  # (the restatement alone decides this)
    assert compare.sum() >= 5
    assert flips == 0
    assert worst <= MARGIN * LRF_F32_VS_F64[name]


# ---- 6. descriptors, the frames and the normals given -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(shot_util.SMALL))
def test_descriptors_against_the_float64_restatement_over_the_mirrors_frames(given, name, tmp_path):
    g = given(name)
    desc, _, index, _ = shot_util.run_host(g["pts"], tmp_path, normals=g["nrm"], rf=g["lrf"])
    assert np.array_equal(_bits(desc), _bits(g["desc"]))  # (the frames read back are the frames estimated)
    r64 = shot_ref.shot_pipeline(g["pts"], np.float64, normals_given=g["nrm"], rf_given=g["lrf"])
    assert np.array_equal(index, r64["index"])
    want = r64["desc"]
    assert np.array_equal(np.isnan(desc), np.isnan(want)), "the NaN rows are other rows"
    fin = np.isfinite(want).all(1)
    assert np.isnan(want[~fin]).all() and fin.any()
    dev = np.abs(desc[fin].astype(np.float64) - want[fin]).max()
    norm = np.abs(np.sqrt((desc[fin].astype(np.float64) ** 2).sum(1)) - 1).max()
    t = DESC_F32_VS_F64[name]
    print(f"{name}: {int(fin.sum())} finite rows, mirror vs float64 {dev:.3g}, float32 restatement {t:.3g}, ratio {dev / t:.2f}; "
          f"|norm - 1| {norm:.3g}, ratio {norm / t:.2f} (bound {MARGIN:g})")
    assert dev <= MARGIN * t
    assert norm <= MARGIN * t


def test_tables_are_what_the_restatement_measures(given):
    for name in shot_util.SMALL:
        g = given(name)
        angle, dot, desc, _, _ = shot_ref.scene_tables(g["pts"], g["nrm"], MARGIN)
        assert np.isclose(angle, LRF_F32_VS_F64[name], rtol=0.02), (name, angle)
        assert np.isclose(dot, LRF_DOT_F32_VS_F64[name], rtol=0.02), (name, dot)
        assert np.isclose(desc, DESC_F32_VS_F64[name], rtol=0.02), (name, desc)


# ---- 7. exact cases ----------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", ["duplicates", "five-rule"])
def test_copies_of_a_point_carry_equal_bits(mirror, name):
    pts = shot_util.scene(name)
    desc, rf, index = mirror(name)
    assert np.array_equal(index, np.arange(len(pts)))
    pairs = shot_util.fpfh_util.duplicate_pairs(pts)
    assert len(pairs) == (20 if name == "duplicates" else 4)
    for a, b in pairs:
        assert np.array_equal(_bits(desc[a]), _bits(desc[b])) and np.array_equal(_bits(rf[a]), _bits(rf[b])), (a, b)


@pytest.mark.parametrize("name", ["isolated", "five-rule"])
def test_four_point_groups_are_nan_in_every_word(given, mirror, name):
    desc, rf, index = mirror(name)
    ref = given(name)["ref"]
    four = np.nonzero(ref["in2"] & (ref["row_len"] == 4))[0]
    assert len(four) >= 4
    at = np.searchsorted(index, four)
    assert np.array_equal(index[at], four)
    assert np.isnan(desc[at]).all() and np.isnan(rf[at]).all()  # all 352 + 9 words


@pytest.mark.parametrize("name", list(shot_util.SMALL))
def test_kept_indices_are_the_points_with_a_finite_normal(mirror, name):
    pts = shot_util.scene(name)
    nrm = oracle.normals_radius(np.ascontiguousarray(pts), 0.05)[:, :3]
    assert np.array_equal(mirror(name)[2], np.nonzero(np.isfinite(nrm).all(1))[0])


def test_big_scene_meets_the_input_condition():
    """the 20 000-point cluster of the GPU test and of tools/exp_shot.py (too large for the O(n^2) restatement): rows counted on a sample"""
    p = shot_util.scene("volume20000")
    sample = p[::20]
    d = sample[:, None, :] - p[None, :, :]
    rows = ((d * d).sum(-1) < np.float32(0.04 * 0.04)).sum(1)
    assert np.median(rows) >= 10 and rows.max() > 64


# ---- 8. the stand-alone tool under ASan and UBSan ------------------------------------------------------------------------------------
def test_host_mirror_is_clean_under_the_sanitizers(tmp_path):
    subprocess.check_call(["make", "build/asan/shot_host"], cwd=ROOT)
    r = subprocess.run([str(ROOT / "build" / "asan" / "shot_host"), "--self", str(tmp_path / "self.bin")], capture_output=True, text=True,
                       timeout=300, env={"ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0 and "shot_host n=240" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    desc, rf, index = shot_util.read_result(tmp_path / "self.bin")
    assert 200 <= len(index) < 240 and np.isfinite(desc).all(1).sum() >= 200
