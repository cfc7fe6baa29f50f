"""NormalEstimation (K neighbours) and RegionGrowing on the GPU against the oracle's restatements
(reference: src/segmentation.cpp:232-271 -- K = 50 normals, RegionGrowing with 100 neighbours, 3 degrees,
curvature threshold 1, cluster sizes 50..1000000)."""
import numpy as np
import pytest

import oracle
from pointcloudcomparator_amd import capi, synth

pytestmark = pytest.mark.gpu


def _room(n_per=3000, seed=3, noise=0.002):
    """three orthogonal walls + a sphere: planar regions with distinct normals and a curved blob"""
    rng = np.random.default_rng(seed)
    u, v = rng.random((2, n_per)).astype(np.float32) * 2.0
    floor = np.stack([u, v, np.zeros_like(u)], 1)
    u, v = rng.random((2, n_per)).astype(np.float32) * 2.0
    wall1 = np.stack([u, np.zeros_like(u), v], 1)
    u, v = rng.random((2, n_per)).astype(np.float32) * 2.0
    wall2 = np.stack([np.zeros_like(u), u, v], 1)
    d = rng.normal(size=(n_per, 3))
    ball = (d / np.linalg.norm(d, axis=1, keepdims=True) * 0.3 + np.array([1.0, 1.0, 1.0])).astype(np.float32)
    pts = np.concatenate([floor, wall1, wall2, ball]).astype(np.float32)
    pts += rng.normal(0, noise, pts.shape).astype(np.float32)
    pts += np.float32(3.0)  # away from the origin: PCL's single-pass float covariance is sensitive here
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


def _same_bits(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _assert_normals_close(got, want, min_same=None):
    """Covariance, scaling, cross products and the flip are the same float operations on both sides, and so -- since
    round 5 -- are the three transcendental calls of the closed-form roots: csrc/libm_f32.hpp restates the host libm's
    atan2f / cosf / sinf (glibc 2.35) operation for operation, tests/test_libm_cpu.py pins it.  Every normal and every
    curvature carries the oracle's bits; rows that are NaN are NaN on both sides.  (Until round 5 the device rounded
    double results once and 2.3 % of all points differed in their last bits.)"""
    same = _same_bits(got, want).all(axis=1)
    assert same.all(), (int((~same).sum()), len(same), np.nonzero(~same)[0][:5])


@pytest.mark.parametrize("k", [3, 10, 50])
def test_normals_match_oracle_on_the_same_neighbourhoods(k):
    pts = _room()
    ix = capi.Index(pts)
    got = ix.normals(k)
    nbr, _ = ix.knn(pts, k)
    want = oracle.normals(pts, k, neighbours=nbr)
    _assert_normals_close(got, want)
    # unit length, flipped towards the origin
    ok = np.isfinite(got).all(axis=1)  # k = 3 leaves a few degenerate covariances (0/0), as in PCL
    assert ok.mean() > 0.99
    ln = np.linalg.norm(got[ok, :3].astype(np.float64), axis=1)
    np.testing.assert_allclose(ln, 1.0, atol=1e-5)
    assert ((got[ok, :3] * -pts[ok]).sum(1) >= -1e-6).all()


def test_normals_against_the_kdtree_oracle():
    """the full restatement (FLANN tree order) differs only where neighbours tie in distance"""
    pts = _room(1500, seed=5)
    ix = capi.Index(pts)
    got = ix.normals(50)
    want = oracle.normals(pts, 50)
    dots = np.abs((got[:, :3].astype(np.float64) * want[:, :3]).sum(1))
    assert (dots > 1 - 1e-6).mean() > 0.999
    assert np.median(np.abs(got[:, 3] - want[:, 3])) < 1e-7


def test_normals_viewpoint_and_device_output():
    import torch
    pts = _room(1000, seed=7)
    ix = capi.Index(pts)
    vp = np.array([10.0, 10.0, 10.0], np.float32)
    host = ix.normals(20, viewpoint=vp)
    dev = ix.normals(20, viewpoint=vp, device="cuda:0").cpu().numpy()
    assert _same_bits(host, dev).all()
    assert ((host[:, :3] * (vp - pts)).sum(1) >= -1e-6).all()
    want = oracle.normals(pts, 20, viewpoint=vp, neighbours=ix.knn(pts, 20)[0])
    _assert_normals_close(host, want)


def test_normals_edge_cases():
    # fewer than three points -> NaN (PCL: indices.size() < 3); k larger than the cloud is clamped
    two = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    assert np.isnan(capi.Index(two).normals(50)).all()
    pts = _room(200, seed=11)[:40].copy()
    pts[7] = np.nan
    ix = capi.Index(pts)
    got = ix.normals(100)
    assert np.isnan(got[7]).all() and np.isfinite(np.delete(got, 7, 0)).all()
    nbr, _ = ix.knn(pts, 100)
    want = oracle.normals(pts, 100, neighbours=nbr)
    _assert_normals_close(got, want, 0.8)
    with pytest.raises(capi.PccError):
        ix.normals(0)


@pytest.mark.parametrize("k,theta_deg,curv_thr,min_size", [(100, 3.0, 1.0, 50), (30, 6.0, 0.05, 20), (10, 3.0, 1.0, 1)])
def test_region_growing_matches_oracle(k, theta_deg, curv_thr, min_size):
    pts = _room()
    ix = capi.Index(pts)
    nrm = ix.normals(50)
    labels, ncl = ix.region_growing(nrm, k=k, smoothness=theta_deg / 180.0 * np.pi, curvature_threshold=curv_thr,
                                    min_size=min_size, max_size=1000000)
    nbr, _ = ix.knn(pts, k)
    want, want_n = oracle.region_growing(nrm, nbr, theta_deg / 180.0 * np.pi, curv_thr, min_size, 1000000)
    assert ncl == want_n
    np.testing.assert_array_equal(labels, want)
    if min_size == 50:
        # the three walls come out as large regions
        sizes = np.sort(np.bincount(labels[labels >= 0]))[::-1]
        assert ncl >= 3 and sizes[2] > 1500


def test_region_growing_device_normals_and_size_filter():
    import torch
    pts = _room(1500, seed=13)
    ix = capi.Index(pts)
    nrm = ix.normals(50, device="cuda:0")
    lab_d, n_d = ix.region_growing(nrm, k=40, min_size=100, max_size=1400)
    lab_h, n_h = ix.region_growing(nrm.cpu().numpy(), k=40, min_size=100, max_size=1400)
    assert n_d == n_h
    np.testing.assert_array_equal(lab_d.cpu().numpy(), lab_h)
    cnt = np.bincount(lab_h[lab_h >= 0], minlength=max(n_h, 1))
    assert n_h == 0 or ((cnt >= 100) & (cnt <= 1400)).all()


@pytest.mark.parametrize("seed,k,theta_deg,nan_frac,curv_thr", [
    (1, 8, 25.0, 0.0, 1.0), (2, 16, 35.0, 0.01, 1.0), (3, 5, 50.0, 0.0, 1.0), (4, 40, 15.0, 0.002, 1.0), (5, 3, 80.0, 0.05, 1.0),
    # points above the curvature threshold join a region without spreading -- unless they seed one themselves
    (6, 8, 40.0, 0.0, 0.15), (7, 12, 60.0, 0.01, 0.05), (8, 4, 85.0, 0.03, 0.25), (9, 20, 30.0, 0.0, 0.0), (10, 6, 89.0, 0.02, 0.29)])
def test_region_growing_order_free_form_equals_pcl_walk(seed, k, theta_deg, nan_frac, curv_thr):
    """Adversarial graphs for the GPU formulation (label = lowest-ranked ancestor): random normals make
    the smooth-edge graph sparse, strongly one-directional and full of small components, NaN normals
    accept every edge, duplicated curvatures exercise the rank tie-break.  The result must equal the
    sequential walk of the oracle, label for label."""
    rng = np.random.default_rng(seed)
    n = 20000
    pts = rng.random((n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    nrm = np.zeros((n, 4), np.float32)
    nrm[:, :3] = d / np.linalg.norm(d, axis=1, keepdims=True)
    nrm[:, 3] = np.round(rng.random(n) * 0.3, 3)  # many equal curvatures
    bad = rng.random(n) < nan_frac
    nrm[bad] = np.nan
    ix = capi.Index(pts)
    labels, ncl = ix.region_growing(nrm, k=k, smoothness=theta_deg / 180.0 * np.pi, curvature_threshold=curv_thr,
                                    min_size=1, max_size=n)
    nbr, _ = ix.knn(pts, k)
    want, want_n = oracle.region_growing(nrm, nbr, theta_deg / 180.0 * np.pi, curv_thr, 1, n)
    assert ncl == want_n
    np.testing.assert_array_equal(labels, want)
    assert ncl > 10


@pytest.mark.parametrize("radius", [0.03, 0.06, 0.15])
def test_normals_with_radius_search(radius):
    """NormalEstimation::setRadiusSearch (the RIFT pipeline's normals, src/comparator.cpp:628-635): neighbourhood =
    sorted radius search result"""
    pts = _room(2500, seed=21)
    pts[11] = np.nan
    ix = capi.Index(pts)
    got = ix.normals_radius(radius)
    want = oracle.normals_radius(pts, radius)
    assert np.isnan(got[11]).all() and np.isnan(want[11]).all()
    # same rows (sorted by (d2, index); FLANN's tie order differs only where distances tie), same arithmetic
    both_nan = np.isnan(got).all(1) & np.isnan(want).all(1)
    assert (np.isnan(got).all(1) == np.isnan(want).all(1)).all()
    ok = ~both_nan
    same = (got[ok].view(np.uint32) == want[ok].view(np.uint32)).all(axis=1)
    assert same.mean() > 0.99                  # (all but the rows where two neighbours tie in distance)
    dots = np.abs((got[ok, :3].astype(np.float64) * want[ok, :3]).sum(1))
    assert (dots > 1 - 1e-5).all()
    np.testing.assert_allclose(got[ok, 3], want[ok, 3], rtol=0, atol=1e-6)
    if radius == 0.03:
        assert both_nan.sum() > 1  # sparse corners: fewer than 3 points within 3 cm


def test_normals_radius_into_device_memory_equals_the_host_call():
    """pcc_normals_radius with PCC_MEM_DEVICE writes the caller's device array itself; 1000 points, the host call's bits"""
    import ctypes as C
    import torch
    pts = _room(n_per=250)
    with capi.Index(pts) as ix:
        host = ix.normals_radius(0.3)
        dev = torch.zeros((len(pts), 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        assert capi.LIB.pcc_normals_radius(ix._h, C.c_double(0.3), None, capi.MEM_DEVICE, dev.data_ptr()) == 0
        ix.sync()
        assert np.isfinite(host).all(1).sum() > 900 and _same_bits(dev.cpu().numpy(), host).all()


# ---- degenerate neighbourhoods through k_normals' own accumulation ---------------------------------------------------------
# tests/cpp/test_device_math.hip runs the plane fit function by function; these clouds run the kernels' sums as well, at the
# neighbourhoods the painted rooms never produce.  2000 points each (the rooms: 4 x 500), one row non-finite.  The radius is
# one per cloud, chosen so that most rows hold 3 to 100 neighbours.
def _degenerate_cloud(name):
    rng = np.random.default_rng(97)
    n = 2000
    if name == "plane_z0":          # an exact plane: the smallest root is 0 up to the cubic's rounding
        pts = np.concatenate([rng.random((n, 2)), np.zeros((n, 1))], 1)
    elif name == "plane_z3_grid":   # an exact plane away from the origin, every coordinate on a 2^-8 grid: exact sums
        pts = np.concatenate([3.0 + rng.integers(0, 256, (n, 2)) / 256.0, np.full((n, 1), 3.0)], 1)
    elif name == "lattice":         # pitch 2^-4: every neighbourhood is full of distance ties
        g = np.stack(np.meshgrid(*[np.arange(13)] * 3, indexing="ij"), -1).reshape(-1, 3)
        pts = g[rng.permutation(len(g))[:n]] / 16.0
    elif name == "line_x":          # on the x axis: two rows of the covariance are exactly zero, every cross product too: NaN
        pts = np.stack([rng.permutation(4096)[:n] / 1024.0, np.zeros(n), np.zeros(n)], 1)
    elif name == "line_diagonal":   # (t, 2t, 3t), t of 22 bits so that 3t is exact: rank 1 only up to the rounding of the sums,
        t = rng.integers(0, 1 << 22, n) / float(1 << 20)  # normals made of rounding noise; no regular spacing, so few distance ties
        pts = np.stack([t, 2.0 * t, 3.0 * t], 1)
    elif name == "duplicates":      # 40 points on a 2^-4 grid, 50 times each: every k <= 50 neighbourhood is one point, its
        pts = np.repeat(rng.permutation(4096)[:40, None] // np.array([1, 16, 256]) % 16 / 16.0, 50, axis=0)[rng.permutation(n)]  # sums exact: the zero matrix
    elif name == "room_1e-6":
        pts = _room(500).astype(np.float64) * 1e-6
    elif name == "room_1e4":
        pts = _room(500).astype(np.float64) * 1e4
    elif name == "room_offset_1000":  # the single-pass float covariance cancels: zero and negative variances
        pts = _room(500).astype(np.float64) + 1000.0
    else:
        raise KeyError(name)
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    assert pts.shape == (n, 3)
    pts[1234] = (np.nan, np.inf, -np.inf) if name == "line_x" else np.nan
    return pts


# cloud -> (radius, share of rows whose neighbour list holds a distance tie as the oracle's exhaustive search gives it, what
# is asked of those rows).  A tie row may be summed in another order on the two sides (FLANN's order against (d2, index)):
#   "bits"  the sums do not depend on the order, so tie rows carry the oracle's bits like every other row.  lattice:
#           coordinates m / 16 with m <= 12, at most 33 neighbours: every product and every partial sum is an integer below
#           2^13 in units of 2^-8, exact in float.  duplicates: within 0.05 on a 1 / 16 grid there is one point, 50 times: 50
#           equal terms.  line_x: y = z = 0 make two rows of the covariance exactly zero in any order, c0 = 0, the smallest
#           root 0 and every cross product 0: NaN normal and curvature 0 whatever x sums to.
#   "weak"  the rule of test_normals_with_radius_search: |dot| > 1 - 1e-5, curvature within 1e-6.  The plane at z = 3 has 10-bit
#           coordinates and up to 38 neighbours: partial sums pass 2^24 and round by order, the normal stays (0, 0, +-1).
#   "nan"   only the NaN rule that holds for every row (fewer than 3 neighbours: NaN on both sides): the normals of the
#           diagonal line and of the room at offset 1000 are made of rounding noise, so a tie row there has no direction to
#           compare.  The oracle finds 10 such rows on the line and none at offset 1000.
_DEGENERATE = {
    "plane_z0": (0.05, 0.0, "weak"),
    "plane_z3_grid": (0.06, 0.911, "weak"),
    "lattice": (0.13, 1.0, "bits"),
    "line_x": (0.01, 0.9365, "bits"),
    "line_diagonal": (0.04, 0.005, "nan"),
    "duplicates": (0.05, 1.0, "bits"),
    "room_1e-6": (0.12e-6, 0.0, "weak"),
    "room_1e4": (0.12e4, 0.0, "weak"),
    "room_offset_1000": (0.12, 0.0, "nan"),
}


def _tie_rows(pts, radius):
    """rows whose radius neighbourhood, sorted by distance, holds two equal distances (the oracle's exhaustive search):
    there FLANN's order and the (d2, index) order may sum the same points in a different order"""
    cnt = oracle.radius_count_exhaustive(pts, pts, radius)
    kmax = max(int(cnt.max()), 2)
    _, d2 = oracle.knn_exhaustive(pts, pts, kmax)
    col = np.arange(kmax - 1)[None, :]
    return ((d2[:, 1:] == d2[:, :-1]) & (col + 1 < cnt[:, None])).any(axis=1), cnt


@pytest.mark.parametrize("name", list(_DEGENERATE))
def test_normals_of_degenerate_neighbourhoods(name):
    pts = _degenerate_cloud(name)
    ix = capi.Index(pts)
    for k in (3, 10, 50):
        got = ix.normals(k)
        want = oracle.normals(pts, k, neighbours=ix.knn(pts, k)[0])
        assert np.isnan(got[1234]).all()
        _assert_normals_close(got, want)
    # the class the cloud is there for (k = 50, still in got / want)
    ok = np.arange(len(pts)) != 1234
    if name.startswith("plane"):
        assert (got[ok, 3] == 0).mean() > 0.5 and np.isfinite(got[ok]).all()
    if name == "line_x":
        assert np.isnan(got[ok, :3]).all()
    if name == "duplicates":  # (sum / k can round an ulp off the coordinate for k = 50: such a group gets a normal of rounding noise)
        assert np.isnan(got[ok, :3]).all(axis=1).mean() > 0.9 and (got[ok, 3] == 0).all()
    if name == "line_diagonal":
        assert (got[ok, 3] == 0).mean() > 0.5
    if name == "room_offset_1000":
        assert (got[ok, 3] == 0).mean() > 0.5  # zero and negative variances: the smallest root is clamped to 0
    radius, tie_share, tie_rule = _DEGENERATE[name]
    got = ix.normals_radius(radius)
    want = oracle.normals_radius(pts, radius)
    tie, cnt = _tie_rows(pts, radius)
    assert ((cnt >= 3) & (cnt <= 100)).mean() > 0.5
    assert abs(tie[ok].mean() - tie_share) <= 0.02, tie[ok].mean()
    # every row: fewer than 3 neighbours (the non-finite row has none) is NaN on both sides, whatever the order
    few = cnt < 3
    assert few[1234] and np.isnan(got[few]).all() and np.isnan(want[few]).all()
    # the oracle's bits on every row without a tie, and on the tie rows too where the sums are order-free
    exact = np.ones(len(pts), bool) if tie_rule == "bits" else ~tie
    assert (exact & ~few).sum() > 100  # rows with a neighbourhood to fit, compared bit for bit
    same = _same_bits(got, want).all(axis=1)
    assert same[exact].all(), (int((~same[exact]).sum()), int(exact.sum()), np.nonzero(~same & exact)[0][:5])
    if tie_rule == "weak" and (~exact).any():
        g, w = got[~exact], want[~exact]
        assert (np.isnan(g) == np.isnan(w)).all()
        fin = np.isfinite(g).all(axis=1)
        dots = np.abs((g[fin, :3].astype(np.float64) * w[fin, :3]).sum(1))
        assert (dots > 1 - 1e-5).all()
        np.testing.assert_allclose(g[fin, 3], w[fin, 3], rtol=0, atol=1e-6)
