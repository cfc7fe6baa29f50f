"""Shared by the pcc_plane_removal tests: the scenes, the oracle's plane-removal loop (reference src/segmentation.cpp:88-117
over oracle.sac_plane + np.delete), a replay of the first sample batch of a turn, and a raw C-ABI call with sentinel-filled
outputs for the refusal tests."""
import ctypes as C
import functools

import numpy as np

import oracle


def plane_scene(n_plane, n_clutter, seed, noise=0.005, tilt=(0.1, -0.2, 1.0), offset=0.5):
    """tests/test_sac_gpu.py's _scene: a noisy plane patch of 3 x 3 plus uniform clutter, shuffled"""
    rng = np.random.default_rng(seed)
    nrm = np.asarray(tilt, np.float64)
    nrm /= np.linalg.norm(nrm)
    e1 = np.cross(nrm, [1.0, 0, 0] if abs(nrm[0]) < 0.9 else [0, 1.0, 0]); e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    uv = rng.random((n_plane, 2)) * 3
    plane = uv[:, :1] * e1 + uv[:, 1:] * e2 + offset * nrm + rng.normal(0, noise, (n_plane, 1)) * nrm
    clutter = rng.random((n_clutter, 3)) * 3 - 0.5
    pts = np.concatenate([plane, clutter]).astype(np.float32)
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


def three_planes(seed=1):
    """250 / 200 / 150 points on planes with normals along z, x, y plus 100 clutter points, shuffled: 700 points"""
    rng = np.random.default_rng(seed)
    a = plane_scene(250, 0, seed + 1, tilt=(0, 0, 1), offset=0.0)
    b = plane_scene(200, 0, seed + 2, tilt=(1, 0, 0), offset=-0.5)
    c = plane_scene(150, 0, seed + 3, tilt=(0, 1, 0), offset=-0.25)
    clutter = (rng.random((100, 3)) * 3 - 0.5).astype(np.float32)
    pts = np.concatenate([a, b, c, clutter])
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


def long_scene():
    """the 700-point scene repeated with further seeds (2100 points): its first 255 ... 2049 points straddle the edges of a
    workgroup of the partition (256) and of a block of the scan (2048)"""
    return np.ascontiguousarray(np.concatenate([three_planes(1), three_planes(2), three_planes(3)]))


def lattice():
    g = np.stack(np.meshgrid(np.arange(7.0), np.arange(7.0)), -1).reshape(-1, 2)
    return np.ascontiguousarray(np.concatenate([g, np.full((49, 1), 2.0)], 1).astype(np.float32))


def with_nans():
    pts = three_planes(1).copy()
    pts[::9, 1] = np.nan
    return pts


def duplicates(seed=3):
    return np.ascontiguousarray(three_planes(1)[np.random.default_rng(seed).integers(0, 700, 3000)])


def two_plane_room():
    """the 33 000-point scene of tests/test_sac_gpu.py::test_plane_removal_loop_like_the_reference"""
    rng = np.random.default_rng(11)
    a = plane_scene(15000, 0, 1, tilt=(0, 0, 1), offset=0.0)
    b = plane_scene(12000, 0, 2, tilt=(1, 0, 0), offset=-0.5)
    c = (rng.random((6000, 3)) * 0.5 + 1.0).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([a, b, c])[rng.permutation(33000)])


def oracle_loop(pts, stop_fraction, max_planes=None, optimize=True):
    """(remaining_index, plane_of_point, coefficients (p, 4), sizes, iterations, ended_without_model, first-batch flags): the
    loop of the issue over oracle.sac_plane, original indices tracked.  xyz = the first three columns."""
    xyz = np.ascontiguousarray(pts[:, :3])
    n = len(xyz)
    cur, orig = xyz, np.arange(n, dtype=np.int32)
    pop = np.full(n, -1, np.int32)
    coeff, sizes, its, degenerate = [], [], [], []
    ended = False
    while float(len(cur)) > stop_fraction * float(n):
        if max_planes is not None and len(sizes) == max_planes:
            break
        degenerate.append(first_batch_degenerate(cur))
        inl, c, it = oracle.sac_plane(cur, 100, 0.02, 0.99, optimize)
        if len(inl) == 0:
            ended = True
            break
        pop[orig[inl]] = len(sizes)
        coeff.append(np.array(c, np.float32)); sizes.append(len(inl)); its.append(it)
        cur = np.ascontiguousarray(np.delete(cur, inl, 0))
        orig = np.delete(orig, inl)
    return (orig, pop, np.array(coeff, np.float32).reshape(-1, 4), np.array(sizes, np.uint32), np.array(its, np.int32), ended,
            degenerate)


@functools.lru_cache(maxsize=None)
def cached_loop(scene, stop_fraction, head=None):
    """oracle_loop over a named scene (computed once per session; the arrays are shared: do not write to them)"""
    pts = SCENES[scene]()
    if head is not None:
        pts = np.ascontiguousarray(pts[:head])
    return pts, oracle_loop(pts, stop_fraction)


SCENES = dict(three=three_planes, long=long_scene, lattice=lattice, nans=with_nans, dup=duplicates, room=two_plane_room)


def first_batch_degenerate(cur):
    """Whether the FIRST batch of 32 samples of a RANSAC turn over `cur` holds a degenerate sample.  PCL's sampling replayed:
    mt19937(12345), eng() / 2, three swaps i <-> i + rnd % (n - i) of the shuffled index array per sample, the sample its first
    three entries; degenerate when (p1 - p0) / (p2 - p0) is equal on all three axes (float).  With max_iterations >= 31 the
    library draws these 32 samples before it has any count, so such a turn on a cloud in device memory must take the host copy."""
    n = len(cur)
    if n < 3:
        return False
    gen = np.random.MT19937()
    gen._legacy_seeding(12345)
    raw = gen.random_raw(96)
    shuffled = {}
    k = 0
    for _ in range(32):
        for i in range(3):
            j = i + (int(raw[k]) // 2) % (n - i)
            k += 1
            shuffled[i], shuffled[j] = shuffled.get(j, j), shuffled.get(i, i)
        p0, p1, p2 = (cur[shuffled.get(i, i)].astype(np.float32) for i in range(3))
        with np.errstate(all="ignore"):
            d = (p1 - p0) / (p2 - p0)
        if d[0] == d[1] and d[2] == d[1]:
            return True
    return False


SENTINEL = 0x5A


class RawCall:
    """pcc_plane_removal through ctypes with every output filled with SENTINEL bytes: status, and whether anything was written"""

    def __init__(self, n=8, max_planes=4):
        self.pts = np.zeros((n, 8), np.float32)
        self.pts[:, :3] = np.arange(3 * n, dtype=np.float32).reshape(n, 3) * 0.01
        self.out = dict(coeff=np.zeros((max_planes, 4), np.float32), sizes=np.zeros(max_planes, np.uint32), its=np.zeros(max_planes, np.int32),
                        n_planes=np.zeros(1, np.uintp), ended=np.zeros(1, np.int32), pop=np.zeros(n, np.int32), rem=np.zeros(n, np.int32),
                        n_rem=np.zeros(1, np.uintp), points=np.zeros((n, 8), np.float32))
        self.max_planes = max_planes
        self.n = n

    def __call__(self, handle, **kw):
        from pointcloudcomparator_amd import capi
        for a in self.out.values():
            a.view(np.uint8)[...] = SENTINEL
        o = {k: v.ctypes.data for k, v in self.out.items()}
        a = dict(pts=self.pts.ctypes.data, n=self.n, stride=32, mem=0, stop=0.3, its_max=100, thr=0.02, prob=0.99, opt=1, max_planes=self.max_planes,
                 out_stride=32, record=32, **o)
        a.update(kw)
        return capi.LIB.pcc_plane_removal(handle, a["pts"], a["n"], a["stride"], a["mem"], a["stop"], a["its_max"], a["thr"], a["prob"], a["opt"],
                                          a["max_planes"], a["coeff"], a["sizes"], a["its"], C.cast(a["n_planes"], C.POINTER(C.c_size_t)),
                                          C.cast(a["ended"], C.POINTER(C.c_int)), a["pop"], a["rem"], C.cast(a["n_rem"], C.POINTER(C.c_size_t)),
                                          a["points"], a["out_stride"], a["record"])

    def untouched(self):
        return all((a.view(np.uint8) == SENTINEL).all() for a in self.out.values())


# (keyword arguments of RawCall, the status): every refusal of the issue's list.  -1 PCC_ERR_INVALID, -5 PCC_ERR_UNSUPPORTED
REFUSALS = [
    (dict(mem=7), -1),                      # what pcc_sac_plane refuses: a bad memory space,
    (dict(pts=None), -1),                   # a null cloud with n > 0,
    (dict(stride=10), -1),                  # a bad stride,
    (dict(stride=8), -1),
    (dict(n=2 ** 31), -5),                  # 2^31 points,
    (dict(its_max=-1), -1),                 # bad RANSAC parameters
    (dict(thr=-0.5), -1),
    (dict(thr=float("nan")), -1),
    (dict(prob=0.0), -1),
    (dict(prob=1.0), -1),
    (dict(stop=-0.1), -1),                  # stop_fraction negative or not finite
    (dict(stop=float("nan")), -1),
    (dict(stop=float("inf")), -1),
    (dict(n_planes=None), -1),              # null counts
    (dict(n_rem=None), -1),
    (dict(coeff=None), -1),                 # null host tables with max_planes > 0
    (dict(sizes=None), -1),
    (dict(record=10), -1),                  # record_bytes / out_stride_bytes with out_points given
    (dict(record=8), -1),
    (dict(record=36), -1),
    (dict(record=32, out_stride=16), -1),
    (dict(record=16, out_stride=18), -1),
]
