"""The morphological ground filter without a GPU: pcc_pmf_windows against the NumPy restatement (tests/ground_util.py), and every
refusal of the three device entry points that happens before the handle is looked at (a NULL handle comes last)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ground_util as gu

ROOT = Path(__file__).resolve().parent.parent
NAMES = ["pcc_pmf_windows", "pcc_morphological_operator", "pcc_progressive_morphological_filter", "pcc_ground_segmentation"]


def test_symbols_are_exported():
    from pointcloudcomparator_amd import capi
    for name in NAMES:
        assert name in capi.SYMBOLS and hasattr(capi.LIB, name)
    assert callable(capi.pmf_windows) and callable(capi.Index.morphological_operator)
    assert callable(capi.Index.progressive_morphological_filter) and callable(capi.Index.ground_segmentation)


def test_reference_table():
    from pointcloudcomparator_amd import capi
    w, h = capi.pmf_windows(**gu.REFERENCE)
    assert w.tolist() == [3.0, 5.0, 9.0, 17.0, 33.0] and h.tolist() == [0.5, 2.5, 3.0, 3.0, 3.0]
    rw, rh = gu.pmf_windows(**gu.REFERENCE)
    assert np.array_equal(w, rw) and np.array_equal(h, rh)


@pytest.mark.parametrize("params", [
    dict(gu.REFERENCE, exponential=False),                                          # the linear form
    dict(gu.TERRAIN), dict(gu.TERRAIN, exponential=False),
    dict(max_window_size=40, slope=0.7, initial_distance=0.15, max_distance=2.5, cell_size=0.3, base=1.7, exponential=True),
    dict(max_window_size=33, slope=1.3, initial_distance=0.2, max_distance=1e9, cell_size=0.37, base=2.6, exponential=False),
    dict(max_window_size=100, slope=3.0, initial_distance=0.1, max_distance=0.6, cell_size=1.0, base=3.0, exponential=True),  # hits max_distance
    dict(gu.REFERENCE, max_window_size=0), dict(gu.REFERENCE, max_window_size=-3),  # no window at all
    dict(gu.REFERENCE, max_window_size=3),                                          # 3 is not below 3: one window
])
def test_tables_match_the_restatement(params):
    from pointcloudcomparator_amd import capi
    w, h = capi.pmf_windows(**params)
    rw, rh = gu.pmf_windows(**params)
    assert len(w) == len(rw) and np.array_equal(w, rw) and np.array_equal(h, rh)
    if params["max_window_size"] > 0:
        assert w[-1] >= params["max_window_size"] and (len(w) == 1 or w[-2] < params["max_window_size"])
        assert (h <= np.float32(params["max_distance"])).all()


def test_a_table_that_hits_max_distance():
    from pointcloudcomparator_amd import capi
    _, h = capi.pmf_windows(max_window_size=100, slope=3.0, initial_distance=0.1, max_distance=0.6, cell_size=1.0, base=3.0)
    assert h[0] == np.float32(0.1) and (h[1:] == np.float32(0.6)).all() and len(h) >= 3


def test_overflow_of_capacity():
    from pointcloudcomparator_amd import capi
    with pytest.raises(capi.PccError) as e:
        capi.pmf_windows(**gu.REFERENCE, capacity=3)
    assert e.value.status == -6 and e.value.n_windows == 5
    w = np.full(4, -1.0, np.float32)
    h = np.full(4, -1.0, np.float32)
    nw = C.c_size_t(0)
    st = capi.LIB.pcc_pmf_windows(20, 1.0, 0.5, 3.0, 1.0, 2.0, 1, 3, w.ctypes.data, h.ctypes.data, C.byref(nw))
    assert st == -6 and nw.value == 5 and w.tolist() == [3.0, 5.0, 9.0, -1.0] and h.tolist() == [0.5, 2.5, 3.0, -1.0]
    # the library's own cap: a base just above 1 needs more than 64 windows
    with pytest.raises(capi.PccError) as e:
        capi.pmf_windows(max_window_size=1000, cell_size=1.0, base=1.0001)
    assert e.value.status == -6 and e.value.n_windows == capi.PMF_MAX_WINDOWS + 1
    with pytest.raises(capi.PccError) as e:
        capi.pmf_windows(max_window_size=1000, cell_size=1.0, base=1.0, exponential=False)
    assert e.value.status == -6 and e.value.n_windows == capi.PMF_MAX_WINDOWS + 1
    w64, _ = capi.pmf_windows(max_window_size=129, cell_size=1.0, base=1.0, exponential=False)
    assert len(w64) == 64 and w64[-1] == 129.0


NAN, INF = float("nan"), float("inf")
PMF_REFUSALS = [
    (dict(slope=NAN), b"finite"), (dict(slope=INF), b"finite"), (dict(initial_distance=NAN), b"finite"),
    (dict(initial_distance=-INF), b"finite"), (dict(max_distance=NAN), b"finite"), (dict(max_distance=INF), b"finite"),
    (dict(cell_size=NAN), b"finite"), (dict(cell_size=INF), b"finite"), (dict(base=NAN), b"finite"), (dict(base=INF), b"finite"),
    (dict(cell_size=0.0), b"cell size"), (dict(cell_size=-1.0), b"cell size"),
    (dict(base=1.0), b"base must exceed 1"), (dict(base=0.5), b"base must exceed 1"),
    (dict(base=0.0, exponential=False), b"base must be positive"), (dict(base=-2.0, exponential=False), b"base must be positive"),
]


@pytest.mark.parametrize("kw,message", PMF_REFUSALS)
def test_pmf_windows_refusals(kw, message):
    from pointcloudcomparator_amd import capi
    with pytest.raises(capi.PccError) as e:
        capi.pmf_windows(**dict(gu.REFERENCE, **kw))
    assert e.value.status == -1 and message.decode() in str(e.value) and e.value.n_windows == 0


def test_pmf_windows_null_outputs():
    from pointcloudcomparator_amd import capi
    w = np.zeros(8, np.float32)
    nw = C.c_size_t(7)
    assert capi.LIB.pcc_pmf_windows(20, 1.0, 0.5, 3.0, 1.0, 2.0, 1, 8, w.ctypes.data, w.ctypes.data, None) == -1
    assert capi.LIB.pcc_pmf_windows(20, 1.0, 0.5, 3.0, 1.0, 2.0, 1, 8, None, w.ctypes.data, C.byref(nw)) == -1
    assert capi.LIB.pcc_pmf_windows(20, 1.0, 0.5, 3.0, 1.0, 2.0, 1, 8, w.ctypes.data, None, C.byref(nw)) == -1
    assert nw.value == 7 and b"null output" in capi.LIB.pcc_last_error()
    # counting alone needs no arrays
    assert capi.LIB.pcc_pmf_windows(20, 1.0, 0.5, 3.0, 1.0, 2.0, 1, 0, None, None, C.byref(nw)) == -6 and nw.value == 5


# ---- the device entry points, NULL handle -----------------------------------------------------------------------------------
class Raw:
    """the three calls with good arguments and a NULL handle; keywords replace single arguments"""

    def __init__(self):
        self.pts = np.zeros((8, 4), np.float32)
        self.out = np.full((8, 4), 7.0, np.float32)
        self.out2 = np.full((8, 4), 7.0, np.float32)
        self.out3 = np.full((8, 4), 7.0, np.float32)
        self.z = np.full(8, 7.0, np.float32)
        self.idx = np.full(8, 7, np.int32)
        self.sizes = np.full(64, 7, np.uintp)
        self.nv, self.ng = C.c_size_t(7), C.c_size_t(7)

    def _pmf(self, kw):
        p = dict(gu.REFERENCE)
        p.update({k: kw.pop(k) for k in list(kw) if k in p})
        return (int(p["max_window_size"]), p["slope"], p["initial_distance"], p["max_distance"], p["cell_size"], p["base"],
                int(p["exponential"]))

    def _common(self, kw):
        pts = kw.pop("pts", self.pts.ctypes.data)
        return pts, kw.pop("n", 8), kw.pop("stride", 16), kw.pop("mem", 0)

    def operator(self, **kw):
        from pointcloudcomparator_amd import capi
        a = self._common(kw)
        r = capi.LIB.pcc_morphological_operator(None, *a, kw.pop("window", 1.0), kw.pop("op", capi.MORPH_OPEN), kw.pop("out", self.z.ctypes.data))
        assert not kw
        return r

    def filter(self, **kw):
        from pointcloudcomparator_amd import capi
        a, p = self._common(kw), self._pmf(kw)
        r = capi.LIB.pcc_progressive_morphological_filter(None, *a, *p, kw.pop("out", self.idx.ctypes.data),
                                                          kw.pop("n_ground", C.byref(self.ng)), kw.pop("sizes", self.sizes.ctypes.data),
                                                          kw.pop("max_passes", 64))
        assert not kw
        return r

    def segmentation(self, **kw):
        from pointcloudcomparator_amd import capi
        a, p = self._common(kw), self._pmf(kw)
        r = capi.LIB.pcc_ground_segmentation(None, *a, kw.pop("leaf", 0.01), *p, kw.pop("out", self.out.ctypes.data),
                                             kw.pop("out_stride", 16), kw.pop("n_filtered", C.byref(self.nv)),
                                             kw.pop("index", self.idx.ctypes.data), kw.pop("n_ground", C.byref(self.ng)),
                                             kw.pop("gpoints", self.out2.ctypes.data), kw.pop("opoints", self.out3.ctypes.data))
        assert not kw
        return r

    def untouched(self):
        return ((self.out == 7).all() and (self.out2 == 7).all() and (self.out3 == 7).all() and (self.z == 7).all() and
                (self.idx == 7).all() and (self.sizes == 7).all() and self.nv.value == 7 and self.ng.value == 7)


CLOUD_REFUSALS = [
    (dict(mem=2), -1, b"bad mem space"), (dict(pts=None), -1, b"null point pointer"), (dict(stride=8), -1, b"stride"),
    (dict(stride=14), -1, b"stride"), (dict(n=2 ** 31), -5, b"2^31"),
]
PMF_ARG_REFUSALS = [(kw, -1, m) for kw, m in PMF_REFUSALS] + [(dict(max_window_size=1000, base=1.0001), -6, b"more than 64 windows")]


@pytest.mark.parametrize("kw,status,message", CLOUD_REFUSALS + [
    (dict(out=None), -1, b"null output"), (dict(op=4), -1, b"bad morphological operator"), (dict(op=-1), -1, b"bad morphological operator"),
    (dict(window=0.0), -1, b"window"), (dict(window=-1.0), -1, b"window"), (dict(window=NAN), -1, b"window"), (dict(window=INF), -1, b"window"),
])
def test_operator_refused_before_the_handle(kw, status, message):
    from pointcloudcomparator_amd import capi
    call = Raw()
    assert call.operator(**kw) == status and call.untouched()
    assert message in capi.LIB.pcc_last_error() and b"null index" not in capi.LIB.pcc_last_error()


@pytest.mark.parametrize("kw,status,message", CLOUD_REFUSALS + PMF_ARG_REFUSALS + [
    (dict(out=None), -1, b"null output"), (dict(n_ground=None), -1, b"null output"),
])
def test_filter_refused_before_the_handle(kw, status, message):
    from pointcloudcomparator_amd import capi
    call = Raw()
    assert call.filter(**dict(kw)) == status and call.untouched()
    assert message in capi.LIB.pcc_last_error() and b"null index" not in capi.LIB.pcc_last_error()


@pytest.mark.parametrize("kw,status,message", CLOUD_REFUSALS + PMF_ARG_REFUSALS + [
    (dict(out=None), -1, b"null output"), (dict(out_stride=8), -1, b"bad output stride"), (dict(out_stride=18), -1, b"bad output stride"),
    (dict(leaf=0.0), -1, b"leaf size"), (dict(leaf=NAN), -1, b"leaf size"), (dict(n_filtered=None), -1, b"null output"),
    (dict(n_ground=None), -1, b"null output"),
])
def test_segmentation_refused_before_the_handle(kw, status, message):
    from pointcloudcomparator_amd import capi
    call = Raw()
    assert call.segmentation(**dict(kw)) == status and call.untouched()
    assert message in capi.LIB.pcc_last_error() and b"null index" not in capi.LIB.pcc_last_error()


def test_null_handle_is_refused_last():
    from pointcloudcomparator_amd import capi
    call = Raw()
    for op in (capi.MORPH_DILATE, capi.MORPH_ERODE, capi.MORPH_OPEN, capi.MORPH_CLOSE):
        assert call.operator(op=op) == -1 and capi.LIB.pcc_last_error() == b"null index"
    assert call.operator(n=0, pts=None, out=None) == -1 and capi.LIB.pcc_last_error() == b"null index"
    assert call.filter() == -1 and capi.LIB.pcc_last_error() == b"null index"
    assert call.filter(sizes=None, max_passes=0) == -1 and call.filter(n=0, pts=None, out=None) == -1
    assert call.filter(max_window_size=0) == -1 and call.filter(exponential=False) == -1
    assert call.segmentation() == -1 and capi.LIB.pcc_last_error() == b"null index"
    assert call.segmentation(index=None, gpoints=None, opoints=None) == -1 and call.segmentation(n=0, pts=None) == -1
    assert call.segmentation(stride=12, out_stride=12) == -1 and call.segmentation(stride=32, out_stride=32) == -1
    assert capi.LIB.pcc_last_error() == b"null index" and call.untouched()


def test_two_faults_resolve_in_the_documented_order():
    from pointcloudcomparator_amd import capi
    call, err = Raw(), capi.LIB.pcc_last_error
    assert call.operator(n=2 ** 31, window=0.0) == -5
    assert call.operator(out=None, op=9) == -1 and b"null output" in err()
    assert call.operator(op=9, window=0.0) == -1 and b"operator" in err()
    assert call.filter(stride=8, cell_size=0.0) == -1 and b"stride" in err()
    assert call.filter(n_ground=None, cell_size=0.0) == -1 and b"null output" in err()
    assert call.segmentation(leaf=0.0, cell_size=0.0) == -1 and b"leaf size" in err()
    assert call.segmentation(n_filtered=None, cell_size=0.0) == -1 and b"null output" in err()
    assert call.segmentation(out_stride=8, leaf=0.0) == -1 and b"bad output stride" in err()
    assert call.untouched()


def test_python_wrapper_argument_handling():
    from pointcloudcomparator_amd import capi
    ix = capi.Index.__new__(capi.Index)  # (no handle: the checks below come first)
    ix._h, ix.auto_sync = None, True
    pts = np.zeros((8, 4), np.float32)
    for call in (lambda p: ix.morphological_operator(p, 1.0, capi.MORPH_OPEN), ix.progressive_morphological_filter, ix.ground_segmentation):
        with pytest.raises(AssertionError):
            call(pts.astype(np.float64))
        with pytest.raises(AssertionError):
            call(np.zeros((8, 2), np.float32))
        with pytest.raises(capi.PccError) as e:  # all arguments good: the NULL handle
            call(pts)
        assert e.value.status == -1 and "null index" in str(e.value)
    with pytest.raises(capi.PccError) as e:
        ix.morphological_operator(pts, 0.0, capi.MORPH_ERODE)
    assert e.value.status == -1 and "window" in str(e.value)
    with pytest.raises(capi.PccError) as e:
        ix.progressive_morphological_filter(pts, base=1.0)
    assert e.value.status == -1 and "base" in str(e.value)
    with pytest.raises(capi.PccError) as e:
        ix.ground_segmentation(pts, leaf=-1.0)
    assert e.value.status == -1 and "leaf size" in str(e.value)
    ix._h = None  # (nothing for __del__ to destroy)


# ---- the restatement itself, and the plan header on the CPU -----------------------------------------------------------------
def test_restatement_edge_cases():
    """the scenes the GPU tests rely on do exercise what they are there for"""
    p = gu.lattice_points()
    B, _ = gu.box_matrix(p, 0.5)
    d = np.maximum(np.abs(p[:, None, 0] - p[None, :, 0]), np.abs(p[:, None, 1] - p[None, :, 1]))
    assert B.sum() == 850 and (d < 0.25).sum() == 108  # inclusive ends against strict ones on the 12 x 9 lattice
    g = gu.georeferenced()
    B, _ = gu.box_matrix(g, 0.7)
    S, _ = gu.box_matrix(g, 0.7, short_form=True)
    assert (B != S).sum() > 0  # the edges as written differ from |d| <= half at these coordinates
    assert (gu.morph(g, 0.7, "erode") != gu.morph(g, 0.7, "erode", short_form=True)).sum() > 0
    q = gu.terrain(200, 3)
    q[100, 0] = np.nan
    for op in ("erode", "dilate", "open", "close"):
        assert gu.morph(q, 0.5, op)[100] == q[100, 2]
    assert 100 not in gu.pmf(q, **gu.TERRAIN)[0]


def test_plan_header_on_the_cpu():
    exe = ROOT / "build" / "test_ground_plan"
    assert exe.exists(), "build/test_ground_plan: run `make hosttest`"
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
