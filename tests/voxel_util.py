"""The clouds of the exact voxel-grid tests, and pcc_voxel_grid through ctypes with any row widths and either memory space
(capi.Index.voxel_grid takes host arrays of one width).  Clouds and references are built once and handed out read-only."""
import ctypes as C
import functools

import numpy as np

from voxel_ref import voxel_grid_ref

FILL = 0xA5


def records(xyz, rng):
    """32-byte x, y, z, 1, rgb rows; the colour words random over all 32 bits (the top byte is set)"""
    rec = np.zeros((len(xyz), 8), np.float32)
    rec[:, :3] = xyz
    rec[:, 3] = 1.0
    rec.view(np.uint32)[:, 4] = rng.integers(0, 2 ** 32, len(xyz), dtype=np.uint64).astype(np.uint32)
    return rec


def _faces_xyz(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(-1024, 1024, (n, 3)).astype(np.float64) * 2.0 ** -10).astype(np.float32), rng


def _faces():
    xyz, rng = _faces_xyz(20000, 101)
    return records(xyz, rng)


def _far():
    rng = np.random.default_rng(102)
    xyz = np.array([1000.0, 1e5, -1e5]) + rng.integers(0, 256, (6000, 3)).astype(np.float64) * 2.0 ** -6
    assert (xyz.astype(np.float32).astype(np.float64) == xyz).all()
    return records(xyz.astype(np.float32), rng)


def _nonfinite():
    xyz, rng = _faces_xyz(5000, 103)
    rec = records(xyz, rng)
    rec[::97, 1] = np.nan
    rec[0, 0] = np.nan
    rec[-1, 2] = np.inf
    rec[2000:2064, 0] = -np.inf
    return rec


def _heavy(white):
    rng = np.random.default_rng(104)
    heavy = 0.5 + rng.integers(0, 64, (60000, 3)).astype(np.float64) * 2.0 ** -12
    scattered = rng.integers(-16, 16, (300, 3)).astype(np.float64) * 2.0 ** -3
    xyz = np.concatenate([heavy, scattered])[rng.permutation(60300)].astype(np.float32)
    rec = records(xyz, rng)
    if white:
        rec.view(np.uint32)[:, 4] = 0xFFFFFFFF
    return rec


def _one():
    return records(np.array([[0.3, -7.25, 1e3]], np.float32), np.random.default_rng(105))


def _one_voxel():
    rng = np.random.default_rng(106)
    return records((rng.integers(0, 512, (257, 3)).astype(np.float64) * 2.0 ** -10).astype(np.float32), rng)


def _all_nonfinite():
    rec = records(np.zeros((100, 3), np.float32), np.random.default_rng(107))
    rec[:, :3] = np.nan
    return rec


def _general(shift_y):
    rng = np.random.default_rng(108)
    xyz = (rng.random((20000, 3)) * 2 - 1).astype(np.float32)
    if shift_y:
        xyz[:, 1] += np.float32(1000.0)
    return records(xyz, rng)


# name -> (builder, leaf).  Every case but the two `general` ones is dyadic: its float64 sums are exact in any order.
CASES = {
    "faces-2^-4": (_faces, 2.0 ** -4),
    "faces-0.025": (_faces, 0.025),
    "far-0.25": (_far, 0.25),
    "far-0.025": (_far, 0.025),
    "non-finite": (_nonfinite, 2.0 ** -4),
    "heavy-white": (functools.partial(_heavy, True), 2.0 ** -4),
    "heavy-random": (functools.partial(_heavy, False), 2.0 ** -4),
    "one-point": (_one, 0.025),
    "one-voxel-257": (_one_voxel, 0.5),
    "all-non-finite": (_all_nonfinite, 0.025),
    "general": (functools.partial(_general, False), 0.1),
    "general-y+1000": (functools.partial(_general, True), 0.1),
}
DYADIC = [k for k in CASES if not k.startswith("general")]


@functools.lru_cache(maxsize=None)
def cloud(name):
    rec = CASES[name][0]()
    rec.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def reference(name, has_rgb=True):
    rows, counts = voxel_grid_ref(cloud(name), CASES[name][1], has_rgb)
    rows.setflags(write=False)
    counts.setflags(write=False)
    return rows, counts


def leaf_of(name):
    return CASES[name][1]


# ---- the call ---------------------------------------------------------------------------------------------------------------
def input_bytes(rec, stride, has_rgb, whole_rows):
    """rec's rows `stride` bytes apart: x, y, z [, 1 [, rgb [, the rest of the 32-byte record]]].  whole_rows False: the buffer
    ends with the last byte the call reads of the last row (z, or the colour word), as a strided view of a larger table does"""
    n = len(rec)
    assert stride in (12, 16, 20, 32) and (not has_rgb or stride >= 20)
    src = np.ascontiguousarray(rec).view(np.uint8).reshape(n, 32)
    buf = np.zeros((n, stride), np.uint8)
    buf[:, :] = src[:, :stride]
    flat = buf.reshape(-1)
    if not whole_rows:
        flat = flat[:(n - 1) * stride + (20 if has_rgb else 12)].copy()
    return flat


def call(handle, rec, leaf, has_rgb=True, in_stride=32, out_stride=32, device=False):
    """pcc_voxel_grid on `handle` (a capi.Index).  Returns (status, out_n, out): out the (len(rec) * out_stride) output bytes,
    filled with FILL before the call."""
    from pointcloudcomparator_amd import capi
    n = len(rec)
    cnt = C.c_size_t(12345)
    if device:
        import torch
        src = torch.from_numpy(input_bytes(rec, in_stride, has_rgb, whole_rows=True)).cuda()
        out = torch.full((max(n * out_stride, 1),), FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        st = capi.LIB.pcc_voxel_grid(handle._h, src.data_ptr(), n, in_stride, capi.MEM_DEVICE, C.c_float(leaf), int(has_rgb), out.data_ptr(),
                                     out_stride, C.byref(cnt))
        handle.sync()
        return st, cnt.value, out.cpu().numpy()[:n * out_stride]
    src = input_bytes(rec, in_stride, has_rgb, whole_rows=False)
    out = np.full(n * out_stride, FILL, np.uint8)
    st = capi.LIB.pcc_voxel_grid(handle._h, src.ctypes.data, n, in_stride, capi.MEM_HOST, C.c_float(leaf), int(has_rgb), out.ctypes.data, out_stride,
                                 C.byref(cnt))
    return st, cnt.value, out


def last_error():
    from pointcloudcomparator_amd import capi
    return capi.LIB.pcc_last_error()


def split_rows(out, out_n, out_stride, has_rgb):
    """(xyz bits (nv, 3) uint32, w bits or None, colour words or None, padding bytes inside the written rows, the bytes behind them)"""
    rows = out[:out_n * out_stride].reshape(out_n, out_stride)
    xyz = np.ascontiguousarray(rows[:, :12]).view(np.uint32)
    w = np.ascontiguousarray(rows[:, 12:16]).view(np.uint32)[:, 0] if out_stride >= 16 else None
    rgb = np.ascontiguousarray(rows[:, 16:20]).view(np.uint32)[:, 0] if has_rgb else None
    defined = 20 if has_rgb else min(out_stride, 16)
    return xyz, w, rgb, rows[:, defined:], out[out_n * out_stride:]


def assert_equals_reference(result, ref_rows, out_stride, has_rgb, device, what=""):
    """status PCC_OK, the reference's count, every field the reference's bits, the rows behind *out_n untouched, and the bytes of
    a written row the call does not define: the caller's on the device route, zeros on the host route"""
    st, out_n, out = result
    assert st == 0, (what, st, last_error())
    assert out_n == len(ref_rows), (what, out_n, len(ref_rows))
    xyz, w, rgb, pad, tail = split_rows(out, out_n, out_stride, has_rgb)
    want = np.ascontiguousarray(ref_rows[:, :3]).view(np.uint32)
    differ = np.flatnonzero((xyz != want).any(axis=1))
    assert len(differ) == 0, (what, "rows whose x, y, z differ", len(differ), differ[:5], xyz[differ[:5]], want[differ[:5]])
    if w is not None:
        assert (w == 0x3F800000).all(), what
    if has_rgb:
        assert (rgb == np.ascontiguousarray(ref_rows[:, 4]).view(np.uint32)).all(), what
    assert (tail == FILL).all(), (what, "rows from *out_n on were written")
    assert (pad == (FILL if device else 0)).all(), (what, "padding bytes")
