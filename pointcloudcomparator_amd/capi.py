"""ctypes binding of the libpcc_nn C-ABI (include/pcc_nn.h).

Thin by design: every method maps 1:1 onto one exported function; numpy arrays
are passed as host pointers, torch CUDA tensors as device pointers.  No search
is ever computed in Python -- a missing library is a hard error.
"""
from __future__ import annotations

import collections
import ctypes as C
import os
from pathlib import Path

import numpy as np

MEM_HOST, MEM_DEVICE = 0, 1
TIES_LOWEST_INDEX, TIES_FLANN = 0, 1
ENGINE_AUTO, ENGINE_BRUTE, ENGINE_GRID = 0, 1, 2
KNN_MAX_K = 65536
# enum pcc_option
(OPT_GRID_PPC, OPT_GRID_TRIM, OPT_FAR_MODE, OPT_ICP_WARM, OPT_ICP_DEVICE_LOOP, OPT_EC_CELLS, OPT_SORT_MP_MIN,
 OPT_SORT_MP_MIN_Q, OPT_NN1_KERNEL, OPT_FLANN_SPLIT, OPT_NN1_DENSE_MIN, OPT_KNN_KERNEL, OPT_KNN_CACHE_K, OPT_NN1_OPEN_FLAT, OPT_SORT_STAGE1,
 OPT_ICP_SORTED, OPT_OVERLAP_PREP, OPT_GRID_AXES, OPT_XCD_RUN, OPT_FUSE_PARAMS, OPT_HOST_PIPE, OPT_SCAN_CHAINED, OPT_KNN_RUN,
 OPT_RIFT_LAYOUT, OPT_SIFT_LAYOUT, OPT_RIFT_BATCH_BRUTE_MAX, OPT_SIFT_BATCH_BRUTE_MAX, OPT_RGB_BATCH_BRUTE_MAX, OPT_FPFH_LAYOUT,
 OPT_FPFH_BATCH_BRUTE_MAX, OPT_VFH_BATCH_BRUTE_MAX) = range(1, 32)

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("PCC_LIB", _HERE / "lib" / "libpcc_nn.so"))

# every symbol include/pcc_nn.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = [
    "pcc_version", "pcc_last_error", "pcc_device_count",
    "pcc_index_create", "pcc_index_destroy", "pcc_index_size", "pcc_index_set_stream",
    "pcc_index_sync", "pcc_index_engine", "pcc_index_set_engine",
    "pcc_nn1", "pcc_knn", "pcc_radius_count", "pcc_radius_fill", "pcc_radius_count_max", "pcc_radius_fill_max",
    "pcc_euclidean_clusters", "pcc_sor", "pcc_icp_step", "pcc_transform", "pcc_icp_align",
    "pcc_match_knn", "pcc_match_knn_batch", "pcc_match_knn_batch_dims", "pcc_match_fpfh_batch", "pcc_index_stats", "pcc_index_set_input", "pcc_index_enable_timing",
    "pcc_index_timing", "pcc_first_within", "pcc_voxel_grid",
    "pcc_normals", "pcc_region_growing", "pcc_region_growing_rgb", "pcc_region_growing_rgb_batch", "pcc_sac_plane", "pcc_plane_removal", "pcc_extract_clusters", "pcc_region_growing_segmentation", "pcc_euclidean_cluster_segmentation", "pcc_rigid_from_sums",
    "pcc_rigid_from_sums_about", "pcc_icp_step_about",
    "pcc_normals_radius", "pcc_rift_descriptors", "pcc_rift_descriptors_batch", "pcc_sift_keypoints", "pcc_sift_keypoints_batch", "pcc_cluster_descriptors", "pcc_cluster_matching", "pcc_match_colour_elements", "pcc_index_wait_stream", "pcc_stream_wait_index", "pcc_index_clone_to_device", "pcc_index_set_tie_order",
    "pcc_index_set_option", "pcc_index_get_option", "pcc_index_clone_to_devices", "pcc_counts_pairs", "pcc_index_sor_on_device",
    "pcc_debug_fail_alloc", "pcc_debug_live_buffers",
    "pcc_comm_unique_id", "pcc_comm_create_rank", "pcc_comm_create_local", "pcc_comm_destroy", "pcc_comm_info",
    "pcc_index_create_broadcast", "pcc_icp_align_sharded", "pcc_sor_partial", "pcc_sor_threshold", "pcc_sor_sharded",
    "pcc_pmf_windows", "pcc_morphological_operator", "pcc_progressive_morphological_filter", "pcc_ground_segmentation",
    "pcc_change_detection", "pcc_fpfh_descriptors", "pcc_shot_descriptors", "pcc_fpfh_descriptors_batch", "pcc_vfh_descriptor", "pcc_match_vfh", "pcc_vfh_descriptors_batch",
]
# enum pcc_morph_op
MORPH_DILATE, MORPH_ERODE, MORPH_OPEN, MORPH_CLOSE = range(4)
PMF_MAX_WINDOWS = 64


class PccError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"libpcc_nn status {status}: {msg}")
        self.status = status


def _preload_hip_runtime() -> None:
    """One HIP runtime per process.  torch wheels ship their own libamdhip64.so (SONAME
    libamdhip64.so.7, same as /opt/rocm's).  If libpcc_nn pulled in /opt/rocm's copy first and
    torch were imported later, two runtimes would fight over the device ("No HIP GPUs are
    available").  Loading torch's copy first (without importing torch) makes both resolve to it."""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    cand = Path(list(spec.submodule_search_locations)[0]) / "lib" / "libamdhip64.so"
    if cand.exists():
        C.CDLL(str(cand), mode=C.RTLD_GLOBAL)


def _load() -> C.CDLL:
    _preload_hip_runtime()
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} not found: build it with `make lib` (or __graft_entry__.build()). "
            "pointcloudcomparator_amd has no CPU fallback.")
    lib = C.CDLL(str(LIB_PATH))
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
    lib.pcc_last_error.restype = C.c_char_p
    lib.pcc_index_create.argtypes = [vp, sz, sz, i32, i32, i32, i32, C.POINTER(vp)]
    lib.pcc_index_destroy.argtypes = [vp]
    lib.pcc_index_set_input.argtypes = [vp, vp, sz, sz, i32, i32]
    lib.pcc_index_enable_timing.argtypes = [vp, i32]
    lib.pcc_index_timing.argtypes = [vp, C.POINTER(C.c_float)]
    lib.pcc_index_size.argtypes = [vp, C.POINTER(sz)]
    lib.pcc_index_set_stream.argtypes = [vp, vp]
    lib.pcc_index_sync.argtypes = [vp]
    lib.pcc_index_set_tie_order.argtypes = [vp, i32]
    lib.pcc_index_clone_to_device.argtypes = [vp, i32, C.POINTER(vp)]
    lib.pcc_index_clone_to_devices.argtypes = [vp, C.POINTER(i32), i32, C.POINTER(vp)]
    lib.pcc_index_set_option.argtypes = [vp, i32, C.c_double]
    lib.pcc_index_get_option.argtypes = [vp, i32, C.POINTER(C.c_double)]
    lib.pcc_index_wait_stream.argtypes = [vp, vp]
    lib.pcc_stream_wait_index.argtypes = [vp, vp]
    lib.pcc_index_engine.argtypes = [vp, C.POINTER(i32)]
    lib.pcc_index_set_engine.argtypes = [vp, i32]
    lib.pcc_index_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.pcc_device_count.argtypes = [C.POINTER(i32)]
    lib.pcc_debug_live_buffers.argtypes = [C.POINTER(C.c_uint64)]
    lib.pcc_nn1.argtypes = [vp, vp, sz, sz, i32, vp, vp]
    lib.pcc_knn.argtypes = [vp, vp, sz, sz, i32, i32, vp, vp]
    lib.pcc_radius_count.argtypes = [vp, vp, sz, sz, i32, C.c_double, vp]
    lib.pcc_first_within.argtypes = [vp, vp, sz, sz, i32, C.c_double, vp]
    lib.pcc_rigid_from_sums.argtypes = [vp, vp]
    lib.pcc_rigid_from_sums_about.argtypes = [vp, vp, vp]
    lib.pcc_icp_step_about.argtypes = [vp, vp, sz, sz, i32, vp, vp, vp, C.POINTER(C.c_double)]
    lib.pcc_sac_plane.argtypes = [vp, vp, sz, sz, i32, i32, C.c_double, C.c_double, i32, vp, C.POINTER(sz), vp, vp]
    lib.pcc_plane_removal.argtypes = [vp, vp, sz, sz, i32, C.c_double, i32, C.c_double, C.c_double, i32, sz, vp, vp, vp, C.POINTER(sz),
                                      C.POINTER(i32), vp, vp, C.POINTER(sz), vp, sz, sz]
    lib.pcc_extract_clusters.argtypes = [vp, vp, sz, sz, sz, vp, i32, i32, vp, sz, vp, vp]
    lib.pcc_region_growing_segmentation.argtypes = [vp, vp, sz, sz, i32, C.c_float, i32, i32, i32, C.c_float, C.c_float, C.c_uint32,
                                                    C.c_uint32, vp, sz, C.POINTER(sz), vp, vp, sz, C.POINTER(i32), vp, vp, vp]
    lib.pcc_euclidean_cluster_segmentation.argtypes = [vp, vp, sz, sz, i32, C.c_float, i32, C.c_double, i32, C.c_double, C.c_double, i32, sz,
                                                       vp, vp, vp, C.POINTER(sz), C.POINTER(i32), C.c_double, C.c_uint32, C.c_uint32, vp,
                                                       sz, C.POINTER(sz), C.POINTER(sz), vp, sz, C.POINTER(i32), vp, vp, vp]
    lib.pcc_normals.argtypes = [vp, i32, vp, i32, vp]
    lib.pcc_normals_radius.argtypes = [vp, C.c_double, vp, i32, vp]
    lib.pcc_rift_descriptors.argtypes = [vp, vp, sz, i32, C.c_double, C.c_double, C.c_double, i32, i32, vp, vp, C.POINTER(sz)]
    lib.pcc_fpfh_descriptors.argtypes = [vp, i32, C.c_double, C.c_double, i32, i32, i32, vp, vp, C.POINTER(sz)]
    lib.pcc_shot_descriptors.argtypes = [vp, i32, C.c_double, C.c_double, vp, vp, vp, C.POINTER(sz)]
    lib.pcc_vfh_descriptor.argtypes = [vp, i32, C.c_double, vp, C.POINTER(sz)]
    lib.pcc_match_vfh.argtypes = [vp, vp, sz, vp, sz, i32, vp]
    lib.pcc_vfh_descriptors_batch.argtypes = [vp, vp, sz, vp, sz, i32, C.c_double, vp, vp]
    lib.pcc_fpfh_descriptors_batch.argtypes = [vp, vp, sz, vp, sz, i32, C.c_double, C.c_double, i32, i32, i32, vp, vp, vp]
    lib.pcc_rift_descriptors_batch.argtypes = [vp, sz, vp, vp, sz, vp, sz, i32, C.c_double, C.c_double, C.c_double, i32, i32, vp, vp, vp]
    lib.pcc_sift_keypoints.argtypes = [vp, vp, sz, sz, vp, sz, i32, C.c_float, i32, i32, C.c_float, vp, sz, C.POINTER(sz)]
    lib.pcc_sift_keypoints_batch.argtypes = [vp, sz, vp, vp, sz, vp, sz, i32, C.c_float, i32, i32, C.c_float, C.c_double, vp, vp, sz, vp]
    lib.pcc_cluster_descriptors.argtypes = [vp, vp, sz, vp, sz, vp, sz, i32, sz, C.c_float, i32, i32, C.c_float, C.c_double, C.c_double, C.c_double,
                                            C.c_double, i32, i32, vp, vp, sz, vp, vp, vp]
    lib.pcc_cluster_matching.argtypes = [vp, vp, vp, sz, vp, vp, sz, sz, i32, i32, vp, vp, vp, vp, C.c_float, vp, vp, vp, vp]
    lib.pcc_match_colour_elements.argtypes = [vp, vp, vp, vp, sz, vp, vp, vp, sz, sz, sz, i32, vp, sz, C.c_float, C.c_float, C.c_float, C.c_uint32,
                                              C.c_uint32, C.c_uint, C.c_uint, vp]
    lib.pcc_region_growing.argtypes = [vp, vp, i32, i32, C.c_float, C.c_float, C.c_uint32, C.c_uint32, vp, vp]
    lib.pcc_region_growing_rgb.argtypes = [vp, vp, sz, i32, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_uint, C.c_uint, vp,
                                           C.POINTER(C.c_int32)]
    lib.pcc_region_growing_rgb_batch.argtypes = [vp, sz, vp, vp, sz, vp, sz, i32, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_uint,
                                                 C.c_uint, vp, vp]
    lib.pcc_voxel_grid.argtypes = [vp, vp, sz, sz, i32, C.c_float, i32, vp, sz, C.POINTER(sz)]
    lib.pcc_radius_fill.argtypes = [vp, vp, sz, sz, i32, C.c_double, i32, vp, vp, vp]
    lib.pcc_radius_count_max.argtypes = [vp, vp, sz, sz, i32, C.c_double, C.c_uint, vp]
    lib.pcc_radius_fill_max.argtypes = [vp, vp, sz, sz, i32, C.c_double, i32, C.c_uint, vp, vp, vp]
    lib.pcc_euclidean_clusters.argtypes = [vp, C.c_double, C.c_uint32, C.c_uint32, i32, vp,
                                           C.POINTER(C.c_int32), vp, i32]
    lib.pcc_sor.argtypes = [vp, i32, C.c_double, i32, vp, vp, C.POINTER(C.c_double), C.POINTER(sz)]
    lib.pcc_icp_step.argtypes = [vp, vp, sz, sz, i32, vp, vp, C.POINTER(C.c_double)]
    lib.pcc_transform.argtypes = [vp, C.POINTER(C.c_float), vp, sz, sz, vp, sz, i32]
    lib.pcc_icp_align.argtypes = [vp, vp, sz, sz, i32, i32, i32, C.POINTER(C.c_float),
                                  C.POINTER(C.c_double), C.POINTER(i32), C.POINTER(i32)]
    lib.pcc_match_knn.argtypes = [vp, vp, sz, sz, i32, C.c_float, vp, C.POINTER(C.c_int32)]
    lib.pcc_match_knn_batch.argtypes = [vp, sz, vp, vp, vp, vp, sz, i32, C.c_float, vp, vp]
    lib.pcc_match_knn_batch_dims.argtypes = [vp, sz, vp, vp, vp, vp, sz, i32, i32, C.c_float, vp, vp, vp]
    lib.pcc_match_fpfh_batch.argtypes = [vp, sz, vp, vp, vp, vp, sz, i32, C.c_float, vp, vp, vp]
    lib.pcc_comm_unique_id.argtypes = [vp, sz]
    lib.pcc_comm_create_rank.argtypes = [vp, sz, i32, i32, i32, C.POINTER(vp)]
    lib.pcc_comm_create_local.argtypes = [C.POINTER(i32), i32, C.POINTER(vp)]
    lib.pcc_comm_destroy.argtypes = [vp]
    lib.pcc_comm_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    lib.pcc_index_create_broadcast.argtypes = [vp, i32, vp, sz, sz, i32, i32, C.POINTER(vp), C.POINTER(sz)]
    lib.pcc_icp_align_sharded.argtypes = [vp, vp, vp, sz, sz, i32, i32, i32, C.POINTER(C.c_float), C.POINTER(C.c_double),
                                          C.POINTER(i32), C.POINTER(i32)]
    lib.pcc_sor_partial.argtypes = [vp, sz, sz, i32, i32, vp, C.POINTER(C.c_double)]
    lib.pcc_sor_threshold.argtypes = [C.POINTER(C.c_double), C.c_uint64, i32, C.c_double, C.POINTER(C.c_double), C.POINTER(i32)]
    lib.pcc_sor_sharded.argtypes = [vp, vp, sz, sz, i32, C.c_double, i32, vp, vp, C.POINTER(C.c_double), C.POINTER(sz)]
    f32 = C.c_float
    lib.pcc_pmf_windows.argtypes = [i32, f32, f32, f32, f32, f32, i32, sz, vp, vp, C.POINTER(sz)]
    lib.pcc_morphological_operator.argtypes = [vp, vp, sz, sz, i32, f32, i32, vp]
    lib.pcc_progressive_morphological_filter.argtypes = [vp, vp, sz, sz, i32, i32, f32, f32, f32, f32, f32, i32, vp, C.POINTER(sz), vp, sz]
    lib.pcc_ground_segmentation.argtypes = [vp, vp, sz, sz, i32, f32, i32, f32, f32, f32, f32, f32, i32, vp, sz, C.POINTER(sz), vp,
                                            C.POINTER(sz), vp, vp]
    lib.pcc_change_detection.argtypes = [vp, vp, sz, sz, vp, sz, sz, i32, C.c_double, i32, vp, vp, C.POINTER(sz)]
    for name in SYMBOLS:
        fn = getattr(lib, name)  # raises AttributeError if the library lacks a declared symbol
        if name != "pcc_last_error":
            fn.restype = C.c_int
    return lib


LIB = _load()


def _check(status: int) -> None:
    if status != 0:
        raise PccError(status, (LIB.pcc_last_error() or b"").decode())


def device_count() -> int:
    """number of HIP devices; 0 when the runtime reports none (no exception)."""
    n = C.c_int(0)
    st = LIB.pcc_device_count(C.byref(n))
    return n.value if st == 0 else 0


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _points(x):
    """(pointer, n, stride_bytes, mem) of an (n, >=3) float32 numpy array or torch tensor."""
    if _is_torch(x):
        assert x.dtype.is_floating_point and x.element_size() == 4 and x.dim() == 2 and x.shape[1] >= 3
        assert x.shape[0] == 0 or x.stride(1) == 1  # (an empty tensor made from an empty array has no strides to speak of)
        mem = MEM_DEVICE if x.is_cuda else MEM_HOST
        return x.data_ptr(), x.shape[0], x.stride(0) * 4 if x.shape[0] > 1 else x.shape[1] * 4, mem
    a = x
    assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.ndim == 2 and a.shape[1] >= 3
    assert a.shape[0] == 0 or a.strides[1] == 4
    stride = a.strides[0] if a.shape[0] > 1 else a.shape[1] * 4
    return a.ctypes.data, a.shape[0], stride, MEM_HOST


def _records(a, dim):
    """(pointer, n, stride_bytes, mem) of an (n, >= dim) float32 numpy array of descriptor records (host memory)."""
    assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.ndim == 2 and a.shape[1] >= min(max(int(dim), 1), 32)
    assert a.shape[0] == 0 or a.strides[1] == 4
    stride = a.strides[0] if a.shape[0] > 1 else a.shape[1] * 4
    return a.ctypes.data, a.shape[0], stride, MEM_HOST


def _out(like, shape, dtype):
    """allocate an output in the memory space of `like`."""
    if _is_torch(like) and like.is_cuda:
        import torch
        tdt = {np.int32: torch.int32, np.float32: torch.float32, np.uint8: torch.uint8,
               np.int64: torch.int64, np.float64: torch.float64}[dtype]
        t = torch.empty(shape, dtype=tdt, device=like.device)
        return t, t.data_ptr()
    a = np.empty(shape, dtype=dtype)
    return a, a.ctypes.data


def _colour_words(rgb):
    """(keep-alive, pointer, stride_bytes, mem) of one colour per point, numpy array or torch tensor:
    (n, 3) uint8 r, g, b;  (n,) uint32 / int32 packed colour words (bytes b, g, r, a from the low byte);  or the (n, >= 5)
    float32 records of pcl::PointXYZRGB (colour word in column 4), read in place with their stride."""
    torch_in = _is_torch(rgb)
    if torch_in:
        import torch
    if rgb.ndim == 2 and rgb.shape[1] == 3 and rgb.dtype == (torch.uint8 if torch_in else np.uint8):
        c = rgb.to(torch.int32) if torch_in else rgb.astype(np.uint32)
        words = c[:, 2] | (c[:, 1] << 8) | (c[:, 0] << 16)
        words = words.contiguous() if torch_in else np.ascontiguousarray(words)
        ptr, stride = (words.data_ptr() if torch_in else words.ctypes.data), 4
    elif rgb.ndim == 1:
        words = rgb.contiguous() if torch_in else np.ascontiguousarray(rgb)
        assert (words.element_size() if torch_in else words.itemsize) == 4, "packed colour words are 32-bit"
        ptr, stride = (words.data_ptr() if torch_in else words.ctypes.data), 4
    else:
        words = rgb  # pcl::PointXYZRGB records: the colour word sits 16 bytes into each
        base, _, stride, _ = _points(rgb)
        assert rgb.shape[1] >= 5, "PointXYZRGB records have their colour word in column 4"
        ptr = base + 16
    mem = MEM_DEVICE if torch_in and words.is_cuda else MEM_HOST
    return words, ptr, stride, mem


# the host clouds of a *_batch call as the C-ABI takes them; `keep` holds the staged arrays the pointers point into
_CloudBatch = collections.namedtuple("_CloudBatch", "n pts counts stride rgb rgb_stride keep")


def _cloud_batch(clouds, rgbs, fn_name):
    """_CloudBatch of clouds / rgbs (None: the clouds are pcl::PointXYZRGB records, their colour words read in place); counts is
    the c_size_t array of the sizes.  The result must stay referenced for the length of the call."""
    clouds = list(clouds)
    rgbs = list(clouds if rgbs is None else rgbs)
    n = len(clouds)
    assert len(rgbs) == n, "one colour array per cloud"
    args = [_points(a) for a in clouds]
    cols = [_colour_words(r) if len(r) else (None, None, None, MEM_HOST) for r in rgbs]
    assert all(len(r) == a[1] for r, a in zip(rgbs, args)), "one colour per point"
    assert all(a[3] == MEM_HOST for a in args) and all(c[3] == MEM_HOST for c in cols), f"{fn_name} takes host arrays"
    strides = {a[2] for a in args if a[1] > 1}
    cstrides = {c[2] for c, a in zip(cols, args) if a[1] > 1}
    assert len(strides) <= 1 and len(cstrides) <= 1, "every cloud of a batch must have the same row stride, and so every colour array"
    single = [(a[2], c[2]) for c, a in zip(cols, args) if a[1] == 1]  # (one row: any stride the others use will do)
    stride = strides.pop() if strides else (single[0][0] if single else 12)
    cstride = cstrides.pop() if cstrides else (single[0][1] if single else 4)
    vps, szs = (C.c_void_p * max(n, 1)), (C.c_size_t * max(n, 1))
    pp = vps(*[a[0] if a[1] else None for a in args])
    cp = vps(*[c[1] if a[1] else None for c, a in zip(cols, args)])
    return _CloudBatch(n, pp, szs(*[a[1] for a in args]), stride, cp, cstride, (clouds, cols))


def rigid_from_sums(sums, center=None):
    """4x4 float32 rigid transform from the 17 ICP sums (pcc_rigid_from_sums[_about]; host arithmetic, no handle).
    center: the point the sums were taken about (Index.icp_step(..., center=...)); None = the origin."""
    sm = np.ascontiguousarray(sums, dtype=np.float64)
    assert sm.shape == (17,)
    T = np.zeros(16, dtype=np.float32)
    if center is None:
        _check(LIB.pcc_rigid_from_sums(sm.ctypes.data, T.ctypes.data))
    else:
        cc = np.ascontiguousarray(center, dtype=np.float64)
        assert cc.shape == (3,)
        _check(LIB.pcc_rigid_from_sums_about(sm.ctypes.data, cc.ctypes.data, T.ctypes.data))
    return T.reshape(4, 4)


def pmf_windows(max_window_size: int = 20, slope: float = 1.0, initial_distance: float = 0.5, max_distance: float = 3.0,
                cell_size: float = 1.0, base: float = 2.0, exponential: bool = True, capacity: int = PMF_MAX_WINDOWS):
    """pcc_pmf_windows: the window table of pcl::ProgressiveMorphologicalFilter (host arithmetic, no handle); the defaults are the
    reference's parameters (src/segmentation.cpp:330-387).  Returns (windows, thresholds), float32 arrays.  A table longer than
    `capacity` or than PMF_MAX_WINDOWS raises PccError (PCC_ERR_OVERFLOW) whose `n_windows` is the length needed."""
    capacity = int(capacity)
    assert capacity >= 0
    w = np.zeros(max(capacity, 1), dtype=np.float32)
    h = np.zeros(max(capacity, 1), dtype=np.float32)
    nw = C.c_size_t(0)
    status = LIB.pcc_pmf_windows(int(max_window_size), float(slope), float(initial_distance), float(max_distance), float(cell_size),
                                 float(base), int(bool(exponential)), capacity, w.ctypes.data, h.ctypes.data, C.byref(nw))
    if status != 0:
        err = PccError(status, (LIB.pcc_last_error() or b"").decode())
        err.n_windows = nw.value
        raise err
    return w[:nw.value], h[:nw.value]


COMM_ID_BYTES = 128


def comm_unique_id() -> bytes:
    """the id rank 0 makes and hands to the other ranks (pcc_comm_unique_id)"""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(LIB.pcc_comm_unique_id(buf, COMM_ID_BYTES))
    return buf.raw


class Comm:
    """one rank of an RCCL communicator (pcc_comm): one per (process, GPU)"""

    def __init__(self, handle):
        self._c = handle

    @classmethod
    def from_id(cls, uid: bytes, world: int, rank: int, device: int):
        h = C.c_void_p()
        _check(LIB.pcc_comm_create_rank(uid, len(uid), world, rank, device, C.byref(h)))
        return cls(h)

    @classmethod
    def local(cls, devices):
        """communicators for several GPUs driven by this process: [rank 0 on devices[0], ...]"""
        arr = (C.c_int * len(devices))(*devices)
        hs = (C.c_void_p * len(devices))()
        _check(LIB.pcc_comm_create_local(arr, len(devices), hs))
        return [cls(C.c_void_p(h)) for h in hs]

    def info(self):
        r, w, d = C.c_int(0), C.c_int(0), C.c_int(0)
        _check(LIB.pcc_comm_info(self._c, C.byref(r), C.byref(w), C.byref(d)))
        return r.value, w.value, d.value

    def close(self):
        if self._c:
            LIB.pcc_comm_destroy(self._c)
            self._c = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def sor_threshold(sums, n_valid: int, mean_k: int = 50, stddev_mult: float = 1.5):
    """PCL's threshold from the combined (+, +, min, min) sums of all shards: (threshold, exact)"""
    sm = (C.c_double * 4)(*[float(v) for v in sums])
    thr, ex = C.c_double(0), C.c_int(0)
    _check(LIB.pcc_sor_threshold(sm, int(n_valid), mean_k, float(stddev_mult), C.byref(thr), C.byref(ex)))
    return thr.value, bool(ex.value)


class Index:
    """Owner of one pcc_index handle (the role pcl::KdTreeFLANN plays in the reference).

    auto_sync (default on): every call on torch CUDA tensors is bracketed with pcc_index_wait_stream / pcc_stream_wait_index
    against torch's current stream, so `ix.nn1(x * s)` reads finished data and `idx.cpu()` sees the result.  The bracket AFTER
    set_input makes torch's stream wait for the whole build, and the next call's bracket makes the library wait for torch's
    stream again: with auto_sync on, the query staging beside the build (PCC_OPT_OVERLAP_PREP) therefore hides nothing -- correct,
    only serial.  Callers that time or pipeline (bench.py) pass auto_sync=False and order the streams themselves (sync(),
    wait_stream(), stream_wait())."""

    _ties = TIES_LOWEST_INDEX  # what set_tie_order last set (a new handle starts with the lowest index)

    @classmethod
    def broadcast(cls, comm: "Comm", root: int, points=None, engine: int = ENGINE_AUTO, auto_sync: bool = True):
        """the reference cloud of rank `root` indexed on every rank of `comm` (pcc_index_create_broadcast; collective).
        points: read on the root only."""
        ptr, n, stride, mem = _points(points) if points is not None else (None, 0, 12, MEM_HOST)
        if points is not None and _is_torch(points) and points.is_cuda:
            import torch
            torch.cuda.current_stream(points.device).synchronize()
        h = C.c_void_p()
        n_all = C.c_size_t(0)
        _check(LIB.pcc_index_create_broadcast(comm._c, root, ptr, n, stride, mem, engine, C.byref(h), C.byref(n_all)))
        self = cls.__new__(cls)
        self._h = h
        self.auto_sync = auto_sync
        self.n_original = n_all.value
        return self

    def __init__(self, points, engine: int = ENGINE_AUTO, device: int = 0, auto_sync: bool = True):
        """auto_sync: calls that take torch CUDA tensors are ordered against torch's current stream on both
        sides (inputs produced by torch are complete before the library reads them; torch work issued after the
        call sees the outputs) with pcc_index_wait_stream / pcc_stream_wait_index -- two event records per call,
        no host wait.  A caller that brackets its calls with sync() itself (bench.py's timed region) turns it off."""
        ptr, n, stride, mem = _points(points)
        if _is_torch(points) and points.is_cuda:
            device = points.device.index or 0
            import torch
            torch.cuda.current_stream(points.device).synchronize()  # create is synchronous anyway
        h = C.c_void_p()
        _check(LIB.pcc_index_create(ptr, n, stride, 3, mem, device, engine, C.byref(h)))
        self._h = h
        self.n_original = n
        self.auto_sync = auto_sync
        self._cuda = points.device if _is_torch(points) and points.is_cuda else None  # results without an input array follow the cloud's memory space

    def _torch_stream(self, *tensors):
        """hipStream_t of torch's current stream on the device of the first CUDA tensor argument (None: no
        device tensor involved, or auto_sync off)."""
        if not self.auto_sync:
            return None
        for t in tensors:
            if t is not None and _is_torch(t) and t.is_cuda:
                import torch
                return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
        return None

    def _before(self, *tensors):
        st = self._torch_stream(*tensors)
        if st is not None:
            _check(LIB.pcc_index_wait_stream(self._h, st))
        return st

    def _after(self, st):
        if st is not None:
            _check(LIB.pcc_stream_wait_index(self._h, st))

    def clone_to_device(self, device: int) -> "Index":
        """a second handle over the same cloud on `device` (packed cloud copied device to device, index rebuilt there)"""
        h = C.c_void_p()
        _check(LIB.pcc_index_clone_to_device(self._h, device, C.byref(h)))
        other = Index.__new__(Index)
        other._h, other.n_original, other.auto_sync = h, self.n_original, self.auto_sync
        return other

    def clone_to_devices(self, devices):
        """one more handle over the same cloud per entry of `devices`: all peer copies in flight together, then the builds"""
        n = len(devices)
        arr = (C.c_int * n)(*devices)
        hs = (C.c_void_p * n)()
        _check(LIB.pcc_index_clone_to_devices(self._h, arr, n, hs))
        res = []
        for k in range(n):
            other = Index.__new__(Index)
            other._h, other.n_original, other.auto_sync = C.c_void_p(hs[k]), self.n_original, self.auto_sync
            res.append(other)
        return res

    def set_input(self, points):
        """pcl::KdTreeFLANN::setInputCloud on an existing object: rebuild over a new cloud,
        reusing the device allocations."""
        ptr, n, stride, mem = _points(points)
        st = self._before(points)
        _check(LIB.pcc_index_set_input(self._h, ptr, n, stride, 3, mem))
        # the pack kernel reads the caller's tensor on the library's stream after this returns: torch work issued
        # from here on (an overwrite, the allocator reusing the block) waits for it
        self._after(st)
        self.n_original = n
        self._cuda = points.device if _is_torch(points) and points.is_cuda else None

    def set_option(self, option: int, value: float):
        """pcc_index_set_option (OPT_*): implementation choices of this handle; no result bit depends on them"""
        _check(LIB.pcc_index_set_option(self._h, option, float(value)))

    def get_option(self, option: int) -> float:
        v = C.c_double(0)
        _check(LIB.pcc_index_get_option(self._h, option, C.byref(v)))
        return v.value

    def enable_timing(self, level=2):
        """0/False off, 1 main kernel only (cheap enough for a timed region), 2/True full breakdown"""
        level = 2 if level is True else int(level)
        _check(LIB.pcc_index_enable_timing(self._h, level))

    def timing(self):
        """ms of the instrumented kernels of the last call (see pcc_index_timing)."""
        t = (C.c_float * 8)()
        _check(LIB.pcc_index_timing(self._h, t))
        return list(t)

    def close(self):
        if getattr(self, "_h", None) and LIB is not None:  # (LIB is gone when the interpreter tears the module down)
            LIB.pcc_index_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def size(self) -> int:
        n = C.c_size_t(0)
        _check(LIB.pcc_index_size(self._h, C.byref(n)))
        return n.value

    @property
    def engine(self) -> int:
        e = C.c_int(0)
        _check(LIB.pcc_index_engine(self._h, C.byref(e)))
        return e.value

    def set_engine(self, engine: int):
        _check(LIB.pcc_index_set_engine(self._h, engine))

    def set_tie_order(self, ties: int):
        """TIES_LOWEST_INDEX (default) or TIES_FLANN: which of several equally near references nn1 / match_knn name"""
        _check(LIB.pcc_index_set_tie_order(self._h, ties))
        self._ties = ties

    def set_stream(self, stream_ptr: int):
        _check(LIB.pcc_index_set_stream(self._h, C.c_void_p(stream_ptr)))

    def wait_stream(self, stream_ptr: int):
        """pcc_index_wait_stream: calls made after this one start only when everything submitted so far to the stream
        `stream_ptr` (a hipStream_t as an integer, e.g. torch.cuda.Stream().cuda_stream) has finished"""
        _check(LIB.pcc_index_wait_stream(self._h, C.c_void_p(stream_ptr)))

    def stream_wait(self, stream_ptr: int):
        """pcc_stream_wait_index: work submitted to `stream_ptr` from now on waits for what the index has been asked so far"""
        _check(LIB.pcc_stream_wait_index(self._h, C.c_void_p(stream_ptr)))

    def sync(self):
        _check(LIB.pcc_index_sync(self._h))

    def stats(self):
        s = (C.c_uint64 * 8)()
        _check(LIB.pcc_index_stats(self._h, s))
        return list(s)

    # -- searches ------------------------------------------------------------
    def nn1(self, queries, out_idx=None, out_d2=None):
        ptr, n, stride, mem = _points(queries)
        if out_idx is None:
            out_idx, pi = _out(queries, (n,), np.int32)
        else:
            pi = out_idx.data_ptr() if _is_torch(out_idx) else out_idx.ctypes.data
        if out_d2 is None:
            out_d2, pd = _out(queries, (n,), np.float32)
        else:
            pd = out_d2.data_ptr() if _is_torch(out_d2) else out_d2.ctypes.data
        st = self._before(queries, out_idx, out_d2)
        _check(LIB.pcc_nn1(self._h, ptr, n, stride, mem, pi, pd))
        self._after(st)
        return out_idx, out_d2

    def knn(self, queries, k: int):
        ptr, n, stride, mem = _points(queries)
        idx, pi = _out(queries, (n, k), np.int32)
        d2, pd = _out(queries, (n, k), np.float32)
        st = self._before(queries)
        _check(LIB.pcc_knn(self._h, ptr, n, stride, mem, k, pi, pd))
        self._after(st)
        return idx, d2

    def radius_count(self, queries, radius: float, max_nn: int = 0):
        ptr, n, stride, mem = _points(queries)
        cnt, pc = _out(queries, (n,), np.int32)
        st = self._before(queries)
        _check(LIB.pcc_radius_count_max(self._h, ptr, n, stride, mem, float(radius), int(max_nn), pc))
        self._after(st)
        return cnt

    def voxel_grid(self, points, leaf: float, has_rgb: bool = False):
        """pcl::VoxelGrid centroids of `points` (host array (n, >=3) float32; rgb word in column 4)."""
        ptr, n, stride, mem = _points(points)
        assert mem == MEM_HOST
        out = np.zeros((n, points.shape[1]), dtype=np.float32)
        cnt = C.c_size_t(0)
        _check(LIB.pcc_voxel_grid(self._h, ptr, n, stride, mem, np.float32(leaf), int(has_rgb), out.ctypes.data,
                                  out.strides[0] if n > 1 else points.shape[1] * 4, C.byref(cnt)))
        return out[:cnt.value]

    def first_within(self, queries, radius: float):
        """lowest index of a reference within `radius` (double-precision test), -1 if none"""
        ptr, n, stride, mem = _points(queries)
        idx, pi = _out(queries, (n,), np.int32)
        st = self._before(queries)
        _check(LIB.pcc_first_within(self._h, ptr, n, stride, mem, float(radius), pi))
        self._after(st)
        return idx

    def radius_search(self, queries, radius: float, sorted: bool = True, max_nn: int = 0):
        """CSR (offsets, idx, d2) of all neighbours with d2 < float(radius^2); max_nn > 0: the max_nn nearest of them."""
        ptr, n, stride, mem = _points(queries)
        cnt = self.radius_count(queries, radius, max_nn)
        if _is_torch(cnt):
            import torch
            if not self.auto_sync:
                self.sync()  # device results are written on the library's stream, torch works on its own
            offs = torch.zeros(n + 1, dtype=torch.int64, device=cnt.device)
            offs[1:] = torch.cumsum(cnt.to(torch.int64), 0)
            total = int(offs[-1].item())
            po = offs.data_ptr()
        else:
            offs = np.zeros(n + 1, dtype=np.int64)
            np.cumsum(cnt, out=offs[1:])
            total = int(offs[-1])
            po = offs.ctypes.data
        idx, pi = _out(queries, (max(total, 1),), np.int32)
        d2, pd = _out(queries, (max(total, 1),), np.float32)
        st = self._before(queries, offs)
        _check(LIB.pcc_radius_fill_max(self._h, ptr, n, stride, mem, float(radius), int(sorted), int(max_nn), po, pi, pd))
        self._after(st)
        return offs, idx[:total], d2[:total]

    def radius_fill(self, queries, radius: float, offsets, sorted: bool = True, max_nn: int = 0):
        """the fill pass alone, for CSR offsets the caller already holds (host queries, numpy int64 offsets[nq + 1])"""
        ptr, n, stride, mem = _points(queries)
        assert mem == MEM_HOST and len(offsets) == n + 1
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        total = int(offs[-1])
        idx = np.empty(max(total, 1), np.int32)
        d2 = np.empty(max(total, 1), np.float32)
        _check(LIB.pcc_radius_fill_max(self._h, ptr, n, stride, mem, float(radius), int(sorted), int(max_nn), offs.ctypes.data,
                                       idx.ctypes.data, d2.ctypes.data))
        return idx[:total], d2[:total]

    def euclidean_clusters(self, tolerance: float, min_size: int, max_size: int, device_out=None,
                           max_sizes: int = 65536):
        if device_out is not None:
            labels, pl = _out(device_out, (self.n_original,), np.int32)
            mem = MEM_DEVICE
        else:
            labels = np.empty(self.n_original, dtype=np.int32)
            pl, mem = labels.ctypes.data, MEM_HOST
        ncl = C.c_int32(0)
        sizes = np.zeros(max_sizes, dtype=np.int32)
        st = self._before(device_out)
        _check(LIB.pcc_euclidean_clusters(self._h, float(tolerance), min_size, max_size, mem, pl,
                                          C.byref(ncl), sizes.ctypes.data, max_sizes))
        self._after(st)
        return labels, ncl.value, sizes[:min(ncl.value, max_sizes)]

    def sor(self, mean_k: int = 50, stddev_mult: float = 1.5, device=None):
        """pcl::StatisticalOutlierRemoval over the indexed cloud: (mean distances, inlier mask, threshold, kept).
        device: a torch device -> the two arrays stay in HBM (torch tensors), nothing cloud-sized crosses PCIe."""
        thr = C.c_double(0)
        kept = C.c_size_t(0)
        if device is not None:
            import torch
            md = torch.empty(self.n_original, dtype=torch.float32, device=device)
            inl = torch.empty(self.n_original, dtype=torch.uint8, device=device)
            st = self._before(md)
            _check(LIB.pcc_sor(self._h, mean_k, float(stddev_mult), MEM_DEVICE, md.data_ptr(), inl.data_ptr(), C.byref(thr), C.byref(kept)))
            self._after(st)
            return md, inl, thr.value, kept.value
        md = np.empty(self.n_original, dtype=np.float32)
        inl = np.empty(self.n_original, dtype=np.uint8)
        _check(LIB.pcc_sor(self._h, mean_k, float(stddev_mult), MEM_HOST, md.ctypes.data, inl.ctypes.data,
                           C.byref(thr), C.byref(kept)))
        return md, inl, thr.value, kept.value

    def sor_on_device(self) -> bool:
        """whether the last sor() took its sums, threshold and mask on the device (else: the in-order host loop)"""
        f = C.c_int(0)
        _check(LIB.pcc_index_sor_on_device(self._h, C.byref(f)))
        return bool(f.value)

    def sor_partial(self, start: int, count: int, mean_k: int = 50):
        """mean distances of the points [start, start + count) and the shard's share of the statistics (pcc_sor_partial)"""
        md = np.empty(count, dtype=np.float32)
        sums = (C.c_double * 4)()
        _check(LIB.pcc_sor_partial(self._h, start, count, mean_k, MEM_HOST, md.ctypes.data, sums))
        return md, np.array(list(sums))

    def sor_sharded(self, comm: "Comm", start: int, count: int, mean_k: int = 50, stddev_mult: float = 1.5):
        md = np.empty(count, dtype=np.float32)
        inl = np.empty(count, dtype=np.uint8)
        thr, kept = C.c_double(0), C.c_size_t(0)
        _check(LIB.pcc_sor_sharded(self._h, comm._c, start, count, mean_k, float(stddev_mult), MEM_HOST, md.ctypes.data,
                                   inl.ctypes.data, C.byref(thr), C.byref(kept)))
        return md, inl, thr.value, kept.value

    def icp_align_sharded(self, comm: "Comm", source_shard, max_iter: int = 20, fixed: bool = False):
        """pcc_icp_align_sharded: (T 4x4, fitness over all shards, iterations, converged)"""
        ptr, n, stride, mem = _points(source_shard)
        T = (C.c_float * 16)()
        fit, it, conv = C.c_double(0), C.c_int(0), C.c_int(0)
        st = self._before(source_shard)
        _check(LIB.pcc_icp_align_sharded(self._h, comm._c, ptr, n, stride, mem, max_iter, int(fixed), T, C.byref(fit),
                                         C.byref(it), C.byref(conv)))
        self._after(st)
        return np.array(list(T), dtype=np.float32).reshape(4, 4), fit.value, it.value, bool(conv.value)

    def sac_plane(self, points, max_iterations: int = 100, threshold: float = 0.02, probability: float = 0.99,
                  optimize: bool = True):
        """pcl::SACSegmentation(PLANE, RANSAC).segment on `points`: (inlier indices, coefficients[4], iterations)."""
        ptr, n, stride, mem = _points(points)
        inl, pi = _out(points, (max(n, 1),), np.int32)
        cnt = C.c_size_t(0)
        its = C.c_int(0)
        coeff = np.zeros(4, dtype=np.float32)
        st = self._before(points)
        _check(LIB.pcc_sac_plane(self._h, ptr, n, stride, mem, max_iterations, float(threshold), float(probability),
                                 int(optimize), pi, C.byref(cnt), coeff.ctypes.data, C.byref(its)))
        self._after(st)
        return inl[:cnt.value], coeff, its.value

    def plane_removal(self, points, stop_fraction: float = 0.3, max_iterations: int = 100, threshold: float = 0.02,
                      probability: float = 0.99, optimize: bool = True, max_planes: int = 64, with_points: bool = False,
                      record_bytes: int | None = None):
        """pcc_plane_removal: the reference's plane-removal loop (src/segmentation.cpp:79-117) with the cloud staged once.
        points: (n, >= 3) float32 numpy array or torch tensor (a CUDA tensor gives CUDA index arrays and points).
        Returns (remaining_index, plane_of_point, coefficients (p, 4), sizes (p,), iterations (p,), ended_without_model
        [, points]): with_points adds the remaining points' records, the first record_bytes of each input row (default: the
        whole row) as an (n_remaining, record_bytes / 4) float32 array.  More than max_planes planes raises PccError
        (PCC_ERR_OVERFLOW) whose `partial` holds (coefficients, sizes, iterations, n_remaining) of the planes found."""
        ptr, n, stride, mem = _points(points)
        max_planes = int(max_planes)
        assert max_planes >= 0, "max_planes must not be negative"
        row = int(points.shape[1]) * 4
        record_bytes = row if record_bytes is None else int(record_bytes)
        if with_points:
            assert record_bytes % 4 == 0 and 12 <= record_bytes <= row, "record_bytes: a multiple of 4 from 12 to the row's length"
        rem, p_rem = _out(points, (max(n, 1),), np.int32)
        pop, p_pop = _out(points, (max(n, 1),), np.int32)
        out, p_out = _out(points, (max(n, 1), record_bytes // 4), np.float32) if with_points else (None, None)
        coeff = np.zeros((max(max_planes, 1), 4), dtype=np.float32)
        sizes = np.zeros(max(max_planes, 1), dtype=np.uint32)
        its = np.zeros(max(max_planes, 1), dtype=np.int32)
        n_planes, n_rem, ended = C.c_size_t(0), C.c_size_t(0), C.c_int(0)
        st = self._before(points)
        status = LIB.pcc_plane_removal(self._h, ptr, n, stride, mem, float(stop_fraction), int(max_iterations), float(threshold),
                                       float(probability), int(optimize), max_planes, coeff.ctypes.data, sizes.ctypes.data,
                                       its.ctypes.data, C.byref(n_planes), C.byref(ended), p_pop, p_rem, C.byref(n_rem), p_out,
                                       record_bytes, record_bytes)
        self._after(st)
        p = n_planes.value
        if status != 0:
            err = PccError(status, (LIB.pcc_last_error() or b"").decode())
            err.partial = (coeff[:p], sizes[:p], its[:p], n_rem.value)
            raise err
        res = (rem[:n_rem.value], pop[:n], coeff[:p], sizes[:p], its[:p], bool(ended.value))
        return res + (out[:n_rem.value],) if with_points else res

    def extract_clusters(self, records, labels, n_clusters: int, record_bytes: int | None = None, with_records: bool = True):
        """pcc_extract_clusters: labels -> one cloud per cluster (the loop both segmentation paths of the reference end with,
        src/segmentation.cpp:133-152 and :290-318), a stable partition of the point indices by label on the device.
        records: (n, >= 3) float32 numpy array or torch tensor; labels: (n,) int32 in the same memory space, -1 = left out.
        Returns (index, offsets[, records]): cluster c is index[offsets[c]:offsets[c + 1]] -- its points in ascending order --
        and, with_records, the first record_bytes (default: the whole row) of each of them as an (m, record_bytes / 4) float32
        array.  A label outside [-1, n_clusters) raises PccError (PCC_ERR_INVALID)."""
        ptr, n, stride, mem = _points(records)
        n_clusters = int(n_clusters)
        assert n_clusters >= 0, "n_clusters must not be negative"
        if _is_torch(labels):
            import torch
            assert labels.dtype == torch.int32 and labels.dim() == 1 and labels.is_contiguous() and labels.shape[0] == n
            assert labels.is_cuda == (mem == MEM_DEVICE), "records and labels must be in the same memory space"
            p_lab = labels.data_ptr()
        else:
            assert mem == MEM_HOST, "records and labels must be in the same memory space"
            labels = np.ascontiguousarray(labels, dtype=np.int32)
            assert labels.shape == (n,)
            p_lab = labels.ctypes.data
        row = int(records.shape[1]) * 4
        record_bytes = row if record_bytes is None else int(record_bytes)
        assert record_bytes % 4 == 0 and 12 <= record_bytes <= row, "record_bytes: a multiple of 4 from 12 to the row's length"
        index, p_index = _out(records, (max(n, 1),), np.int32)
        out, p_out = _out(records, (max(n, 1), record_bytes // 4), np.float32) if with_records else (None, None)
        offsets = np.zeros(n_clusters + 1, dtype=np.uintp)
        st = self._before(records, labels)
        status = LIB.pcc_extract_clusters(self._h, ptr, n, stride, record_bytes, p_lab, n_clusters, mem, p_out, record_bytes, p_index,
                                          offsets.ctypes.data)
        self._after(st)
        _check(status)
        m = int(offsets[n_clusters])
        offsets = offsets.astype(np.int64)
        return (index[:m], offsets, out[:m]) if with_records else (index[:m], offsets)

    def region_growing_segmentation(self, points, leaf: float = 0.025, has_rgb: bool = False, normal_k: int = 50, k: int = 100,
                                    smoothness: float = 3.0 / 180.0 * np.pi, curvature_threshold: float = 1.0, min_size: int = 50,
                                    max_size: int = 1000000, max_clusters: int = 4096):
        """pcc_region_growing_segmentation: the reference's default segmentation path (src/segmentation.cpp:218-327) in one call:
        VoxelGrid -> NormalEstimation (normal_k) -> RegionGrowing (k) -> one cloud per cluster, nothing cloud-sized crossing to
        the host in between.  points: (n, >= 3) float32 numpy array or torch tensor (a CUDA tensor gives CUDA results); has_rgb:
        the colour word in column 4 is averaged.  Returns a dict: filtered (nv, columns) records, normals (nv, 4), labels (nv,),
        n_clusters, offsets (n_clusters + 1,), cluster_points (m, columns), cluster_index (m,): cluster c is the slice
        offsets[c]:offsets[c + 1] of the last two.  More than max_clusters clusters raises PccError (PCC_ERR_OVERFLOW) whose
        `partial` holds the dict without the cluster arrays."""
        ptr, n, stride, mem = _points(points)
        max_clusters = int(max_clusters)
        assert max_clusters >= 0, "max_clusters must not be negative"
        cols = int(points.shape[1])
        cap = max(n, 1)
        filtered, p_f = _out(points, (cap, cols), np.float32)
        normals, p_n = _out(points, (cap, 4), np.float32)
        labels, p_l = _out(points, (cap,), np.int32)
        cpts, p_cp = _out(points, (cap, cols), np.float32) if max_clusters else (None, None)
        cidx, p_ci = _out(points, (cap,), np.int32) if max_clusters else (None, None)
        offsets = np.zeros(max_clusters + 1, dtype=np.uintp)
        nv, ncl = C.c_size_t(0), C.c_int32(0)
        st = self._before(points)
        status = LIB.pcc_region_growing_segmentation(self._h, ptr, n, stride, mem, float(leaf), int(has_rgb), int(normal_k), int(k),
                                                     float(smoothness), float(curvature_threshold), int(min_size), int(max_size), p_f,
                                                     cols * 4, C.byref(nv), p_n, p_l, max_clusters, C.byref(ncl), offsets.ctypes.data, p_cp,
                                                     p_ci)
        self._after(st)
        res = dict(filtered=filtered[:nv.value], normals=normals[:nv.value], labels=labels[:nv.value], n_clusters=ncl.value)
        if status != 0:
            err = PccError(status, (LIB.pcc_last_error() or b"").decode())
            err.partial = res
            raise err
        offs = offsets[:ncl.value + 1].astype(np.int64)
        m = int(offs[-1])
        res.update(offsets=offs, cluster_points=cpts[:m] if cpts is not None else None,
                   cluster_index=cidx[:m] if cidx is not None else None)
        return res

    def euclidean_cluster_segmentation(self, points, leaf: float = 0.025, has_rgb: bool = False, stop_fraction: float = 0.3,
                                       max_iterations: int = 100, threshold: float = 0.02, probability: float = 0.99,
                                       optimize: bool = True, max_planes: int = 64, tolerance: float = 0.05, min_size: int = 100,
                                       max_size: int = 250000, max_clusters: int = 4096):
        """pcc_euclidean_cluster_segmentation: the reference's -e segmentation path (src/segmentation.cpp:64-156) in one call:
        VoxelGrid -> the plane-removal loop -> EuclideanClusterExtraction -> one cloud per cluster, nothing cloud-sized crossing to
        the host in between.  points: (n, >= 3) float32 numpy array or torch tensor (a CUDA tensor gives CUDA results); has_rgb:
        the colour word in column 4 is averaged.  Returns a dict: n_filtered (the points after the voxel grid), points
        (n_remaining, columns) the records that remain after the planes, labels (n_remaining,), n_clusters, offsets
        (n_clusters + 1,), cluster_points (m, columns), cluster_index (m,): cluster c is the slice offsets[c]:offsets[c + 1] of
        the last two; coefficients (p, 4), plane_sizes (p,), iterations (p,), ended_without_model as Index.plane_removal gives
        them.  More than max_planes planes or max_clusters clusters raises PccError (PCC_ERR_OVERFLOW) whose `partial` holds the
        dict without the cluster arrays (after too many planes only its counts and plane tables are valid)."""
        ptr, n, stride, mem = _points(points)
        max_planes, max_clusters = int(max_planes), int(max_clusters)
        assert max_planes >= 0, "max_planes must not be negative"
        assert max_clusters >= 0, "max_clusters must not be negative"
        cols = int(points.shape[1])
        cap = max(n, 1)
        remaining, p_r = _out(points, (cap, cols), np.float32)
        labels, p_l = _out(points, (cap,), np.int32)
        cpts, p_cp = _out(points, (cap, cols), np.float32) if max_clusters else (None, None)
        cidx, p_ci = _out(points, (cap,), np.int32) if max_clusters else (None, None)
        offsets = np.zeros(max_clusters + 1, dtype=np.uintp)
        coeff = np.zeros((max(max_planes, 1), 4), dtype=np.float32)
        sizes = np.zeros(max(max_planes, 1), dtype=np.uint32)
        its = np.zeros(max(max_planes, 1), dtype=np.int32)
        nv, nr, n_planes, ended, ncl = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_int32(0), C.c_int32(0)
        st = self._before(points)
        status = LIB.pcc_euclidean_cluster_segmentation(
            self._h, ptr, n, stride, mem, float(leaf), int(has_rgb), float(stop_fraction), int(max_iterations), float(threshold),
            float(probability), int(optimize), max_planes, coeff.ctypes.data, sizes.ctypes.data, its.ctypes.data, C.byref(n_planes),
            C.byref(ended), float(tolerance), int(min_size), int(max_size), p_r, cols * 4, C.byref(nv), C.byref(nr), p_l, max_clusters,
            C.byref(ncl), offsets.ctypes.data, p_cp, p_ci)
        self._after(st)
        p = n_planes.value
        res = dict(n_filtered=nv.value, points=remaining[:nr.value], labels=labels[:nr.value], n_clusters=ncl.value,
                   coefficients=coeff[:p], plane_sizes=sizes[:p], iterations=its[:p], ended_without_model=bool(ended.value))
        if status != 0:
            err = PccError(status, (LIB.pcc_last_error() or b"").decode())
            err.partial = res
            raise err
        offs = offsets[:ncl.value + 1].astype(np.int64)
        m = int(offs[-1])
        res.update(offsets=offs, cluster_points=cpts[:m] if cpts is not None else None,
                   cluster_index=cidx[:m] if cidx is not None else None)
        return res

    def morphological_operator(self, points, window: float, op: int):
        """pcc_morphological_operator: pcl::applyMorphologicalOperator over `points` ((n, >= 3) float32 numpy array or torch
        tensor; a CUDA tensor gives a CUDA result): min / max of z over every point's inclusive xy box of side `window`.
        op: MORPH_ERODE, MORPH_DILATE, MORPH_OPEN or MORPH_CLOSE.  Returns the (n,) float32 heights."""
        ptr, n, stride, mem = _points(points)
        out, p_out = _out(points, (max(n, 1),), np.float32)
        st = self._before(points)
        status = LIB.pcc_morphological_operator(self._h, ptr, n, stride, mem, float(window), int(op), p_out)
        self._after(st)
        _check(status)
        return out[:n]

    def progressive_morphological_filter(self, points, max_window_size: int = 20, slope: float = 1.0, initial_distance: float = 0.5,
                                         max_distance: float = 3.0, cell_size: float = 1.0, base: float = 2.0,
                                         exponential: bool = True):
        """pcc_progressive_morphological_filter: pcl::ProgressiveMorphologicalFilter::extract over `points` ((n, >= 3) float32
        numpy array or torch tensor; a CUDA tensor gives a CUDA index array); the defaults are the reference's parameters
        (src/segmentation.cpp:330-387).  Returns (ground, pass_sizes): the original indices of the ground points, ascending, and
        the survivors after each window (int64 numpy array)."""
        ptr, n, stride, mem = _points(points)
        ground, p_g = _out(points, (max(n, 1),), np.int32)
        sizes = np.zeros(PMF_MAX_WINDOWS, dtype=np.uintp)
        ng = C.c_size_t(0)
        args = (int(max_window_size), float(slope), float(initial_distance), float(max_distance), float(cell_size), float(base),
                int(bool(exponential)))
        st = self._before(points)
        status = LIB.pcc_progressive_morphological_filter(self._h, ptr, n, stride, mem, *args, p_g, C.byref(ng), sizes.ctypes.data,
                                                          PMF_MAX_WINDOWS)
        self._after(st)
        _check(status)
        nw = len(pmf_windows(*args)[0])
        return ground[:ng.value], sizes[:nw].astype(np.int64)

    def ground_segmentation(self, points, leaf: float = 0.01, max_window_size: int = 20, slope: float = 1.0,
                            initial_distance: float = 0.5, max_distance: float = 3.0, cell_size: float = 1.0, base: float = 2.0,
                            exponential: bool = True):
        """pcc_ground_segmentation: the reference's ground_segmentation (src/segmentation.cpp:330-387) in one call: VoxelGrid ->
        ProgressiveMorphologicalFilter -> ExtractIndices, positive and negative, the filtered cloud staying on the device.
        points: (n, >= 3) float32 numpy array or torch tensor (a CUDA tensor gives CUDA results).  Returns a dict: filtered
        (nv, columns) records, ground_index (ng,), ground_points (ng, columns), object_points (nv - ng, columns)."""
        ptr, n, stride, mem = _points(points)
        cols = int(points.shape[1])
        cap = max(n, 1)
        filtered, p_f = _out(points, (cap, cols), np.float32)
        gidx, p_gi = _out(points, (cap,), np.int32)
        gpts, p_gp = _out(points, (cap, cols), np.float32)
        opts, p_op = _out(points, (cap, cols), np.float32)
        nv, ng = C.c_size_t(0), C.c_size_t(0)
        st = self._before(points)
        status = LIB.pcc_ground_segmentation(self._h, ptr, n, stride, mem, float(leaf), int(max_window_size), float(slope),
                                             float(initial_distance), float(max_distance), float(cell_size), float(base),
                                             int(bool(exponential)), p_f, cols * 4, C.byref(nv), p_gi, C.byref(ng), p_gp, p_op)
        self._after(st)
        _check(status)
        return dict(filtered=filtered[:nv.value], ground_index=gidx[:ng.value], ground_points=gpts[:ng.value],
                    object_points=opts[:nv.value - ng.value])

    def change_detection(self, a, b, resolution: float, min_points_per_leaf: int = 0, with_records: bool = False):
        """pcc_change_detection: the reference's spatial_change_detection (src/comparator.cpp:54-110) -- the points of `b` in
        voxels of side `resolution` that hold no point of `a` (pcl::octree::OctreePointCloudChangeDetector; the lattice is
        fixed by the first finite point of `a`).  a, b: (n, >= 3) float32 numpy arrays or torch tensors, row strides free; if
        either is a CUDA tensor the other is moved beside it and the results are CUDA tensors.  Returns the int32 indices into
        `b`, ascending; with_records=True: (indices, records), the rows of `b` they name, every column."""
        a_cuda, b_cuda = (_is_torch(x) and x.is_cuda for x in (a, b))
        if a_cuda != b_cuda:
            import torch
            if a_cuda:
                b = (b if _is_torch(b) else torch.from_numpy(b)).to(a.device)
            else:
                a = (a if _is_torch(a) else torch.from_numpy(a)).to(b.device)
        pa, na, sa, mem = _points(a)
        pb, nb, sb, mem_b = _points(b)
        assert mem == mem_b
        index, p_i = _out(b, (max(nb, 1),), np.int32)
        records, p_r = _out(b, (max(nb, 1), int(b.shape[1])), np.float32) if with_records else (None, None)
        if with_records:
            assert nb <= 1 or sb == int(b.shape[1]) * 4, "with_records needs the rows of b back to back"
        count = C.c_size_t(0)
        st = self._before(a, b)
        status = LIB.pcc_change_detection(self._h, pa, na, sa, pb, nb, sb, mem, float(resolution), int(min_points_per_leaf), p_i, p_r,
                                          C.byref(count))
        self._after(st)
        _check(status)
        return (index[:count.value], records[:count.value]) if with_records else index[:count.value]

    def normals(self, k: int = 50, viewpoint=None, device=None):
        """pcl::NormalEstimation over the index's own points: (n, 4) = nx, ny, nz, curvature.
        device: a torch cuda device to get the result as a device tensor."""
        vp = None
        if viewpoint is not None:
            vpa = np.ascontiguousarray(viewpoint, dtype=np.float32)
            vp = vpa.ctypes.data
        if device is not None:
            import torch
            out = torch.empty((self.n_original, 4), dtype=torch.float32, device=device)
            st = self._before(out)
            _check(LIB.pcc_normals(self._h, k, vp, MEM_DEVICE, out.data_ptr()))
            self._after(st)
            if st is None:
                self.sync()
            return out
        out = np.empty((self.n_original, 4), dtype=np.float32)
        _check(LIB.pcc_normals(self._h, k, vp, MEM_HOST, out.ctypes.data))
        return out

    def normals_radius(self, radius: float, viewpoint=None):
        """pcl::NormalEstimation with setRadiusSearch(radius): (n, 4) = nx, ny, nz, curvature (host array)."""
        vp = None
        if viewpoint is not None:
            vpa = np.ascontiguousarray(viewpoint, dtype=np.float32)
            vp = vpa.ctypes.data
        out = np.empty((self.n_original, 4), dtype=np.float32)
        _check(LIB.pcc_normals_radius(self._h, float(radius), vp, MEM_HOST, out.ctypes.data))
        return out

    def rift_descriptors(self, rgb, normal_radius: float = 0.03, gradient_radius: float = 0.03, rift_radius: float = 0.05,
                         nr_distance_bins: int = 4, nr_gradient_bins: int = 8):
        """pcc_rift_descriptors: the reference's processRIFT (src/comparator.cpp:590-684) for the indexed cloud.
        rgb, one entry per point of the cloud, numpy array or torch tensor (a CUDA tensor gives CUDA results):
          (n, 3) uint8 r, g, b;  (n,) uint32 / int32 packed colour words (bytes b, g, r, a from the low byte);  or the
          (n, >= 5) float32 records of pcl::PointXYZRGB (colour word in column 4), read in place with their stride.
        Returns (histograms (n_out, 32) float32, point index (n_out,) int32): the descriptors that survive both
        compactions and the original index of the point each belongs to."""
        n = self.n_original
        assert len(rgb) == n, "one colour per point of the indexed cloud"
        words, ptr, stride, mem = _colour_words(rgb)
        hist, ph = _out(words, (max(n, 1), 32), np.float32)
        index, pi = _out(words, (max(n, 1),), np.int32)
        n_out = C.c_size_t(0)
        st = self._before(words, hist)
        _check(LIB.pcc_rift_descriptors(self._h, ptr, stride, mem, float(normal_radius), float(gradient_radius), float(rift_radius),
                                        int(nr_distance_bins), int(nr_gradient_bins), ph, pi, C.byref(n_out)))
        self._after(st)
        return hist[:n_out.value], index[:n_out.value]

    def fpfh_descriptors(self, normal_radius: float = 0.03, fpfh_radius: float = 0.05, nr_bins=(11, 11, 11)):
        """pcc_fpfh_descriptors: the reference's processFPFH (src/comparator.cpp:824-875) for the indexed cloud.
        Returns (histograms (m, 33) float32: the f1, f2 and f3 bins; point index (m,) int32): one descriptor per point with a
        finite normal and the original index of that point.  A handle over a CUDA tensor gives CUDA tensors, any other NumPy
        arrays."""
        n = self.n_original
        like = None
        if getattr(self, "_cuda", None) is not None:
            import torch
            like = torch.empty(0, device=self._cuda)
        hist, ph = _out(like, (max(n, 1), 33), np.float32)
        index, pi = _out(like, (max(n, 1),), np.int32)
        b1, b2, b3 = nr_bins
        n_out = C.c_size_t(0)
        st = self._before(hist)
        _check(LIB.pcc_fpfh_descriptors(self._h, MEM_DEVICE if like is not None else MEM_HOST, float(normal_radius), float(fpfh_radius),
                                        int(b1), int(b2), int(b3), ph, pi, C.byref(n_out)))
        self._after(st)
        return hist[:n_out.value], index[:n_out.value]

    def shot_descriptors(self, normal_radius: float = 0.05, shot_radius: float = 0.04, with_rf: bool = True):
        """pcc_shot_descriptors: the deterministic part of the reference's processSHOT (src/comparator.cpp:941-986) for the
        indexed cloud.  Returns (descriptors (m, 352) float32, rf (m, 9) float32 -- the x, y and z axis of every local
        reference frame -- or None without with_rf, point index (m,) int32): one row per point with a finite normal and the
        original index of that point; a row of NaN where PCL gives none (fewer than 5 neighbours).  A handle over a CUDA
        tensor gives CUDA tensors, any other NumPy arrays."""
        n = self.n_original
        like = None
        if getattr(self, "_cuda", None) is not None:
            import torch
            like = torch.empty(0, device=self._cuda)
        desc, pd = _out(like, (max(n, 1), 352), np.float32)
        rf, pr = _out(like, (max(n, 1), 9), np.float32) if with_rf else (None, None)
        index, pi = _out(like, (max(n, 1),), np.int32)
        n_out = C.c_size_t(0)
        st = self._before(desc)
        _check(LIB.pcc_shot_descriptors(self._h, MEM_DEVICE if like is not None else MEM_HOST, float(normal_radius), float(shot_radius),
                                        pd, pr, pi, C.byref(n_out)))
        self._after(st)
        return desc[:n_out.value], (rf[:n_out.value] if with_rf else None), index[:n_out.value]

    def vfh_descriptor(self, normal_radius: float = 0.03):
        """pcc_vfh_descriptor: the reference's processVHF (src/comparator.cpp:482-516) for the indexed cloud -- its one global
        descriptor.  Returns (308,) float32: the 45 bins of f1, of f2, of f3 and of f4, then the 128 bins of the viewpoint
        component; a cloud of fewer than 2 points has none and gives an empty (0, 308) result.  A handle over a CUDA tensor
        gives a CUDA tensor, any other a NumPy array.  A cloud with a non-finite point is refused."""
        like = None
        if getattr(self, "_cuda", None) is not None:
            import torch
            like = torch.empty(0, device=self._cuda)
        hist, ph = _out(like, (1, 308), np.float32)
        n_out = C.c_size_t(0)
        st = self._before(hist)
        _check(LIB.pcc_vfh_descriptor(self._h, MEM_DEVICE if like is not None else MEM_HOST, float(normal_radius), ph, C.byref(n_out)))
        self._after(st)
        return hist[0] if n_out.value else hist[:0]

    def match_vfh(self, h1, h2):
        """pcc_match_vfh with this handle as the context: the reference's matchVHF (src/comparator.cpp:471-480) for every pair of
        two arrays of VFH descriptors, (n1, 308) and (n2, 308) float32 (a single (308,) descriptor counts as one row), both NumPy
        arrays or both CUDA tensors.  Returns the (n1, n2) float64 distances, a NumPy array or a CUDA tensor accordingly.  The
        cloud the handle indexes is neither read nor changed."""
        on_device = [_is_torch(x) and x.is_cuda for x in (h1, h2)]
        if any(on_device) and not all(on_device):
            raise ValueError("match_vfh takes NumPy arrays or CUDA tensors, not both in one call")
        if all(on_device):
            a, b = (x.reshape(-1, 308).contiguous() for x in (h1, h2))
            assert a.dtype == b.dtype and a.element_size() == 4 and a.dtype.is_floating_point, "VFH descriptors are float32"
            pa, pb, mem = a.data_ptr(), b.data_ptr(), MEM_DEVICE
        else:
            a, b = (np.ascontiguousarray(x.numpy() if _is_torch(x) else x, dtype=np.float32).reshape(-1, 308) for x in (h1, h2))
            pa, pb, mem = a.ctypes.data, b.ctypes.data, MEM_HOST
        n1, n2 = int(a.shape[0]), int(b.shape[0])
        out, po = _out(a, (n1, n2), np.float64)
        st = self._before(a, b, out) if mem == MEM_DEVICE else None
        _check(LIB.pcc_match_vfh(self._h, pa if n1 else None, n1, pb if n2 else None, n2, mem, po if n1 and n2 else None))
        self._after(st)
        return out

    def vfh_descriptors_batch(self, clouds_or_points, offsets=None, normal_radius: float = 0.03, return_packed: bool = False):
        """pcc_vfh_descriptors_batch with this handle as the context: the reference's processVHF for every cluster in one call.
        clouds_or_points: a list of (n, >= 3) float32 arrays of one kind (NumPy arrays or torch tensors, e.g. (n, 3) points or
        32-byte pcl::PointXYZRGB records; they are laid one behind the other for the call), or with `offsets` ONE such array,
        host or CUDA, read in place: cluster c is rows offsets[c] .. offsets[c + 1] -- what region_growing_segmentation /
        euclidean_cluster_segmentation return as cluster_points / offsets.  Returns one array per cluster, what
        Index(cluster).vfh_descriptor() returns: (308,) float32, or an empty (0, 308) for a cluster of fewer than 2 points
        (which is never read).  For CUDA input these are CUDA tensors, views of the call's one output tensor.
        return_packed: (hist (m, 308), offsets (n_clusters + 1,) uintp) instead -- the descriptors of the clusters that have
        one, in cluster order, and each cluster's rows offsets[c] .. offsets[c + 1]; match_vfh takes hist without a copy.  A
        cluster of 2 points and more with a non-finite point is refused.  The cloud the handle indexes is neither read nor
        changed."""
        if offsets is None:
            clouds = list(clouds_or_points)
            sizes = [len(c) for c in clouds]
            off_in = np.zeros(len(clouds) + 1, dtype=np.uintp)
            off_in[1:] = np.cumsum(sizes, dtype=np.uintp)
            some = [c for c in clouds if len(c)]
            if not some:
                points = np.zeros((0, 3), np.float32)
            elif _is_torch(some[0]):
                import torch
                points = some[0] if len(some) == 1 else torch.cat(some, 0)
            else:
                points = some[0] if len(some) == 1 else np.concatenate(some, 0)
        else:
            points = clouds_or_points
            off_in = np.ascontiguousarray(np.asarray(offsets.cpu() if _is_torch(offsets) else offsets), dtype=np.uintp)
        ptr, n, stride, mem = _points(points)
        assert off_in.ndim == 1 and len(off_in) >= 1, "offsets holds n_clusters + 1 entries"
        n_clusters = len(off_in) - 1
        assert n_clusters == 0 or int(off_in.max()) <= n, "offsets reach beyond the points"
        hist, ph = _out(points, (max(n_clusters, 1), 308), np.float32)
        off = np.zeros(n_clusters + 1, dtype=np.uintp)
        st = self._before(points, hist) if mem == MEM_DEVICE else None
        _check(LIB.pcc_vfh_descriptors_batch(self._h, ptr if n else None, stride, off_in.ctypes.data, n_clusters, mem, float(normal_radius), ph,
                                             off.ctypes.data))
        self._after(st)
        if return_packed:
            return hist[:int(off[-1])], off
        return [hist[int(off[c])] if off[c + 1] > off[c] else hist[:0] for c in range(n_clusters)]

    def fpfh_descriptors_batch(self, clouds_or_points, offsets=None, normal_radius: float = 0.03, fpfh_radius: float = 0.05,
                               nr_bins=(11, 11, 11)):
        """pcc_fpfh_descriptors_batch with this handle as the context: the reference's processFPFH for every cluster in one call.
        clouds_or_points: a list of (n, >= 3) float32 arrays of one kind (NumPy arrays or torch tensors, e.g. (n, 3) points or
        32-byte pcl::PointXYZRGB records; they are laid one behind the other for the call), or with `offsets` ONE such array,
        host or CUDA, read in place: cluster c is rows offsets[c] .. offsets[c + 1] -- what region_growing_segmentation /
        euclidean_cluster_segmentation return as cluster_points / offsets.  Returns one (histograms (m, 33) float32, point index
        (m,) int32 local to the cluster) per cluster, each what Index(cluster).fpfh_descriptors() returns; an empty cluster or one
        without a finite point gives m = 0.  For CUDA input these are CUDA tensors, views of the call's one output array:
        match_fpfh_batch takes them without a copy.  The cloud the handle indexes is neither read nor changed."""
        if offsets is None:
            clouds = list(clouds_or_points)
            sizes = [len(c) for c in clouds]
            off_in = np.zeros(len(clouds) + 1, dtype=np.uintp)
            off_in[1:] = np.cumsum(sizes, dtype=np.uintp)
            some = [c for c in clouds if len(c)]
            if not some:
                points = np.zeros((0, 3), np.float32)
            elif _is_torch(some[0]):
                import torch
                points = some[0] if len(some) == 1 else torch.cat(some, 0)
            else:
                points = some[0] if len(some) == 1 else np.concatenate(some, 0)
        else:
            points = clouds_or_points
            off_in = np.ascontiguousarray(np.asarray(offsets.cpu() if _is_torch(offsets) else offsets), dtype=np.uintp)
        ptr, n, stride, mem = _points(points)
        assert off_in.ndim == 1 and len(off_in) >= 1, "offsets holds n_clusters + 1 entries"
        n_clusters = len(off_in) - 1
        assert n_clusters == 0 or int(off_in.max()) <= n, "offsets reach beyond the points"
        total = int(off_in[-1]) - int(off_in[0]) if n_clusters and off_in[-1] >= off_in[0] else 0
        hist, ph = _out(points, (max(total, 1), 33), np.float32)
        index, pi = _out(points, (max(total, 1),), np.int32)
        off = np.zeros(n_clusters + 1, dtype=np.uintp)
        b1, b2, b3 = nr_bins
        st = self._before(points, hist, index) if mem == MEM_DEVICE else None
        _check(LIB.pcc_fpfh_descriptors_batch(self._h, ptr if n else None, stride, off_in.ctypes.data, n_clusters, mem, float(normal_radius),
                                              float(fpfh_radius), int(b1), int(b2), int(b3), ph, pi, off.ctypes.data))
        self._after(st)
        return [(hist[int(off[c]):int(off[c + 1])], index[int(off[c]):int(off[c + 1])]) for c in range(n_clusters)]

    def rift_descriptors_batch(self, clouds, rgbs=None, normal_radius: float = 0.03, gradient_radius: float = 0.03,
                               rift_radius: float = 0.05, nr_distance_bins: int = 4, nr_gradient_bins: int = 8):
        """pcc_rift_descriptors_batch with this handle as the context: the descriptors of every cloud in one call (the
        reference's per-cluster loop, src/comparator.cpp:1224-1272).  clouds[c]: (n, >= 3) float32 numpy array with rgbs[c]
        in any of rift_descriptors' three forms, or (n, >= 5) pcl::PointXYZRGB records with rgbs omitted (the colour word is
        read in place).  Returns one (histograms (m, 32) float32, point index (m,) int32) per cloud, each what
        Index(clouds[c]).rift_descriptors(rgbs[c]) returns; an empty cloud or one without a finite point gives m = 0.  The
        cloud the handle indexes is neither read nor changed."""
        b = _cloud_batch(clouds, rgbs, "pcc_rift_descriptors_batch")
        n, total = b.n, sum(b.counts[:b.n])
        hist = np.empty((max(total, 1), 32), dtype=np.float32)
        index = np.empty(max(total, 1), dtype=np.int32)
        off = np.zeros(n + 1, dtype=np.uintp)
        _check(LIB.pcc_rift_descriptors_batch(self._h, n, b.pts, b.counts, b.stride, b.rgb, b.rgb_stride, MEM_HOST, float(normal_radius),
                                              float(gradient_radius), float(rift_radius), int(nr_distance_bins), int(nr_gradient_bins),
                                              hist.ctypes.data, index.ctypes.data, off.ctypes.data))
        return [(hist[int(off[c]):int(off[c + 1])].copy(), index[int(off[c]):int(off[c + 1])].copy()) for c in range(n)]

    def sift_keypoints(self, points, rgb, min_scale: float = 0.005, nr_octaves: int = 5, nr_scales_per_octave: int = 5,
                       min_contrast: float = 0.001):
        """pcc_sift_keypoints: the reference's processSift (src/comparator.cpp:435-469, pcl::SIFTKeypoint) for `points`, an
        (n, >= 3) float32 numpy array or torch tensor; this handle is the context only (device, stream, scratch), the cloud it
        indexes is not read.  rgb: one colour per point in any of rift_descriptors' three forms, in the memory space of
        `points` (the records themselves may be passed for both).  Returns (m, 4) float32 x, y, z, scale in the detector's
        order (octave, point of the octave cloud, scale) -- a CUDA tensor for CUDA input."""
        ptr, n, stride, mem = _points(points)
        assert len(rgb) == n, "one colour per point"
        words, cptr, cstride, cmem = _colour_words(rgb)
        assert cmem == mem, "points and colours live in the same memory space"
        found = C.c_size_t(0)
        capacity = 256
        for attempt in range(2):
            out, po = _out(points, (capacity, 4), np.float32)
            st = self._before(points, words, out)
            status = LIB.pcc_sift_keypoints(self._h, ptr, n, stride, cptr, cstride, mem, float(min_scale), int(nr_octaves),
                                            int(nr_scales_per_octave), float(min_contrast), po, capacity, C.byref(found))
            self._after(st)
            if status == -6 and attempt == 0:  # PCC_ERR_OVERFLOW: once more with the room it asks for
                capacity = found.value
                continue
            _check(status)
            break
        return out[:found.value]

    def sift_keypoints_batch(self, clouds, rgbs=None, min_scale: float = 0.005, nr_octaves: int = 5, nr_scales_per_octave: int = 5,
                             min_contrast: float = 0.001, snap_radius=None):
        """pcc_sift_keypoints_batch with this handle as the context: the SIFT keypoints of every cloud in one call, and with
        snap_radius the first point of its own cloud within that radius of every keypoint (the front of the reference's
        processRIFTwithSIFT, src/comparator.cpp:686-822, for all clusters at once).  clouds[c] / rgbs[c]: host arrays in any
        of sift_keypoints' forms ((n, >= 5) pcl::PointXYZRGB records with rgbs omitted: the colour word is read in place).
        Returns (keypoints (m, 4) float32, offsets (n_clouds + 1,) -- cloud c owns rows offsets[c] .. offsets[c + 1], each slice
        what sift_keypoints returns for that cloud alone --[, snap index (m,) int32, local to the cloud, -1 for none])."""
        b = _cloud_batch(clouds, rgbs, "pcc_sift_keypoints_batch")
        n = b.n
        off = np.zeros(n + 1, dtype=np.uintp)
        capacity = max(256, sum(b.counts[:n]) // 8)
        for attempt in range(2):
            kp = np.empty((capacity, 4), dtype=np.float32)
            snap = np.empty(capacity, dtype=np.int32) if snap_radius is not None else None
            status = LIB.pcc_sift_keypoints_batch(self._h, n, b.pts, b.counts, b.stride, b.rgb, b.rgb_stride, MEM_HOST, float(min_scale), int(nr_octaves),
                                                  int(nr_scales_per_octave), float(min_contrast), 0.0 if snap_radius is None else float(snap_radius),
                                                  kp.ctypes.data, None if snap is None else snap.ctypes.data, capacity, off.ctypes.data)
            if status == -6 and attempt == 0:  # PCC_ERR_OVERFLOW: once more with the room it asks for
                capacity = int(off[n])
                continue
            _check(status)
            break
        m = int(off[n])
        offsets = off.astype(np.int64)
        return (kp[:m], offsets) if snap is None else (kp[:m], offsets, snap[:m])

    def cluster_descriptors(self, points, rgb=None, offsets=None, sift_above: int | None = 700, min_scale: float = 0.005, nr_octaves: int = 5,
                            nr_scales_per_octave: int = 5, min_contrast: float = 0.001, snap_radius: float = 0.05,
                            normal_radius: float = 0.03, gradient_radius: float = 0.03, rift_radius: float = 0.05,
                            nr_distance_bins: int = 4, nr_gradient_bins: int = 8, capacity: int | None = None):
        """pcc_cluster_descriptors with this handle as the context: the reference's per-cluster descriptor loop
        (src/comparator.cpp:1224-1290) in one call.  points: (n, >= 3) float32 numpy array or torch tensor (host or CUDA); rgb: one
        colour per point in any of rift_descriptors' three forms, in the memory space of `points`, or None when `points` are
        pcl::PointXYZRGB records (the colour word is read in place); offsets: (n_clusters + 1,) non-decreasing, cluster c is
        points[offsets[c]:offsets[c + 1]] -- what region_growing_segmentation / euclidean_cluster_segmentation return as
        cluster_points / offsets.  Clusters above sift_above points take SIFT keypoints, their snap and RIFT over the snapped
        points; the others RIFT over all their points (sift_above=None: every cluster).  Returns a dict: histograms (m, 32) float32,
        point_index (m,) int32 local to the cluster, offsets (n_clusters + 1,) int64 -- cluster c owns rows offsets[c] ..
        offsets[c + 1] --, n_keypoints (n_clusters,) uint32, centroids (n_clusters, 3) float32.  Too little capacity is retried
        once with the room the call asks for."""
        ptr, n, stride, mem = _points(points)
        if rgb is None:
            assert points.shape[1] >= 5, "PointXYZRGB records have their colour word in column 4"
            words, cptr, cstride, cmem = points, (ptr + 16 if n else ptr), stride, mem
        else:
            assert len(rgb) == n, "one colour per point"
            words, cptr, cstride, cmem = _colour_words(rgb) if n else (rgb, None, 4, mem)
        assert cmem == mem, "points and colours live in the same memory space"
        assert offsets is not None, "offsets: the clusters' bounds"
        off_in = np.ascontiguousarray(np.asarray(offsets), dtype=np.uintp)
        assert off_in.ndim == 1 and len(off_in) >= 1, "offsets holds n_clusters + 1 entries"
        n_clusters = len(off_in) - 1
        assert n_clusters == 0 or int(off_in.max()) <= n, "offsets reach beyond the points"
        gate = (2 ** (8 * C.sizeof(C.c_size_t)) - 1) if sift_above is None else int(sift_above)
        assert gate >= 0, "sift_above must not be negative"
        off = np.zeros(n_clusters + 1, dtype=np.uintp)
        nkp = np.zeros(max(n_clusters, 1), dtype=np.uint32)
        cent = np.zeros((max(n_clusters, 1), 3), dtype=np.float32)
        capacity = max(256, n) if capacity is None else int(capacity)
        for attempt in range(2):
            hist = np.empty((max(capacity, 1), 32), dtype=np.float32)
            index = np.empty(max(capacity, 1), dtype=np.int32)
            st = self._before(points, words)
            status = LIB.pcc_cluster_descriptors(self._h, ptr if n else None, stride, cptr if n else None, cstride, off_in.ctypes.data, n_clusters,
                                                 mem, gate, float(min_scale), int(nr_octaves), int(nr_scales_per_octave), float(min_contrast),
                                                 float(snap_radius), float(normal_radius), float(gradient_radius), float(rift_radius),
                                                 int(nr_distance_bins), int(nr_gradient_bins), hist.ctypes.data, index.ctypes.data, capacity,
                                                 off.ctypes.data, nkp.ctypes.data, cent.ctypes.data)
            self._after(st)
            if status == -6 and attempt == 0:  # PCC_ERR_OVERFLOW: once more with the room it asks for
                capacity = int(off[n_clusters])
                continue
            _check(status)
            break
        m = int(off[n_clusters])
        return dict(histograms=hist[:m], point_index=index[:m], offsets=off.astype(np.int64), n_keypoints=nkp[:n_clusters],
                    centroids=cent[:n_clusters])

    def cluster_matching(self, des1, offsets1, des2, offsets2, centroids1, centroids2, points1, points2, threshold: float = 0.05, dim: int = 3):
        """pcc_cluster_matching with this handle as the context: the reference's cluster-matching loop (src/comparator.cpp:1296-1366)
        in one call.  des1 / des2: the descriptors of all clusters of a scene one behind the other, (n, >= dim) float32 numpy arrays
        or torch CUDA tensors (both in the same memory space; rows may be strided) -- with offsets what cluster_descriptors returns
        as histograms / offsets; offsets_s: (n_clusters_s + 1,) non-decreasing, cluster c of scene s owns rows offsets_s[c] ..
        offsets_s[c + 1]; centroids_s: (n_clusters_s, 3) float32; points_s: (n_clusters_s,) the clusters' point counts.  The first
        `dim` floats of every record are searched.  Returns a dict: candidates (n_clusters1, 3) int32 -- the three nearest free
        clusters of scene 2 by centroid, -1: none --, state (n_clusters1, 3) int32 -- 0 no candidate, 1 gated out by the descriptor
        counts, 2 gated out by size, 3 searched --, correspondences (n_clusters1, 3) uint32 -- the length of the row match_knn_batch
        returns for a searched pair, else 0 --, matches (n_clusters1,) int32 -- the accepted cluster of scene 2, or -1."""
        sides = []
        for des in (des1, des2):
            if _is_torch(des):
                assert des.dtype.is_floating_point and des.element_size() == 4 and des.dim() == 2, "descriptors: (n, >= dim) float32"
                assert des.shape[0] == 0 or des.stride(1) == 1
                stride = des.stride(0) * 4 if des.shape[0] > 1 else des.shape[1] * 4
                sides.append((des.data_ptr() if des.shape[0] else None, des.shape[0], des.shape[1], stride, MEM_DEVICE if des.is_cuda else MEM_HOST))
            else:
                assert isinstance(des, np.ndarray) and des.dtype == np.float32 and des.ndim == 2, "descriptors: (n, >= dim) float32"
                assert des.shape[0] == 0 or des.strides[1] == 4
                stride = des.strides[0] if des.shape[0] > 1 else des.shape[1] * 4
                sides.append((des.ctypes.data if des.shape[0] else None, des.shape[0], des.shape[1], stride, MEM_HOST))
        (p1, n1, w1, s1, m1), (p2, n2, w2, s2, m2) = sides
        if n1 == 0 or n2 == 0:  # (an empty side has no memory space and no stride of its own)
            if n1 == 0:
                s1, m1, w1 = s2, m2, w2
            if n2 == 0:
                s2, m2, w2 = s1, m1, w1
        assert m1 == m2, "both descriptor arrays live in the same memory space"
        assert s1 == s2, "both descriptor arrays have the same row stride"
        offs = []
        for off, n in ((offsets1, n1), (offsets2, n2)):
            assert off is not None, "offsets: the clusters' bounds"
            o = np.ascontiguousarray(np.asarray(off), dtype=np.uintp)
            assert o.ndim == 1 and len(o) >= 1, "offsets holds n_clusters + 1 entries"
            assert len(o) == 1 or int(o.max()) <= n, "offsets reach beyond the descriptors"
            offs.append(o)
        nc1, nc2 = len(offs[0]) - 1, len(offs[1]) - 1
        cents, pts = [], []
        for c, p, nc in ((centroids1, points1, nc1), (centroids2, points2, nc2)):
            c = np.ascontiguousarray(np.asarray(c, dtype=np.float32).reshape(-1, 3))
            p = np.ascontiguousarray(np.asarray(p), dtype=np.uintp).reshape(-1)
            assert len(c) == nc and len(p) == nc, "one centroid and one point count per cluster"
            cents.append(c)
            pts.append(p)
        cand = np.full((max(nc1, 1), 3), -1, dtype=np.int32)
        state = np.zeros((max(nc1, 1), 3), dtype=np.int32)
        corr = np.zeros((max(nc1, 1), 3), dtype=np.uint32)
        matches = np.full(max(nc1, 1), -1, dtype=np.int32)
        st = self._before(des1, des2)
        status = LIB.pcc_cluster_matching(self._h, p1, offs[0].ctypes.data, nc1, p2, offs[1].ctypes.data, nc2, s1, int(dim), m1,
                                          cents[0].ctypes.data if nc1 else None, cents[1].ctypes.data if nc2 else None,
                                          pts[0].ctypes.data if nc1 else None, pts[1].ctypes.data if nc2 else None, float(threshold),
                                          cand.ctypes.data, state.ctypes.data, corr.ctypes.data, matches.ctypes.data)
        self._after(st)
        _check(status)
        return dict(candidates=cand[:nc1], state=state[:nc1], correspondences=corr[:nc1], matches=matches[:nc1])

    def match_colour_elements(self, points1, offsets1, points2, offsets2, matches, rgb1=None, rgb2=None, min_points: int = 10,
                              distance: float = 10.0, point_colour: float = 6.0, region_colour: float = 5.0, min_size: int = 200,
                              max_size: int | None = None, nn: int = 30, region_nn: int = 100):
        """pcc_match_colour_elements with this handle as the context: the colour-element counts of the reference's match loop
        (src/comparator.cpp:1379-1509) in one call.  points_s: the clusters of scene s one behind the other, (n, >= 3) float32 numpy
        arrays (host) or torch CUDA tensors (device), both in the same memory space with the same row stride; offsets_s:
        (n_clusters_s + 1,) non-decreasing, cluster c owns rows offsets_s[c] .. offsets_s[c + 1] -- what
        region_growing_segmentation / euclidean_cluster_segmentation return as cluster_points / offsets; rgb_s: one colour per
        point in any of rift_descriptors' three forms, in the memory space of the points, or None when the points are (n, 8)
        pcl::PointXYZRGB records (rgb = pts + 16).  matches: (n_clusters1,) the matched cluster of scene 2 or -1, what
        cluster_matching returns.  Returns an (n_clusters1, 2) int32 array: row i is (-1, -1) without a match, else the counts of
        cluster i of scene 1 and of cluster matches[i] of scene 2; a cluster with at most min_points finite points counts 0, any
        other what Index(cluster).region_growing_rgb(...) counts.  Every distinct cluster is segmented once."""
        sides = []
        for points, rgb in ((points1, rgb1), (points2, rgb2)):
            ptr, n, stride, mem = _points(points)
            if rgb is None:
                assert points.shape[1] >= 5, "PointXYZRGB records have their colour word in column 4"
                words, cptr, cstride, cmem = points, ptr + 16, stride, mem
            else:
                assert len(rgb) == n, "one colour per point"
                words, cptr, cstride, cmem = _colour_words(rgb) if n else (rgb, None, 4, mem)
            assert cmem == mem, "points and colours live in the same memory space"
            sides.append([ptr if n else None, cptr if n else None, n, stride, cstride, mem, words])
        a, b = sides
        for x, y in ((a, b), (b, a)):  # (an empty side has no memory space and no strides of its own)
            if x[2] == 0:
                x[3:6] = y[3:6]
            elif x[2] == 1 and y[2] > 1:
                x[3:5] = y[3:5]
        assert a[5] == b[5], "both scenes live in the same memory space"
        assert a[3] == b[3] and a[4] == b[4], "both scenes have the same row stride, and so both colour arrays"
        offs = []
        for off, side in ((offsets1, a), (offsets2, b)):
            assert off is not None, "offsets: the clusters' bounds"
            o = np.ascontiguousarray(np.asarray(off), dtype=np.uintp)
            assert o.ndim == 1 and len(o) >= 1, "offsets holds n_clusters + 1 entries"
            assert len(o) == 1 or int(o.max()) <= side[2], "offsets reach beyond the points"
            offs.append(o)
        nc1, nc2 = len(offs[0]) - 1, len(offs[1]) - 1
        m = np.ascontiguousarray(np.asarray(matches), dtype=np.int32).reshape(-1)
        assert len(m) == nc1, "one match per cluster of scene 1"
        out = np.zeros((max(nc1, 1), 2), dtype=np.int32)
        st = self._before(points1, points2, a[6], b[6])
        if a[5] == MEM_DEVICE and st is None:
            import torch
            torch.cuda.current_stream((points1 if a[2] else points2).device).synchronize()
        status = LIB.pcc_match_colour_elements(self._h, a[0], a[1], offs[0].ctypes.data, nc1, b[0], b[1], offs[1].ctypes.data, nc2, a[3], a[4], a[5],
                                               m.ctypes.data if nc1 else None, int(min_points), np.float32(distance), np.float32(point_colour),
                                               np.float32(region_colour), int(min_size), 2**31 - 1 if max_size is None else int(max_size),
                                               int(nn), int(region_nn), out.ctypes.data)
        self._after(st)
        _check(status)
        return out[:nc1]

    def region_growing(self, normals, k: int = 100, smoothness: float = 3.0 / 180.0 * np.pi,
                       curvature_threshold: float = 1.0, min_size: int = 50, max_size: int = 1000000):
        """pcl::RegionGrowing::extract over the index's own points: (labels, n_clusters)."""
        ncl = C.c_int32(0)
        if _is_torch(normals) and normals.is_cuda:
            import torch
            assert normals.dtype == torch.float32 and normals.is_contiguous()
            labels = torch.empty(self.n_original, dtype=torch.int32, device=normals.device)
            st = self._before(normals)
            if st is None:
                torch.cuda.current_stream(normals.device).synchronize()
            _check(LIB.pcc_region_growing(self._h, normals.data_ptr(), MEM_DEVICE, k, np.float32(smoothness),
                                          np.float32(curvature_threshold), min_size, max_size, labels.data_ptr(),
                                          C.byref(ncl)))
            self._after(st)
            return labels, ncl.value
        nm = np.ascontiguousarray(normals, dtype=np.float32)
        assert nm.shape == (self.n_original, 4)
        labels = np.empty(self.n_original, dtype=np.int32)
        _check(LIB.pcc_region_growing(self._h, nm.ctypes.data, MEM_HOST, k, np.float32(smoothness),
                                      np.float32(curvature_threshold), min_size, max_size, labels.ctypes.data,
                                      C.byref(ncl)))
        return labels, ncl.value

    def region_growing_rgb(self, rgb, distance: float = 10.0, point_colour: float = 6.0, region_colour: float = 5.0,
                           min_size: int = 200, max_size: int = 2**31 - 1, nn: int = 30, region_nn: int = 100, device=None):
        """pcc_region_growing_rgb: pcl::RegionGrowingRGB::extract as the reference's color_growing_segmentation sets it up
        (src/segmentation.cpp:161-216) over the index's own points, rows and growing on the device: (labels, n_clusters).
        rgb: one colour per point in any of rift_descriptors' three forms (a CUDA tensor gives CUDA labels).
        device: a torch cuda device to get the labels as a device tensor whatever memory `rgb` lives in."""
        n = self.n_original
        assert len(rgb) == n, "one colour per point of the indexed cloud"
        if device is not None and not (_is_torch(rgb) and rgb.is_cuda):
            import torch
            if not _is_torch(rgb):
                rgb = np.ascontiguousarray(rgb)
                rgb = torch.from_numpy(rgb.view(np.int32) if rgb.dtype == np.uint32 else rgb)
            rgb = rgb.to(device)
        words, ptr, stride, mem = _colour_words(rgb)
        labels, pl = _out(words, (max(n, 1),), np.int32)
        ncl = C.c_int32(0)
        st = self._before(words, labels)
        if mem == MEM_DEVICE and st is None:
            import torch
            torch.cuda.current_stream(words.device).synchronize()
        _check(LIB.pcc_region_growing_rgb(self._h, ptr, stride, mem, np.float32(distance), np.float32(point_colour),
                                          np.float32(region_colour), int(min_size), int(max_size), int(nn), int(region_nn), pl,
                                          C.byref(ncl)))
        self._after(st)
        return labels[:n], ncl.value

    def region_growing_rgb_batch(self, clouds, rgbs=None, distance: float = 10.0, point_colour: float = 6.0, region_colour: float = 5.0,
                                 min_size: int = 200, max_size: int = 2**31 - 1, nn: int = 30, region_nn: int = 100):
        """pcc_region_growing_rgb_batch with this handle as the context: colour region growing of every cloud in one call (the
        reference's two color_growing_segmentation calls per accepted match, src/comparator.cpp:1456-1495).  clouds[c] /
        rgbs[c]: host arrays as rift_descriptors_batch takes them.  Returns one (labels (n,) int32, n_clusters) per cloud, each
        what Index(clouds[c]).region_growing_rgb(rgbs[c], ...) returns; a cloud without a finite point gives all -1 and 0.  The
        cloud the handle indexes is neither read nor changed."""
        b = _cloud_batch(clouds, rgbs, "pcc_region_growing_rgb_batch")
        n = b.n
        off = np.concatenate([[0], np.cumsum(b.counts[:n], dtype=np.int64)]).astype(np.int64)
        labels = np.empty(max(int(off[n]), 1), dtype=np.int32)
        ncl = np.zeros(max(n, 1), dtype=np.int32)
        _check(LIB.pcc_region_growing_rgb_batch(self._h, n, b.pts, b.counts, b.stride, b.rgb, b.rgb_stride, MEM_HOST, np.float32(distance),
                                                np.float32(point_colour), np.float32(region_colour), int(min_size), int(max_size), int(nn),
                                                int(region_nn), labels.ctypes.data, ncl.ctypes.data))
        return [(labels[int(off[c]):int(off[c + 1])].copy(), int(ncl[c])) for c in range(n)]

    def icp_step(self, src, want_corr: bool = True, center=None):
        """correspondences of `src` against the index + the 17 Umeyama sums; center: take the sums about this point
        (every rank of a sharded loop the SAME one) -- needed for small clouds at large coordinates"""
        ptr, n, stride, mem = _points(src)
        sums = (C.c_double * 17)()
        if want_corr:
            idx, pi = _out(src, (n,), np.int32)
            d2, pd = _out(src, (n,), np.float32)
        else:
            idx = d2 = None
            pi = pd = None
        st = self._before(src)
        if center is None:
            _check(LIB.pcc_icp_step(self._h, ptr, n, stride, mem, pi, pd, sums))
        else:
            cc = np.ascontiguousarray(center, dtype=np.float64)
            assert cc.shape == (3,)
            _check(LIB.pcc_icp_step_about(self._h, ptr, n, stride, mem, cc.ctypes.data, pi, pd, sums))
        self._after(st)
        return idx, d2, np.array(list(sums), dtype=np.float64)

    def transform(self, T, src, dst=None):
        ptr, n, stride, mem = _points(src)
        Tm = np.ascontiguousarray(np.asarray(T, dtype=np.float32).reshape(16))
        if dst is None:
            if _is_torch(src):
                import torch
                dst = torch.empty((n, 3), dtype=torch.float32, device=src.device)
            else:
                dst = np.empty((n, 3), dtype=np.float32)
        dptr, dn, dstride, dmem = _points(dst)
        assert dn == n and dmem == mem
        st = self._before(src, dst)
        _check(LIB.pcc_transform(self._h, Tm.ctypes.data_as(C.POINTER(C.c_float)), ptr, n, stride, dptr,
                                 dstride, mem))
        self._after(st)
        return dst

    def icp_align(self, src, max_iter: int = 20, fixed: bool = False):
        ptr, n, stride, mem = _points(src)
        T = (C.c_float * 16)()
        fit = C.c_double(0)
        it = C.c_int(0)
        conv = C.c_int(0)
        self._before(src)  # (the call synchronises the index's stream before it returns)
        _check(LIB.pcc_icp_align(self._h, ptr, n, stride, mem, max_iter, int(fixed), T, C.byref(fit),
                                 C.byref(it), C.byref(conv)))
        return np.array(list(T), dtype=np.float32).reshape(4, 4), fit.value, it.value, bool(conv.value)

    def match_knn(self, des2, threshold: float = 0.05):
        ptr, n, stride, mem = _points(des2)
        out = np.empty(n + 1, dtype=np.int32)
        sz = C.c_int32(0)
        self._before(des2)
        _check(LIB.pcc_match_knn(self._h, ptr, n, stride, mem, np.float32(threshold), out.ctypes.data,
                                 C.byref(sz)))
        return out[:sz.value]

    def match_knn_batch(self, pairs, threshold: float = 0.05, ties=None, dim: int = 3, return_d2: bool = False):
        """pcc_match_knn_batch with this handle as the context: `pairs` is a sequence of (des1, des2) float32 numpy arrays of
        one row stride; returns one int32 array per pair, each what Index(des1).match_knn(des2) returns.  The cloud the
        handle indexes is neither read nor changed.  ties: None = the handle's own tie order, else that order for this call.
        dim: the number of leading floats of a record the search reads, 1 ... 32 (pcc_match_knn_batch_dims; 3 is what the
        single call reads).  return_d2: also the squared distances -- the result is then (indices, d2), two lists of arrays
        of equal shapes (0.0 beside each row's dummy)."""
        pairs = list(pairs)
        n = len(pairs)
        plain = dim == 3 and not return_d2
        args = [(_points(a), _points(b)) if plain else (_records(a, dim), _records(b, dim)) for a, b in pairs]
        strides = {x[2] for ab in args for x in ab} if plain else {x[2] for ab in args for x in ab if x[1] > 1}
        assert len(strides) <= 1, "every descriptor array of a batch must have the same row stride"
        assert all(x[3] == MEM_HOST for ab in args for x in ab), "pcc_match_knn_batch takes host arrays"
        stride = strides.pop() if strides else (12 if plain else 4 * max(int(dim), 1))
        vps, szs = (C.c_void_p * max(n, 1)), (C.c_size_t * max(n, 1))
        d1 = vps(*[a[0] if a[1] else None for a, _ in args])
        d2 = vps(*[b[0] if b[1] else None for _, b in args])
        n1 = szs(*[a[1] for a, _ in args])
        n2 = szs(*[b[1] for _, b in args])
        out = np.empty(sum(b[1] for _, b in args) + n, dtype=np.int32)
        dist = np.empty(len(out), dtype=np.float32) if return_d2 else None
        off = np.zeros(n + 1, dtype=np.uintp)
        own = self._ties
        if ties is not None and ties != own:
            self.set_tie_order(ties)
        try:
            if plain:
                _check(LIB.pcc_match_knn_batch(self._h, n, d1, n1, d2, n2, stride, MEM_HOST, np.float32(threshold),
                                               out.ctypes.data, off.ctypes.data))
            else:
                _check(LIB.pcc_match_knn_batch_dims(self._h, n, d1, n1, d2, n2, stride, int(dim), MEM_HOST, np.float32(threshold),
                                                    out.ctypes.data, dist.ctypes.data if return_d2 else None, off.ctypes.data))
        finally:
            if self._ties != own:
                self.set_tie_order(own)
        rows = [out[int(off[p]):int(off[p + 1])].copy() for p in range(n)]
        if not return_d2:
            return rows
        return rows, [dist[int(off[p]):int(off[p + 1])].copy() for p in range(n)]

    def match_fpfh_batch(self, pairs, threshold: float = 0.25, return_d2: bool = False):
        """pcc_match_fpfh_batch with this handle as the context: the reference's matchFPFH (src/comparator.cpp:877-910) for every
        (des1, des2) pair of (n, >= 33) float32 FPFH descriptor arrays of one row stride at once, on the 33 bins.  The pairs are
        all NumPy arrays (host memory) or all CUDA tensors (device memory, as fpfh_descriptors leaves them on a handle over a
        CUDA tensor); a mixture is a ValueError.  Returns one int32 NumPy array per pair: the dummy 0, then per row of des2 in
        order the index of its nearest row of des1 when the squared distance is < threshold; among rows of des1 at exactly the
        same distance the lowest index.  return_d2: also the squared distances -- the result is then (indices, d2), two lists of
        arrays of equal shapes (0.0 beside each row's dummy).  The cloud the handle indexes is neither read nor changed."""
        pairs = list(pairs)
        n = len(pairs)
        flat = [x for ab in pairs for x in ab]
        on_device = [_is_torch(x) and x.is_cuda for x in flat]
        if any(on_device) and not all(on_device):
            raise ValueError("match_fpfh_batch takes NumPy arrays or CUDA tensors, not both in one call")
        mem = MEM_DEVICE if any(on_device) else MEM_HOST
        for x in flat:
            assert x.ndim == 2 and x.shape[1] >= 33, "FPFH descriptor arrays are (n, >= 33) float32"
        args = [(_points(a), _points(b)) for a, b in pairs]
        assert all(x[3] == mem for ab in args for x in ab), "host descriptor arrays are NumPy arrays"
        strides = {x[2] for ab in args for x in ab if x[1] > 1}
        assert len(strides) <= 1, "every descriptor array of a batch must have the same row stride"
        stride = strides.pop() if strides else 132
        vps, szs = (C.c_void_p * max(n, 1)), (C.c_size_t * max(n, 1))
        d1 = vps(*[a[0] if a[1] else None for a, _ in args])
        d2 = vps(*[b[0] if b[1] else None for _, b in args])
        n1 = szs(*[a[1] for a, _ in args])
        n2 = szs(*[b[1] for _, b in args])
        out = np.empty(sum(b[1] for _, b in args) + n, dtype=np.int32)
        dist = np.empty(len(out), dtype=np.float32) if return_d2 else None
        off = np.zeros(n + 1, dtype=np.uintp)
        st = self._before(*flat) if mem == MEM_DEVICE else None
        _check(LIB.pcc_match_fpfh_batch(self._h, n, d1, n1, d2, n2, stride, mem, np.float32(threshold), out.ctypes.data,
                                        dist.ctypes.data if return_d2 else None, off.ctypes.data))
        self._after(st)
        rows = [out[int(off[p]):int(off[p + 1])].copy() for p in range(n)]
        if not return_d2:
            return rows
        return rows, [dist[int(off[p]):int(off[p + 1])].copy() for p in range(n)]


def match_knn_batch(pairs, threshold: float = 0.05, ties: int = TIES_LOWEST_INDEX, ctx=None, dim: int = 3, return_d2: bool = False):
    """Descriptor matching for every (des1, des2) pair at once (pcc_match_knn_batch; pcc_match_knn_batch_dims for another `dim`
    than 3 or with return_d2).  ctx: an Index that lends its device, stream and scratch (its own cloud and tie order are left
    as they are); None makes a one-point handle for the call."""
    if ctx is not None:
        return ctx.match_knn_batch(pairs, threshold, ties, dim, return_d2)
    with Index(np.zeros((1, 3), np.float32), engine=ENGINE_BRUTE) as own:
        return own.match_knn_batch(pairs, threshold, ties, dim, return_d2)


def rift_descriptors_batch(clouds, rgbs=None, normal_radius: float = 0.03, gradient_radius: float = 0.03, rift_radius: float = 0.05,
                           nr_distance_bins: int = 4, nr_gradient_bins: int = 8, ctx=None):
    """RIFT descriptors of every cloud at once (pcc_rift_descriptors_batch): a list of (histograms, point index) per cloud.
    ctx: an Index that lends its device, stream and scratch (its own cloud is left as it is); None makes a one-point handle
    for the call."""
    if ctx is not None:
        return ctx.rift_descriptors_batch(clouds, rgbs, normal_radius, gradient_radius, rift_radius, nr_distance_bins, nr_gradient_bins)
    with Index(np.zeros((1, 3), np.float32), engine=ENGINE_BRUTE) as own:
        return own.rift_descriptors_batch(clouds, rgbs, normal_radius, gradient_radius, rift_radius, nr_distance_bins, nr_gradient_bins)


def match_vfh(h1, h2, ctx=None):
    """matchVHF for every pair of two arrays of VFH descriptors (pcc_match_vfh): the (n1, n2) float64 distances.
    ctx: an Index that lends its device, stream and scratch (its own cloud is left as it is); None makes a one-point handle
    for the call."""
    if ctx is not None:
        return ctx.match_vfh(h1, h2)
    with Index(np.zeros((1, 3), np.float32), engine=ENGINE_BRUTE) as own:
        return own.match_vfh(h1, h2)


def vfh_descriptors_batch(clouds_or_points, offsets=None, normal_radius: float = 0.03, return_packed: bool = False, ctx=None):
    """VFH descriptors of every cluster at once (pcc_vfh_descriptors_batch): one (308,) descriptor per cluster, an empty
    (0, 308) array for a cluster of fewer than 2 points; or with return_packed (hist (m, 308), offsets).
    See Index.vfh_descriptors_batch.  ctx: any Index; without one a small handle is made for the call."""
    if ctx is not None:
        return ctx.vfh_descriptors_batch(clouds_or_points, offsets, normal_radius, return_packed)
    with Index(np.zeros((1, 3), np.float32), engine=ENGINE_BRUTE) as own:
        return own.vfh_descriptors_batch(clouds_or_points, offsets, normal_radius, return_packed)


def fpfh_descriptors_batch(clouds_or_points, offsets=None, normal_radius: float = 0.03, fpfh_radius: float = 0.05, nr_bins=(11, 11, 11), ctx=None):
    """FPFH descriptors of every cluster at once (pcc_fpfh_descriptors_batch): a list of (histograms, point index) per cluster.
    ctx: an Index that lends its device, stream and scratch (its own cloud is left as it is); None makes a one-point handle
    for the call."""
    if ctx is not None:
        return ctx.fpfh_descriptors_batch(clouds_or_points, offsets, normal_radius, fpfh_radius, nr_bins)
    with Index(np.zeros((1, 3), np.float32), engine=ENGINE_BRUTE) as own:
        return own.fpfh_descriptors_batch(clouds_or_points, offsets, normal_radius, fpfh_radius, nr_bins)


def region_growing_rgb_batch(clouds, rgbs=None, distance: float = 10.0, point_colour: float = 6.0, region_colour: float = 5.0,
                             min_size: int = 200, max_size: int = 2**31 - 1, nn: int = 30, region_nn: int = 100, ctx=None):
    """Colour region growing of every cloud at once (pcc_region_growing_rgb_batch): a list of (labels, n_clusters) per cloud.
    ctx: an Index that lends its device, stream and scratch (its own cloud is left as it is); None makes a one-point handle
    for the call."""
    if ctx is not None:
        return ctx.region_growing_rgb_batch(clouds, rgbs, distance, point_colour, region_colour, min_size, max_size, nn, region_nn)
    with Index(np.zeros((1, 3), np.float32), engine=ENGINE_BRUTE) as own:
        return own.region_growing_rgb_batch(clouds, rgbs, distance, point_colour, region_colour, min_size, max_size, nn, region_nn)
