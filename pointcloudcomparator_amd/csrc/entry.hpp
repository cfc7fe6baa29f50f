// entry.hpp -- the scaffold of a C-ABI entry point, included by every translation unit that defines one: the call prologue
// (PCC_ENTER), the staging of caller arrays that are not point clouds (stage_in, Out, finish), the counters and cluster offsets
// of the calls that work through a comparison's clusters (the offsets' arithmetic: range_batch_plan.hpp), and the batch calls'
// WorkLease and check_cloud_batch, and the scaffold of the batch calls over ranges of one array (range_batch.hip).
#pragma once
#include <initializer_list>

#include "pcc_internal.hpp"
#include "range_batch_plan.hpp"

namespace pcc {

// a handle's mutex for a scope: bare for the one caller that is no call on the handle (pcc_index_clone_to_devices and its source)
using HandleLock = std::lock_guard<std::mutex>;

// The prologue of every call on a handle: its lock, its device, entered() -- in this order.  status is PCC_ERR_DEVICE (message set,
// entered() not called) when the device cannot be selected.  PCC_ENTER returns it; a collective call cannot return before its
// peers and folds it into its status exchange instead.
struct Entry {
    HandleLock lock;
    DeviceGuard guard;
    int status = PCC_OK;
    explicit Entry(pcc_index* ix) : lock(ix->mu), guard(ix->device) {
        if (!guard.ok) { set_error("hipSetDevice(%d) failed", ix->device); status = PCC_ERR_DEVICE; return; }
        entered(ix);
    }
};
#define PCC_ENTER(ix)                                                         \
    if (!(ix)) { pcc::set_error("null index"); return PCC_ERR_INVALID; }      \
    pcc::Entry _entry(ix);                                                    \
    if (_entry.status != PCC_OK) return _entry.status;
// entry points that put nothing on the stream leave "the build was the last thing enqueued" as they found it
#define PCC_NOTHING_ENQUEUED(ix) (ix)->build_fresh = (ix)->after_build

// the searches beyond k = 1 need the cell grid whatever engine k = 1 uses (api.hip)
int ensure_grid(pcc_index* ix);
// radiusSearch(pt, double radius): r2 = float(radius*radius) evaluated in double
inline float radius2(double radius) { return (float)(radius * radius); }

// ---- caller arrays that are not point clouds (PCC_MEM_HOST or PCC_MEM_DEVICE) -----------------------------------------------
// An input on the device: the caller's own array, or for host memory a copy in `buf`.
template <class T>
int stage_in(pcc_index* ix, const T* user, size_t count, int mem, DevBuf& buf, const T** dev) {
    *dev = user;
    if (mem != PCC_MEM_HOST) return PCC_OK;
    PCC_TRY(buf.reserve(count * sizeof(T)));
    PCC_HIP(hipMemcpyAsync(buf.p, user, count * sizeof(T), hipMemcpyHostToDevice, ix->stream));
    *dev = buf.as<T>();
    return PCC_OK;
}

// A radius fill's row offsets (nq + 1 of them) on the device, and their total offsets[nq] on the host.
inline int stage_offsets(pcc_index* ix, const int64_t* offsets, size_t nq, int mem, const int64_t** doff, int64_t* total) {
    PCC_TRY(stage_in(ix, offsets, nq + 1, mem, ix->scratch_d, doff));
    if (mem == PCC_MEM_HOST) {
        *total = offsets[nq];
    } else {
        PCC_HIP(hipMemcpyAsync(total, offsets + nq, sizeof(int64_t), hipMemcpyDeviceToHost, ix->stream));
        PCC_HIP(hipStreamSynchronize(ix->stream));
    }
    if (*total < 0) { set_error("negative total"); return PCC_ERR_INVALID; }
    return PCC_OK;
}

// A result array: the kernels write `dev`, which is the caller's own array in device memory and `buf` in host memory (nullptr
// when the caller passed none).  finish() hands the results of a call over.
template <class T>
struct Out {
    T* user = nullptr;
    size_t count = 0;
    T* dev = nullptr;
    int stage(T* u, size_t n, int mem, DevBuf& buf) {
        user = dev = u;
        count = n;
        if (mem != PCC_MEM_HOST) return PCC_OK;
        PCC_TRY(buf.reserve(count * sizeof(T)));
        if (user) dev = buf.as<T>();
        return PCC_OK;
    }
};

// one result into the caller's host array: large pageable arrays through the host pipe (api.hip, host_pipe.hpp), else one copy
int deliver(pcc_index* ix, const void* dev, void* user, size_t bytes);
// host memory: every result in turn, then one wait.  Device memory: nothing to do.
template <class... T>
int finish(pcc_index* ix, int mem, const Out<T>&... outs) {
    if (mem != PCC_MEM_HOST) return PCC_OK;
    int st = PCC_OK;
    (void)(... && ((st = deliver(ix, outs.dev, outs.user, outs.count * sizeof(T))) == PCC_OK));  // (up to the first failure)
    PCC_TRY(st);
    PCC_HIP(hipStreamSynchronize(ix->stream));
    return PCC_OK;
}

// A result the kernels left in a buffer of the library's, into the caller's array in either memory space: one plain copy, never
// the host pipe, for the few calls whose results do not go through Out.  The caller waits.
inline int copy_out(pcc_index* ix, void* user, const void* dev, size_t bytes, int mem) {
    PCC_HIP(hipMemcpyAsync(user, dev, bytes, mem == PCC_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ix->stream));
    return PCC_OK;
}

// A call that has written its own counters into ix->stats[0 ... 4]: nothing of an earlier search is still on its way into
// them, and [5] and [6] are what the call says (they travel in the two tie words).
inline void own_counters(pcc_index* ix, uint64_t ties_flagged) {
    ix->stats_pending = false;
    ix->ties_pending = false;
    ix->ties_flagged = ties_flagged;
    ix->ties_changed = 0;
}

// The cluster offsets of one or two scenes (offsets[c] .. offsets[c + 1]: the records of cluster c; nothing is read of a scene
// without clusters).  Every scene's "must not decrease" comes before any scene's size: fewer than 2^31 clusters and records a
// scene, `what` naming the records.  The arithmetic is range_batch_plan.hpp's (check_scene_offsets); the messages are here.
inline int check_cluster_offsets(std::initializer_list<ClusterOffsets> scenes, const char* what) {
    int side = 0;
    size_t bad = 0;
    switch (check_scene_offsets(scenes, &side, &bad)) {
        case RANGE_OFFSETS_DECREASE:
            if (scenes.size() > 1) set_error("offsets must not decrease (scene %d, cluster %zu)", side, bad);
            else set_error("offsets must not decrease (cluster %zu)", bad);
            return PCC_ERR_INVALID;
        case RANGE_OFFSETS_TOO_MANY: set_error("more than 2^31 - 1 %s", what); return PCC_ERR_UNSUPPORTED;
        default: return PCC_OK;
    }
}

// ---- the batch calls ------------------------------------------------------------------------------------------
// A work handle for a scope: made in `slot` at the first use, its launches join the caller's queue (under the caller's options
// when with_options), and it has its own stream back at the end.
struct WorkLease {
    pcc_index* w = nullptr;
    int take(pcc_index* ix, WorkHandle& slot, bool with_options) {
        if (!slot.ix) PCC_TRY(make_handle(ix->device, PCC_ENGINE_GRID, &slot.ix));
        w = slot.ix;
        w->stream = ix->stream;
        if (with_options) w->opt = ix->opt;
        return PCC_OK;
    }
    ~WorkLease() { if (w) w->stream = w->own_stream; }
};

// The argument checks the batch entry points share, all of it host arithmetic: check_cloud_batch (the memory space and the
// stride) first; then the call's own checks of its outputs, arrays and parameters, whose order and statuses differ between the
// calls; then check_batch_clouds (every cloud; pts, n and rgb are there by then).
inline int check_cloud_batch(const char* fn_name, const CloudBatch& b, int mem) {
    PCC_TRY(check_mem(mem));
    if (mem != PCC_MEM_HOST) { set_error("%s takes host arrays only (PCC_MEM_HOST)", fn_name); return PCC_ERR_UNSUPPORTED; }
    return check_points(nullptr, 0, b.stride, mem);  // (the stride alone)
}
inline int check_batch_clouds(const CloudBatch& b, int mem) {
    size_t total = 0;
    for (size_t c = 0; c < b.n_clouds; ++c) {
        PCC_TRY(check_points(b.pts[c], b.n[c], b.stride, mem));
        if (b.n[c] && !b.rgb[c]) { set_error("null colour pointer"); return PCC_ERR_INVALID; }
        if (b.n[c] && (reinterpret_cast<uintptr_t>(b.rgb[c]) % 4 || reinterpret_cast<uintptr_t>(b.pts[c]) % 4)) {
            set_error("points and colour words must be 4-byte aligned, the colour stride %zu a multiple of 4 and >= 4", b.rgb_stride);
            return PCC_ERR_INVALID;
        }
        total += b.n[c];
        if (total >= (1ull << 31)) { set_error("more than 2^31 - 1 points in one batch"); return PCC_ERR_UNSUPPORTED; }
    }
    return PCC_OK;
}

// ---- the batch calls over ranges of ONE array of records (range_batch.hip; the plain-C++ half -- offsets, routes,
// upload layout, host pack -- is range_batch_plan.hpp) ---------------------------------------------------------------------------
// the argument checks 1 - 4 of such an entry point (`outs`: its output arrays), in front of its own parameters and PCC_ENTER
int check_range_batch(const ClusterRanges& r, const size_t* out_offsets, std::initializer_list<const void*> outs);

// what stage_ranges left on the device (valid until the staging buffers are used again)
constexpr unsigned int RANGE_FLAG_NONE = 0xffffffffu;  // no cluster holds a non-finite point
struct RangeStaged {
    const GridDev* gd;  // nothing but n_valid = total is set: every point of the concatenation is taken, in its order
    const unsigned int *d_src, *d_bases;
    const RiftBatchItem* d_items;
    unsigned int n_items;
    float4* d_pts;  // the concatenation, w = bits(index)
    size_t total;
    const char* d_extra;  // the call's own part of the upload
    // flag_non_finite only: the lowest cluster with a non-finite point on the batch route.  host_bad: of a HOST caller -- nothing
    // was uploaded or launched then; *h_flag (pinned): of a DEVICE caller, on its way down: read it after the next wait.
    unsigned int host_bad;
    const unsigned int* h_flag;
};
// what a range-batch call keeps between calls beside its stages' buffers (up: RangeUpload; down: the call's, and the flag word)
struct RangeStaging : BatchStaging {
    DevBuf offs, keys;  // the CSR of the radius in use: uint32 offsets[total + 1] + the same as int64; u64 keys
    DevBuf flag;        // one word: the lowest cluster with a non-finite point (device callers)
    // count, total (the one wait), scan, fill, sort: batch_radius_rows over a staged concatenation
    int rows(pcc_index* ix, const RangeStaged& st, double radius, const unsigned long long** keys_out, const unsigned int** offsets_out) {
        return batch_radius_rows(ix, st.d_items, st.n_items, st.d_pts, st.total, radius2(radius), offs, keys, keys_out, offsets_out);
    }
};

// The batch route of a call on the device: one pinned buffer (RangeUpload: the tables, the call's extra part -- extra_bytes of
// it, written by fill_extra(at) --, a host caller's points), one copy; a device caller's points through k_range_pack.  No wait.
int stage_ranges(pcc_index* ix, RangeStaging& b, const ClusterRanges& r, const RangeBatchPlan& plan, size_t extra_bytes,
                 const std::function<void(char*)>& fill_extra, bool flag_non_finite, RangeStaged* staged);

// The clusters above the limit, in cluster order, on the work handle (leased once, in the caller's memory space): set_input, the
// count of finite points, then fn(w, c, n_valid) -- the single call, straight into the cluster's place.  The first failure ends it.
template <class Fn>
int for_each_on_work_handle(pcc_index* ix, WorkHandle& work, const ClusterRanges& r, const RangeBatchPlan& plan, Fn fn) {
    if (!plan.n_large) return PCC_OK;
    WorkLease lease;
    PCC_TRY(lease.take(ix, work, true));
    for (size_t c = 0; c < r.n_clusters; ++c) {
        if (!plan.on_work_handle(c)) continue;
        PCC_TRY(pcc_index_set_input(lease.w, r.cluster(c), plan.n[c], r.stride, 3, r.mem));
        size_t n_valid = 0;
        PCC_TRY(pcc_index_size(lease.w, &n_valid));
        PCC_TRY(fn(lease.w, c, n_valid));
    }
    return PCC_OK;
}

}  // namespace pcc
