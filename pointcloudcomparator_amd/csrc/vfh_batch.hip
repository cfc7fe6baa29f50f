// vfh_batch.hip -- the VFH descriptor of EVERY cluster of a segmentation at once (gfx950): pcc_vfh_descriptors_batch.
//
// pcc_match_vfh (vfh.hip) takes two arrays of descriptors and returns all n1 x n2 distances; its producer was set_input +
// pcc_vfh_descriptor once per cluster: an index build, a CSR build with its wait, three kernels on grids of ONE workgroup and a
// copy down, 60 to 200 times a comparison -- the serial centroid chains of each cluster alone on the chip.  Here the clusters of
// a call -- ranges offsets[c] .. offsets[c + 1] of ONE array of records, in host or device memory -- are ONE concatenated cloud
// (point bases[c] + i is point i of cluster c) whose rows hold members of the point's own cluster only (rift_batch.hip's
// exhaustive builder, batch_radius_rows), the plane fit runs once over it, and three kernels follow:
//   k_vfh_batch_centroids  one wave per cluster, all clusters in one launch: vfh_centroid_chains, the body k_vfh_centroids runs
//                          (vfh_device.hpp) -- the chains of different clusters are independent and run side by side;
//   k_vfh_batch_votes      one workgroup per vote item (up to VFH_BATCH_VOTE_POINTS points of ONE cluster): vfh_vote against the
//                          cluster's record, counted in an LDS table and added to the cluster's 263 counters in integers;
//   k_vfh_batch_finish     one workgroup per descriptor: lane b rebuilds bin b from its count, the plain loop of the single call.
// No float atomic anywhere; no point, centroid term or vote of another cluster enters a descriptor.
//
// A cluster of 2 points and more has exactly one descriptor, a smaller one none: the caller's bounds are known on the host
// before anything is launched (vfh_batch_plan.hpp), and every kernel -- and the work handle -- writes a descriptor where it
// stays: the caller's array in device memory, a staging array of the same layout for a host caller, copied down in merged runs.
// Clusters above PCC_OPT_VFH_BATCH_BRUTE_MAX points take set_input + pcc_vfh_descriptor on a work handle kept in ctx, in the
// caller's memory space, straight into their row.
//
// Non-finite points: the single call refuses a cloud that holds one, and so does this call for every cluster of 2 points and
// more.  A host caller's points pass through the staging loop, which refuses before any launch; a device caller's pass through
// the pack kernel, which leaves the lowest such cluster in one word (atomicMin) that travels down beside the CSR's total and is
// read after the wait the CSR build makes anyway.
#include <algorithm>
#include <vector>

#include "entry.hpp"
#include "lane_ops.hpp"
#include "grid_device.hpp"
#include "vfh_math.hpp"
#include "vfh_device.hpp"
#include "cloud_batch.hpp"
#include "vfh_batch_plan.hpp"

namespace pcc {

namespace {

constexpr unsigned int VFH_BATCH_NONE = 0xffffffffu;  // the flag word while no cluster holds a non-finite point

// ---- the pack from device memory (k_fpfh_batch_pack's copy, plus the flag) -----------------------------------------------------
// Point e of the concatenation lies in cluster c = the last one with bases[c] <= e (a cluster off the batch route is empty here
// and never the answer) and is the caller's record src[c] + (e - bases[c]): out[e] = x, y, z, w = bits(e).  V16: the records are
// 16-byte aligned and a multiple of 16 bytes apart: x, y, z in one load; else three scalar loads.  A non-finite point leaves
// its cluster's number in *bad when no lower one is there.
template <bool V16>
__global__ void __launch_bounds__(256)
k_vfh_batch_pack(const unsigned char* __restrict__ pts, size_t stride, const unsigned int* __restrict__ src, const unsigned int* __restrict__ bases,
                 unsigned int n_clusters, unsigned int total, float4* __restrict__ out, unsigned int* __restrict__ bad) {
    for (unsigned int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const unsigned int c = range_of(bases, n_clusters, e);
        const size_t rec = (size_t)src[c] + (e - bases[c]);
        float x, y, z;
        if constexpr (V16) {
            const float4 v = *reinterpret_cast<const float4*>(pts + rec * stride);
            x = v.x; y = v.y; z = v.z;
        } else {
            const float* v = reinterpret_cast<const float*>(pts + rec * stride);
            x = v[0]; y = v[1]; z = v[2];
        }
        if (!finite3(x, y, z)) atomicMin(bad, c);
        out[e] = make_float4(x, y, z, __uint_as_float(e));
    }
}

// ---- the centroids: workgroup g carries the six chains of cluster route[g] over points [bases[c], bases[c + 1]) -----------------
__global__ void __launch_bounds__(64)
k_vfh_batch_centroids(const float4* __restrict__ pts, const float4* __restrict__ normals, const unsigned int* __restrict__ route,
                      const unsigned int* __restrict__ bases, VfhRecord* __restrict__ records) {
    const unsigned int c = route[blockIdx.x];  // (block-uniform: scalar loads)
    const unsigned int first = bases[c], n = bases[c + 1] - first;
    vfh_centroid_chains(pts + first, normals + first, n, records + c);
}

// ---- the votes: one item a workgroup, the table in LDS belongs to the item's cluster --------------------------------------------
// (every bin number is clamped to its range by vfh_math.hpp, so no index leaves the table)
__global__ void __launch_bounds__(256)
k_vfh_batch_votes(const float4* __restrict__ pts, const float4* __restrict__ normals, const VfhVoteItem* __restrict__ items,
                  const VfhRecord* __restrict__ records, unsigned int* __restrict__ counters) {
    __shared__ unsigned int table[VFH_COUNTERS];
    for (unsigned int t = threadIdx.x; t < (unsigned int)VFH_COUNTERS; t += blockDim.x) table[t] = 0u;
    __syncthreads();
    const VfhVoteItem it = items[blockIdx.x];  // (block-uniform)
    const VfhRecord r = records[it.cluster];
    for (unsigned int i = threadIdx.x; i < it.count; i += blockDim.x) {
        const float4 pv = pts[it.first + i], nv = normals[it.first + i];
        const float p[3] = {pv.x, pv.y, pv.z}, nrm[3] = {nv.x, nv.y, nv.z};
        const VfhVote v = vfh_vote(r.centroid, r.normal_centroid, r.d_vp_p, p, nrm);
        if (v.f1 != VFH_NO_VOTE) {
            atomicAdd(&table[v.f1], 1u);
            atomicAdd(&table[VFH_F_BINS + v.f2], 1u);
            atomicAdd(&table[2 * VFH_F_BINS + v.f3], 1u);
        }
        atomicAdd(&table[3 * VFH_F_BINS + v.vp], 1u);
    }
    __syncthreads();
    unsigned int* __restrict__ mine = counters + (size_t)it.cluster * VFH_COUNTERS;
    for (unsigned int t = threadIdx.x; t < (unsigned int)VFH_COUNTERS; t += blockDim.x)
        if (table[t]) atomicAdd(&mine[t], table[t]);
}

// ---- the bins from their counts: workgroup g writes the descriptor of cluster route[g] into row row[c] --------------------------
__global__ void __launch_bounds__(320)
k_vfh_batch_finish(const unsigned int* __restrict__ counters, const unsigned int* __restrict__ route, const unsigned int* __restrict__ bases,
                   const unsigned int* __restrict__ row, float* __restrict__ out_hist) {
    const unsigned int c = route[blockIdx.x];
    const unsigned int n = bases[c + 1] - bases[c];
    const int b = (int)threadIdx.x;
    if (b < VFH_BINS) out_hist[(size_t)row[c] * VFH_BINS + b] = vfh_bin_value(counters + (size_t)c * VFH_COUNTERS, n, b);
}

unsigned int blocks_for(size_t n) { return (unsigned int)std::min<size_t>((n + 255) / 256, 2048); }

// (up: GridDev + the clusters' places, rows, route and vote items + bases + table [+ points]; down: the flag word)
struct VfhBatchScratch : BatchStaging {
    static constexpr ScratchSlot slot = SCRATCH_VFH_BATCH;
    DevBuf offs, keys;          // the CSR at normal_radius: uint32 offsets[n + 1] + the same as int64; u64 keys
    DevBuf normals;             // float4[total] plane fit
    DevBuf records, counters;   // VfhRecord[n_clusters]; uint32[n_clusters][VFH_COUNTERS], zeroed on the stream in every call
    DevBuf flag;                // one word: the lowest cluster with a non-finite point (device callers)
    DevBuf out_hist;            // the descriptors staged for a caller in host memory, laid out like the caller's array
};

struct VfhBatchArgs {
    const unsigned char* pts;
    size_t stride;
    const size_t* offsets;
    size_t n_clusters;
    int mem;
    double normal_radius;
    float* out_hist;
    size_t* out_offsets;
};

int refuse_non_finite(size_t c) {
    set_error("VFH of a cluster with a non-finite point (cluster %zu): the reference strips them when it loads a cloud", c);
    return PCC_ERR_UNSUPPORTED;
}

// The batch route: the clusters of 2 .. limit points staged as one concatenation, the normals, the three kernels.  hist: the
// device array of plan.descriptors() rows the descriptors are written to.  Waits: the CSR's total.
int vfh_batch_brute(pcc_index* ix, const VfhBatchArgs& a, const VfhBatchPlan& plan, float* hist) {
    hipStream_t s = ix->stream;
    VfhBatchScratch* b = scratch<VfhBatchScratch>(ix);
    const size_t n_clusters = a.n_clusters, total = plan.bases[n_clusters];
    const unsigned int nc = (unsigned int)n_clusters;
    const size_t n_route = plan.route.size(), n_votes = plan.votes.size();
    const unsigned char* p0 = a.pts + a.offsets[0] * a.stride;

    // ---- one pinned buffer, one copy: the order's n_valid word, src, row, route, vote items, bases, table -- and from host
    // memory 16 bytes a point ----
    static_assert(sizeof(GridDev) % 16 == 0, "the clusters' places lie directly behind the GridDev");
    const size_t src_at = sizeof(GridDev);
    const size_t row_at = src_at + (n_clusters + 1) * sizeof(uint32_t);
    const size_t route_at = row_at + n_clusters * sizeof(uint32_t);
    const size_t votes_at = align_up(route_at + n_route * sizeof(uint32_t), 16);
    const size_t header = votes_at + n_votes * sizeof(VfhVoteItem);
    const ConcatLayout up(header, 128, n_clusters, plan.items.size(), total);
    const bool host = a.mem == PCC_MEM_HOST;
    const size_t up_bytes = host ? up.rgb_at : up.pts_at;  // (no colour is read: the layout's last part is not used)
    PCC_TRY(b->up.reserve(up_bytes));
    PCC_TRY(b->dev.reserve(up.rgb_at));
    char* u = b->up.as<char>();
    memset(u, 0, up.items_at);
    // (the plane fit reads nothing of the grid but n_valid: every point of the concatenation is taken, in its order)
    reinterpret_cast<GridDev*>(u)->n_valid = (unsigned int)total;
    memcpy(u + src_at, plan.src.data(), (n_clusters + 1) * sizeof(uint32_t));
    memcpy(u + row_at, plan.row.data(), n_clusters * sizeof(uint32_t));
    memcpy(u + route_at, plan.route.data(), n_route * sizeof(uint32_t));
    memcpy(u + votes_at, plan.votes.data(), n_votes * sizeof(VfhVoteItem));
    memcpy(u + up.bases_at, plan.bases.data(), (n_clusters + 1) * sizeof(uint32_t));
    memcpy(u + up.items_at, plan.items.data(), plan.items.size() * sizeof(RiftBatchItem));
    if (host) {
        // the staging loop sees every point of the batch route: a non-finite one refuses the call before any launch
        float* p4 = reinterpret_cast<float*>(u + up.pts_at);
        for (const uint32_t c : plan.route) {
            const unsigned char* src = p0 + (size_t)plan.src[c] * a.stride;
            for (size_t i = 0; i < plan.small_n[c]; ++i) {
                const uint32_t at = plan.bases[c] + (uint32_t)i;
                float v[3];
                memcpy(v, src + i * a.stride, 12);
                if (!finite3(v[0], v[1], v[2])) return refuse_non_finite(c);
                memcpy(p4 + (size_t)at * 4, v, 12);
                memcpy(p4 + (size_t)at * 4 + 3, &at, 4);
            }
        }
    }
    PCC_TRY(b->normals.reserve(total * sizeof(float4)));
    PCC_TRY(b->records.reserve(n_clusters * sizeof(VfhRecord)));
    PCC_TRY(b->counters.reserve(n_clusters * VFH_COUNTERS * sizeof(unsigned int)));
    PCC_TRY(b->flag.reserve(sizeof(unsigned int)));
    PCC_TRY(b->down.reserve(sizeof(unsigned int)));
    PCC_HIP(hipMemcpyAsync(b->dev.p, u, up_bytes, hipMemcpyHostToDevice, s));
    char* d = b->dev.as<char>();
    const GridDev* gd = reinterpret_cast<const GridDev*>(d);
    const unsigned int* d_src = reinterpret_cast<const unsigned int*>(d + src_at);
    const unsigned int* d_row = reinterpret_cast<const unsigned int*>(d + row_at);
    const unsigned int* d_route = reinterpret_cast<const unsigned int*>(d + route_at);
    const VfhVoteItem* d_votes = reinterpret_cast<const VfhVoteItem*>(d + votes_at);
    const unsigned int* d_bases = reinterpret_cast<const unsigned int*>(d + up.bases_at);
    const RiftBatchItem* d_items = reinterpret_cast<const RiftBatchItem*>(d + up.items_at);
    float4* d_pts = reinterpret_cast<float4*>(d + up.pts_at);
    unsigned int* h_flag = b->down.as<unsigned int>();
    *h_flag = VFH_BATCH_NONE;
    if (!host) {
        PCC_HIP(hipMemsetAsync(b->flag.p, 0xff, sizeof(unsigned int), s));
        if (a.stride % 16 == 0 && reinterpret_cast<uintptr_t>(p0) % 16 == 0)
            hipLaunchKernelGGL((k_vfh_batch_pack<true>), dim3(blocks_for(total)), dim3(256), 0, s, p0, a.stride, d_src, d_bases, nc, (unsigned int)total, d_pts,
                               b->flag.as<unsigned int>());
        else
            hipLaunchKernelGGL((k_vfh_batch_pack<false>), dim3(blocks_for(total)), dim3(256), 0, s, p0, a.stride, d_src, d_bases, nc, (unsigned int)total, d_pts,
                               b->flag.as<unsigned int>());
        PCC_HIP(hipGetLastError());
        // (on its way down beside the CSR's total: no wait of its own)
        PCC_HIP(hipMemcpyAsync(h_flag, b->flag.p, sizeof(unsigned int), hipMemcpyDeviceToHost, s));
    }

    // ---- ONE CSR at normal_radius (count, total -- the wait --, scan, fill, sort), then the plane fit over its rows ------------
    const unsigned long long* keys = nullptr;
    const unsigned int* off32 = nullptr;
    PCC_TRY(batch_radius_rows(ix, d_items, (unsigned int)plan.items.size(), d_pts, total, radius2(a.normal_radius), b->offs, b->keys, &keys, &off32));
    if (*h_flag != VFH_BATCH_NONE) return refuse_non_finite(*h_flag);
    const float origin[3] = {0.f, 0.f, 0.f};
    float4* normals = b->normals.as<float4>();
    PCC_TRY(launch_normals_csr(s, d_pts, d_pts, gd, total, keys, off32, origin, normals));

    // ---- the three kernels --------------------------------------------------------------------------------------------------------
    VfhRecord* records = b->records.as<VfhRecord>();
    unsigned int* counters = b->counters.as<unsigned int>();
    PCC_HIP(hipMemsetAsync(counters, 0, n_clusters * VFH_COUNTERS * sizeof(unsigned int), s));
    ev_mark(ix, EV_SORT0);
    hipLaunchKernelGGL(k_vfh_batch_centroids, dim3((unsigned int)n_route), dim3(64), 0, s, (const float4*)d_pts, (const float4*)normals, d_route, d_bases, records);
    PCC_HIP(hipGetLastError());
    ev_mark(ix, EV_SORT1);
    ev_mark(ix, EV_MAIN0);
    hipLaunchKernelGGL(k_vfh_batch_votes, dim3((unsigned int)n_votes), dim3(256), 0, s, (const float4*)d_pts, (const float4*)normals, d_votes,
                       (const VfhRecord*)records, counters);
    PCC_HIP(hipGetLastError());
    ev_mark(ix, EV_MAIN1);
    ev_mark(ix, EV_FB0);
    hipLaunchKernelGGL(k_vfh_batch_finish, dim3((unsigned int)n_route), dim3(320), 0, s, (const unsigned int*)counters, d_route, d_bases, d_row, hist);
    PCC_HIP(hipGetLastError());
    ev_mark(ix, EV_FB1);
    return PCC_OK;
}

int vfh_descriptors_batch(pcc_index* ix, const VfhBatchArgs& a) {
    hipStream_t s = ix->stream;
    const size_t n_clusters = a.n_clusters;
    PCC_TRY(sync_info(ix));  // (a pending mirror of the handle's own grid would overwrite stats[2] later)
    VfhBatchScratch* b = scratch<VfhBatchScratch>(ix);
    const VfhBatchPlan plan = vfh_batch_plan(a.offsets, n_clusters, (size_t)ix->opt.vfh_batch_brute_max);
    const bool host = a.mem == PCC_MEM_HOST;

    // a device caller's rows are written where they stay; a host caller's into a staging array of the same layout
    float* hist = a.out_hist;
    if (!plan.route.empty()) {
        if (host) {
            PCC_TRY(b->out_hist.reserve(plan.descriptors() * VFH_BINS * sizeof(float)));
            hist = b->out_hist.as<float>();
        }
        PCC_TRY(vfh_batch_brute(ix, a, plan, hist));
    }

    // ---- the clusters above the limit: the single call on the work handle, straight into their row --------------------------------
    if (plan.n_large) {
        WorkLease lease;
        PCC_TRY(lease.take(ix, b->work, true));
        pcc_index* w = lease.w;
        for (size_t c = 0; c < n_clusters; ++c) {
            if (!plan.on_work_handle(c)) continue;
            PCC_TRY(pcc_index_set_input(w, a.pts + a.offsets[c] * a.stride, plan.n[c], a.stride, 3, a.mem));
            size_t n_valid = 0;
            PCC_TRY(pcc_index_size(w, &n_valid));
            if (n_valid != plan.n[c]) return refuse_non_finite(c);
            size_t m = 0;
            PCC_TRY(pcc_vfh_descriptor(w, a.mem, a.normal_radius, a.out_hist + plan.out_offsets[c] * VFH_BINS, &m));
        }
    }
    // ---- the staged rows of a host caller, run by run (behind the work handle: a refusal there leaves no copy under way) ---------
    if (host && !plan.copies.empty()) {
        for (const VfhBatchCopy& cp : plan.copies)
            PCC_TRY(copy_out(ix, a.out_hist + cp.row * VFH_BINS, hist + cp.row * VFH_BINS, cp.count * VFH_BINS * sizeof(float), a.mem));
        PCC_HIP(hipStreamSynchronize(s));  // the rows
    }
    ix->stats[0] = plan.n_brute;
    ix->stats[1] = plan.n_large;
    ix->stats[2] = plan.descriptors();
    ix->stats_pending = false;
    for (size_t c = 0; c <= n_clusters; ++c) a.out_offsets[c] = plan.out_offsets[c];
    return PCC_OK;
}

}  // namespace

}  // namespace pcc

extern "C" {

int pcc_vfh_descriptors_batch(pcc_index* ctx, const void* pts, size_t stride_bytes, const size_t* offsets, size_t n_clusters, int mem,
                              double normal_radius, float* out_histograms, size_t* out_offsets) {
    using namespace pcc;
    // the arguments first: all of it host arithmetic, refused before the handle or any device is looked at
    // 1. the memory space
    PCC_TRY(check_mem(mem));
    // 2. null arrays (the clusters' arrays may be null while no cluster holds a point)
    if (!offsets || !out_offsets) { set_error("null argument"); return PCC_ERR_INVALID; }
    const bool any_points = n_clusters && offsets[n_clusters] != offsets[0];
    if (any_points && (!pts || !out_histograms)) { set_error("null argument"); return PCC_ERR_INVALID; }
    // 3. the stride and the alignment
    PCC_TRY(check_points(nullptr, 0, stride_bytes, mem));  // (the stride alone)
    if (reinterpret_cast<uintptr_t>(pts) % 4 || reinterpret_cast<uintptr_t>(out_histograms) % 4) {
        set_error("points and descriptors must be 4-byte aligned");
        return PCC_ERR_INVALID;
    }
    // 4. the offsets
    size_t bad = 0;
    switch (fpfh_batch_check_offsets(offsets, n_clusters, &bad)) {
        case FB_OFFSETS_DECREASE: set_error("offsets must not decrease (cluster %zu)", bad); return PCC_ERR_INVALID;
        case FB_OFFSETS_TOO_MANY: set_error("more than 2^31 - 1 points in one batch"); return PCC_ERR_UNSUPPORTED;
        default: break;
    }
    // 5. the radius
    if (!(normal_radius > 0) || !std::isfinite(normal_radius)) { set_error("bad radius"); return PCC_ERR_INVALID; }
    if (n_clusters == 0) { out_offsets[0] = 0; return PCC_OK; }  // (no device is touched: not even the handle's)
    // 6. the handle
    PCC_ENTER(ctx);
    ev_next(ctx);
    ev_mark(ctx, EV_CALL0);
    const VfhBatchArgs a{static_cast<const unsigned char*>(pts), stride_bytes, offsets, n_clusters, mem, normal_radius, out_histograms, out_offsets};
    const int st = vfh_descriptors_batch(ctx, a);
    ev_mark(ctx, EV_CALL1);
    return st;
}
}  // extern "C"
