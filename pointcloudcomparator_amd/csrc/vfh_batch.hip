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
// the pack kernel, which leaves the lowest such cluster in one word that travels down beside the CSR's total and is read after
// the wait the CSR build makes anyway (stage_ranges with its flag on: range_batch.hip).
//
// Argument checks 1 - 4, routes, upload, pack and the loop over the work handle are the range-batch calls' (DESIGN.md 4.16:
// entry.hpp, range_batch_plan.hpp); this file owns the plan's extras (vfh_batch_plan.hpp), the three kernels and the refusal.
#include <vector>

#include "entry.hpp"
#include "lane_ops.hpp"
#include "grid_device.hpp"
#include "vfh_math.hpp"
#include "vfh_device.hpp"
#include "vfh_batch_plan.hpp"

namespace pcc {

namespace {

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

// (up: RangeUpload, its extra part the rows, route and vote items -- VfhUploadExtra; down: the flag word; the CSR: at normal_radius)
struct VfhBatchScratch : RangeStaging {
    static constexpr ScratchSlot slot = SCRATCH_VFH_BATCH;
    DevBuf normals;             // float4[total] plane fit
    DevBuf records, counters;   // VfhRecord[n_clusters]; uint32[n_clusters][VFH_COUNTERS], zeroed on the stream in every call
    DevBuf out_hist;            // the descriptors staged for a caller in host memory, laid out like the caller's array
};

struct VfhBatchArgs {
    ClusterRanges ranges;
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
    const size_t n_clusters = a.ranges.n_clusters, total = plan.total();
    const size_t n_route = plan.route.size(), n_votes = plan.votes.size();

    // ---- the batch route on the device: a host caller's non-finite point refuses here, a device caller's behind the CSR's wait ----
    const VfhUploadExtra extra(plan, RangeUpload::extra_start(n_clusters));
    RangeStaged st;
    PCC_TRY(stage_ranges(ix, *b, a.ranges, plan, extra.bytes, [&](char* e) { extra.fill(e, plan); }, true, &st));
    if (st.host_bad != RANGE_FLAG_NONE) return refuse_non_finite(st.host_bad);
    const unsigned int *d_row = extra.row(st.d_extra), *d_route = extra.route(st.d_extra), *d_bases = st.d_bases;
    const float4* d_pts = st.d_pts;
    PCC_TRY(b->normals.reserve(total * sizeof(float4)));
    PCC_TRY(b->records.reserve(n_clusters * sizeof(VfhRecord)));
    PCC_TRY(b->counters.reserve(n_clusters * VFH_COUNTERS * sizeof(unsigned int)));

    // ---- ONE CSR at normal_radius (count, total -- the wait --, scan, fill, sort), then the plane fit over its rows ------------
    const unsigned long long* keys = nullptr;
    const unsigned int* off32 = nullptr;
    PCC_TRY(b->rows(ix, st, a.normal_radius, &keys, &off32));
    if (*st.h_flag != RANGE_FLAG_NONE) return refuse_non_finite(*st.h_flag);
    const float origin[3] = {0.f, 0.f, 0.f};
    float4* normals = b->normals.as<float4>();
    PCC_TRY(launch_normals_csr(s, d_pts, d_pts, st.gd, total, keys, off32, origin, normals));

    // ---- the three kernels --------------------------------------------------------------------------------------------------------
    VfhRecord* records = b->records.as<VfhRecord>();
    unsigned int* counters = b->counters.as<unsigned int>();
    PCC_HIP(hipMemsetAsync(counters, 0, n_clusters * VFH_COUNTERS * sizeof(unsigned int), s));
    ev_mark(ix, EV_SORT0);
    hipLaunchKernelGGL(k_vfh_batch_centroids, dim3((unsigned int)n_route), dim3(64), 0, s, d_pts, (const float4*)normals, d_route, d_bases, records);
    PCC_HIP(hipGetLastError());
    ev_mark(ix, EV_SORT1);
    ev_mark(ix, EV_MAIN0);
    hipLaunchKernelGGL(k_vfh_batch_votes, dim3((unsigned int)n_votes), dim3(256), 0, s, d_pts, (const float4*)normals, extra.votes(st.d_extra),
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
    const ClusterRanges& r = a.ranges;
    const size_t n_clusters = r.n_clusters;
    PCC_TRY(sync_info(ix));  // (a pending mirror of the handle's own grid would overwrite stats[2] later)
    VfhBatchScratch* b = scratch<VfhBatchScratch>(ix);
    const VfhBatchPlan plan = vfh_batch_plan(r.offsets, n_clusters, (size_t)ix->opt.vfh_batch_brute_max);
    const bool host = r.mem == PCC_MEM_HOST;

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
    PCC_TRY(for_each_on_work_handle(ix, b->work, r, plan, [&](pcc_index* w, size_t c, size_t n_valid) -> int {
        if (n_valid != plan.n[c]) return refuse_non_finite(c);
        size_t m = 0;
        return pcc_vfh_descriptor(w, r.mem, a.normal_radius, a.out_hist + plan.out_offsets[c] * VFH_BINS, &m);
    }));
    // ---- the staged rows of a host caller, run by run (behind the work handle: a refusal there leaves no copy under way) ---------
    if (host && !plan.copies.empty()) {
        for (const VfhBatchCopy& cp : plan.copies)
            PCC_TRY(copy_out(ix, a.out_hist + cp.row * VFH_BINS, hist + cp.row * VFH_BINS, cp.count * VFH_BINS * sizeof(float), r.mem));
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
    // 1 - 4. the memory space, null arrays, the stride and the alignment, the offsets
    const ClusterRanges ranges{static_cast<const unsigned char*>(pts), stride_bytes, offsets, n_clusters, mem};
    PCC_TRY(check_range_batch(ranges, out_offsets, {out_histograms}));
    // 5. the radius
    if (!(normal_radius > 0) || !std::isfinite(normal_radius)) { set_error("bad radius"); return PCC_ERR_INVALID; }
    if (n_clusters == 0) { out_offsets[0] = 0; return PCC_OK; }  // (no device is touched: not even the handle's)
    // 6. the handle
    PCC_ENTER(ctx);
    ev_next(ctx);
    ev_mark(ctx, EV_CALL0);
    const VfhBatchArgs a{ranges, normal_radius, out_histograms, out_offsets};
    const int st = vfh_descriptors_batch(ctx, a);
    ev_mark(ctx, EV_CALL1);
    return st;
}
}  // extern "C"
