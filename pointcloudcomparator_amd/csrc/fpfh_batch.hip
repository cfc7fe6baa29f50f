// fpfh_batch.hip -- the FPFH descriptor pipeline for EVERY cluster of a segmentation at once (gfx950): pcc_fpfh_descriptors_batch.
//
// pcc_match_fpfh_batch (match_fpfh.hip) matches every pair of descriptor arrays of a comparison at once, from device memory;
// its producer was set_input + pcc_fpfh_descriptors once per cluster: two CSR builds with a wait each, plus the count.  Here the
// clusters of a call -- ranges offsets[c] .. offsets[c + 1] of ONE array of records, in host or device memory -- are ONE
// concatenated cloud (point bases[c] + i is point i of cluster c) whose rows hold members of the point's own cluster only
// (rift_batch.hip's exhaustive builder, batch_radius_rows), and the four stages of fpfh.hip run once over it (fpfh_stages).
//
// One CSR when normal_radius <= fpfh_radius (the reference's 0.03 / 0.05).  A sorted row is ascending in (d2, index), and both
// radii test the same float d2 against float(radius^2): the row at normal_radius is exactly the prefix of the row at fpfh_radius
// whose keys have d2 < float(normal_radius^2).  Only the CSR at fpfh_radius is built; k_fpfh_batch_normals walks each row while
// the key's distance word is below the smaller r2 and fits the plane as k_normals_csr does: the same nine sums in the same
// order.  That halves the row building, sorting and CSR waits of a call.  With normal_radius > fpfh_radius two CSRs are built and
// launch_normals_csr fits the planes, as in the single call.
//
// processFPFH removes nothing after the normals, and the positions of cloud2's points are known before the descriptors are: the
// weighting kernel writes every descriptor where it belongs in the CALLER's array in device memory (a staging buffer for a host
// caller) -- there is no intermediate descriptor buffer.  launch_batch_finish (rift_batch.hip) turns the scan into the slice
// bounds and takes every cluster's base off its point indices.
//
// Clusters above PCC_OPT_FPFH_BATCH_BRUTE_MAX points take set_input + pcc_fpfh_descriptors on a work handle kept in ctx, in the
// caller's memory space, straight into their place in the caller's arrays; the batch route's rows are then written to a buffer
// of the library's and copied to their places run by run (fpfh_batch_plan.hpp: the copy list).
//
// Argument checks 1 - 4, routes, upload, pack and the loop over the work handle are the range-batch calls' (DESIGN.md 4.16:
// entry.hpp, range_batch_plan.hpp); this file owns the prefix plane fit, the choice of one or two CSRs, and the splice.
#include <vector>

#include "entry.hpp"
#include "plane_fit.hpp"
#include "fpfh_math.hpp"
#include "fpfh_batch_plan.hpp"

namespace pcc {

namespace {

// ---- the plane fit over the prefix of the rows at fpfh_radius ----------------------------------------------------------------
// One lane per row, rows in concatenation order: the sums are one dependent chain per row -- their order is part of the result.
// The row is walked while the key's distance word is below r2 (the rows are ascending: nothing closer follows); the nine sums,
// the covariance, the eigenvector and the flip towards the origin are k_normals_csr's; fewer than 3 entries: NaN.
__global__ void __launch_bounds__(256)
k_fpfh_batch_normals(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ offsets, const float4* __restrict__ pts,
                     unsigned int n, float r2, float4* __restrict__ out) {
    const float qnan = __uint_as_float(0x7fc00000u);
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const unsigned int beg = offsets[i], end = offsets[i + 1];
        float acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        unsigned int cnt = 0;
        for (unsigned int j = beg; j < end; ++j) {
            const unsigned long long key = keys[j];
            const unsigned int q = (unsigned int)key;
            if (!(__uint_as_float((unsigned int)(key >> 32)) < r2) || q >= n) break;  // (q < n always: the builder wrote it)
            const float4 p = pts[q];
            acc[0] += p.x * p.x; acc[1] += p.x * p.y; acc[2] += p.x * p.z;
            acc[3] += p.y * p.y; acc[4] += p.y * p.z; acc[5] += p.z * p.z;
            acc[6] += p.x; acc[7] += p.y; acc[8] += p.z;
            ++cnt;
        }
        if (cnt < 3) { out[i] = make_float4(qnan, qnan, qnan, qnan); continue; }
        float cov[9], nrm[3], curv;
        covariance_from_sums(acc, cnt, cov);
        plane_from_covariance(cov, nrm, &curv);
        float nx = nrm[0], ny = nrm[1], nz = nrm[2];
        const float4 p = pts[i];
        const float dx = 0.f - p.x, dy = 0.f - p.y, dz = 0.f - p.z;
        const float cos_theta = dx * nx + dy * ny + dz * nz;
        if (cos_theta < 0) { nx *= -1; ny *= -1; nz *= -1; }
        out[i] = make_float4(nx, ny, nz, curv);
    }
}

// (up: RangeUpload without a part of its own; down: the slice bounds)
struct FpfhBatchScratch : RangeStaging {
    static constexpr ScratchSlot slot = SCRATCH_FPFH_BATCH;
    DevBuf slice;                // uint32[n_clusters + 1]
    DevBuf out_hist, out_index;  // the batch route's rows where the stages cannot write into the caller's arrays
};

struct FpfhBatchArgs {
    ClusterRanges ranges;
    double normal_radius, fpfh_radius;
    float* out_hist;
    int32_t* out_index;
    size_t* out_offsets;
};

// The batch route: the clusters up to the limit staged as one concatenation (stage_ranges: raw coordinates -- the non-finite
// points have empty rows, no normal, and leave with the points outside cloud2), the stages over it, the finish.  hist / index:
// device arrays of plan.total() rows the descriptors are written to.  *h_slice: the slice bounds on the host (valid until the
// scratch's `down` is used again).  Waits: one per CSR, one for the slice bounds.
int fpfh_batch_brute(pcc_index* ix, const FpfhBatchArgs& a, const RangeBatchPlan& plan, float* hist, int32_t* index, unsigned int* n_csr,
                     const unsigned int** h_slice) {
    hipStream_t s = ix->stream;
    FpfhBatchScratch* b = scratch<FpfhBatchScratch>(ix);
    const size_t n_clusters = a.ranges.n_clusters, total = plan.total();
    RangeStaged st;
    PCC_TRY(stage_ranges(ix, *b, a.ranges, plan, 0, nullptr, false, &st));

    // ---- the CSR at a radius: count, total (the wait), scan, fill, sort (batch_radius_rows) ----------------------------------
    *n_csr = 0;
    const RiftRows rows = [&](double radius, const unsigned long long** keys_out, const unsigned int** offsets_out) -> int {
        ++*n_csr;
        return b->rows(ix, st, radius, keys_out, offsets_out);
    };
    // normal_radius <= fpfh_radius: the plane fit over the prefix of the ONE CSR
    const FpfhNormals prefix = [&](float4* normals, const unsigned long long** keys_out, const unsigned int** offsets_out) -> int {
        PCC_TRY(rows(a.fpfh_radius, keys_out, offsets_out));
        PCC_HIP(hipMemsetAsync(normals, 0xff, total * sizeof(float4), s));
        hipLaunchKernelGGL(k_fpfh_batch_normals, dim3(blocks_for(total)), dim3(256), 0, s, *keys_out, *offsets_out, (const float4*)st.d_pts,
                           (unsigned int)total, radius2(a.normal_radius), normals);
        PCC_HIP(hipGetLastError());
        return PCC_OK;
    };
    const bool one_csr = a.normal_radius <= a.fpfh_radius;
    const unsigned int* d_pos = nullptr;
    PCC_TRY(fpfh_stages(ix, st.d_pts, st.d_pts, st.gd, total, rows, a.normal_radius, a.fpfh_radius, one_csr ? &prefix : nullptr, hist, index, &d_pos));
    PCC_TRY(b->slice.reserve((n_clusters + 1) * sizeof(unsigned int)));
    PCC_TRY(launch_batch_finish(s, d_pos, st.d_bases, n_clusters, total, b->slice.as<unsigned int>(), index));
    // the slice bounds in one copy
    PCC_TRY(b->down.reserve((n_clusters + 1) * sizeof(unsigned int)));
    PCC_HIP(hipMemcpyAsync(b->down.p, b->slice.p, (n_clusters + 1) * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
    PCC_HIP(hipStreamSynchronize(s));
    *h_slice = b->down.as<unsigned int>();
    return PCC_OK;
}

int fpfh_descriptors_batch(pcc_index* ix, const FpfhBatchArgs& a) {
    hipStream_t s = ix->stream;
    const ClusterRanges& r = a.ranges;
    const size_t n_clusters = r.n_clusters;
    PCC_TRY(sync_info(ix));  // (a pending mirror of the handle's own grid would overwrite stats[2] later)
    FpfhBatchScratch* b = scratch<FpfhBatchScratch>(ix);
    const RangeBatchPlan plan = range_batch_plan(r.offsets, n_clusters, 0, (size_t)ix->opt.fpfh_batch_brute_max);  // (0: no minimum)
    const size_t total = plan.total();
    const bool host = r.mem == PCC_MEM_HOST;
    // with every cluster on the batch route the rows of a device caller are written where they stay
    const bool in_place = !host && plan.n_large == 0;

    unsigned int n_csr = 0;
    const unsigned int* h_slice = nullptr;
    const std::vector<unsigned int> no_slice(n_clusters + 1, 0u);
    if (total) {
        float* hist = a.out_hist;
        int32_t* index = a.out_index;
        if (!in_place) {
            PCC_TRY(b->out_hist.reserve(total * FPFH_BINS * sizeof(float)));
            PCC_TRY(b->out_index.reserve(total * sizeof(int32_t)));
            hist = b->out_hist.as<float>();
            index = b->out_index.as<int32_t>();
        }
        PCC_TRY(fpfh_batch_brute(ix, a, plan, hist, index, &n_csr, &h_slice));
    }
    if (!h_slice) h_slice = no_slice.data();
    ix->stats[0] = plan.n_brute;
    ix->stats[1] = plan.n_large;
    ix->stats[2] = n_csr;
    ix->stats_pending = false;

    // ---- the clusters above the limit: the single path on the work handle, straight into their place ----------------------------
    // (a cluster's rows start behind the batch route's rows in front of it, h_slice[c], and the work handle's so far)
    std::vector<size_t> single_m(n_clusters, 0);
    size_t singles = 0;
    PCC_TRY(for_each_on_work_handle(ix, b->work, r, plan, [&](pcc_index* w, size_t c, size_t n_valid) -> int {
        if (!n_valid) return PCC_OK;  // (the single path answers PCC_ERR_EMPTY there)
        const size_t at = h_slice[c] + singles;
        PCC_TRY(pcc_fpfh_descriptors(w, r.mem, a.normal_radius, a.fpfh_radius, FPFH_F_BINS, FPFH_F_BINS, FPFH_F_BINS, a.out_hist + at * FPFH_BINS,
                                     a.out_index + at, &single_m[c]));
        singles += single_m[c];
        return PCC_OK;
    }));

    // ---- the slices, in cluster order ----------------------------------------------------------------------------------------------
    std::vector<size_t> offsets;
    std::vector<FpfhBatchCopy> copies;
    fpfh_batch_splice(plan, h_slice, single_m.data(), &offsets, &copies);
    for (size_t c = 0; c <= n_clusters; ++c) a.out_offsets[c] = offsets[c];
    if (in_place || copies.empty()) return PCC_OK;
    for (const FpfhBatchCopy& cp : copies) {
        PCC_TRY(copy_out(ix, a.out_hist + cp.dst * FPFH_BINS, b->out_hist.as<float>() + cp.src * FPFH_BINS, cp.count * FPFH_BINS * sizeof(float), r.mem));
        PCC_TRY(copy_out(ix, a.out_index + cp.dst, b->out_index.as<int32_t>() + cp.src, cp.count * sizeof(int32_t), r.mem));
    }
    if (host) PCC_HIP(hipStreamSynchronize(s));  // the rows
    return PCC_OK;
}

}  // namespace

}  // namespace pcc

extern "C" {

int pcc_fpfh_descriptors_batch(pcc_index* ctx, const void* pts, size_t stride_bytes, const size_t* offsets, size_t n_clusters, int mem,
                               double normal_radius, double fpfh_radius, int nr_bins_f1, int nr_bins_f2, int nr_bins_f3, float* out_histograms,
                               int32_t* out_point_index, size_t* out_offsets) {
    using namespace pcc;
    // the arguments first: all of it host arithmetic, refused before the handle or any device is looked at
    // 1 - 4. the memory space, null arrays, the stride and the alignment, the offsets
    const ClusterRanges ranges{static_cast<const unsigned char*>(pts), stride_bytes, offsets, n_clusters, mem};
    PCC_TRY(check_range_batch(ranges, out_offsets, {out_histograms, out_point_index}));
    // 5. the parameters
    PCC_TRY(check_fpfh_params(normal_radius, fpfh_radius, nr_bins_f1, nr_bins_f2, nr_bins_f3));
    if (n_clusters == 0) { out_offsets[0] = 0; return PCC_OK; }  // (no device is touched: not even the handle's)
    // 6. the handle
    PCC_ENTER(ctx);
    ev_next(ctx);
    ev_mark(ctx, EV_CALL0);
    const FpfhBatchArgs a{ranges, normal_radius, fpfh_radius, out_histograms, out_point_index, out_offsets};
    const int st = fpfh_descriptors_batch(ctx, a);
    ev_mark(ctx, EV_CALL1);
    return st;
}
}  // extern "C"
