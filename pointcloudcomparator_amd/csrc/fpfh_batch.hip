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
// caller) -- there is no intermediate descriptor buffer.  k_fpfh_batch_finish turns the scan into the slice bounds and takes
// every cluster's base off its point indices.
//
// Clusters above PCC_OPT_FPFH_BATCH_BRUTE_MAX points take set_input + pcc_fpfh_descriptors on a work handle kept in ctx, in the
// caller's memory space, straight into their place in the caller's arrays; the batch route's rows are then written to a buffer
// of the library's and copied to their places run by run (fpfh_batch_plan.hpp: routes, bases, items, the copy list).
#include <algorithm>
#include <vector>

#include "entry.hpp"
#include "lane_ops.hpp"
#include "grid_device.hpp"
#include "plane_fit.hpp"
#include "fpfh_math.hpp"
#include "cloud_batch.hpp"
#include "fpfh_batch_plan.hpp"

namespace pcc {

namespace {

// ---- the pack from device memory --------------------------------------------------------------------------------------------
// Point e of the concatenation lies in cluster c = the last one with bases[c] <= e (a cluster off the batch route is empty here
// and never the answer) and is the caller's record src[c] + (e - bases[c]): out[e] = x, y, z, w = bits(e).  A plain streaming
// copy.  V16: the records are 16-byte aligned and a multiple of 16 bytes apart: x, y, z in one load; else three scalar loads.
template <bool V16>
__global__ void __launch_bounds__(256)
k_fpfh_batch_pack(const unsigned char* __restrict__ pts, size_t stride, const unsigned int* __restrict__ src, const unsigned int* __restrict__ bases,
                  unsigned int n_clusters, unsigned int total, float4* __restrict__ out) {
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
        out[e] = make_float4(x, y, z, __uint_as_float(e));
    }
}

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

// ---- after the stages (pos = the exclusive scan of cloud2's flags over the concatenation, pos[n] = the rows written): the rows
// of cluster c are slice[c] .. slice[c + 1], and every point index loses its cluster's base
__global__ void __launch_bounds__(256)
k_fpfh_batch_finish(const unsigned int* __restrict__ pos, const unsigned int* __restrict__ bases, unsigned int n_clusters, unsigned int n,
                    unsigned int* __restrict__ slice, int32_t* __restrict__ out_index) {
    const unsigned int stride = gridDim.x * blockDim.x, t = blockIdx.x * blockDim.x + threadIdx.x;
    for (unsigned int c = t; c <= n_clusters; c += stride) slice[c] = pos[bases[c]];
    const unsigned int kept = min(pos[n], n);
    for (unsigned int row = t; row < kept; row += stride) {
        const unsigned int i = (unsigned int)out_index[row];
        if (i >= n) continue;  // (cannot happen: the weighting kernel wrote a point of the concatenation)
        out_index[row] = (int32_t)(i - bases[range_of(bases, n_clusters, i)]);
    }
}

unsigned int blocks_for(size_t n) { return (unsigned int)std::min<size_t>((n + 255) / 256, 2048); }

// (up: GridDev + the clusters' places among the caller's records + bases + table [+ points]; down: the slice bounds)
struct FpfhBatchScratch : BatchStaging {
    static constexpr ScratchSlot slot = SCRATCH_FPFH_BATCH;
    DevBuf offs, keys;           // the CSR of the radius in use: uint32 offsets[n + 1] + the same as int64; u64 keys
    DevBuf slice;                // uint32[n_clusters + 1]
    DevBuf out_hist, out_index;  // the batch route's rows where the stages cannot write into the caller's arrays
};

struct FpfhBatchArgs {
    const unsigned char* pts;
    size_t stride;
    const size_t* offsets;
    size_t n_clusters;
    int mem;
    double normal_radius, fpfh_radius;
    float* out_hist;
    int32_t* out_index;
    size_t* out_offsets;
};

// The batch route: the clusters up to the limit staged as one concatenation, the stages over it, the finish.  hist / index: device
// arrays of plan.bases[n_clusters] rows the descriptors are written to.  *h_slice: the slice bounds on the host (valid until the
// scratch's `down` is used again).  Waits: one per CSR, one for the slice bounds.
int fpfh_batch_brute(pcc_index* ix, const FpfhBatchArgs& a, const FpfhBatchPlan& plan, float* hist, int32_t* index, unsigned int* n_csr,
                     const unsigned int** h_slice) {
    hipStream_t s = ix->stream;
    FpfhBatchScratch* b = scratch<FpfhBatchScratch>(ix);
    const size_t n_clusters = a.n_clusters, total = plan.bases[n_clusters];
    const unsigned int nc = (unsigned int)n_clusters;
    const unsigned char* p0 = a.pts + a.offsets[0] * a.stride;

    // ---- one pinned buffer, one copy: the order's n_valid word, src, bases, table -- and from host memory 16 bytes a point ----
    static_assert(sizeof(GridDev) % 16 == 0, "the clusters' places lie directly behind the GridDev");
    const size_t header = sizeof(GridDev) + (n_clusters + 1) * sizeof(uint32_t);
    const ConcatLayout up(header, 128, n_clusters, plan.items.size(), total);
    const bool host = a.mem == PCC_MEM_HOST;
    const size_t up_bytes = host ? up.rgb_at : up.pts_at;  // (no colour is read: the layout's last part is not used)
    PCC_TRY(b->up.reserve(up_bytes));
    PCC_TRY(b->dev.reserve(up.rgb_at));
    char* u = b->up.as<char>();
    memset(u, 0, up.items_at);
    // (the consumers read nothing of the grid but n_valid: every point of the concatenation is taken, in its order -- the
    // non-finite ones have empty rows, no normal, and leave with the points outside cloud2)
    reinterpret_cast<GridDev*>(u)->n_valid = (unsigned int)total;
    memcpy(u + sizeof(GridDev), plan.src.data(), (n_clusters + 1) * sizeof(uint32_t));
    memcpy(u + up.bases_at, plan.bases.data(), (n_clusters + 1) * sizeof(uint32_t));
    if (!plan.items.empty()) memcpy(u + up.items_at, plan.items.data(), plan.items.size() * sizeof(RiftBatchItem));
    if (host) {
        float* p4 = reinterpret_cast<float*>(u + up.pts_at);
        for (size_t c = 0; c < n_clusters; ++c) {
            const unsigned char* src = p0 + (size_t)plan.src[c] * a.stride;
            for (size_t i = 0; i < plan.small_n[c]; ++i) {
                const uint32_t at = plan.bases[c] + (uint32_t)i;
                memcpy(p4 + (size_t)at * 4, src + i * a.stride, 12);
                memcpy(p4 + (size_t)at * 4 + 3, &at, 4);
            }
        }
    }
    PCC_HIP(hipMemcpyAsync(b->dev.p, u, up_bytes, hipMemcpyHostToDevice, s));
    char* d = b->dev.as<char>();
    const GridDev* gd = reinterpret_cast<const GridDev*>(d);
    const unsigned int* d_src = reinterpret_cast<const unsigned int*>(d + sizeof(GridDev));
    const unsigned int* d_bases = reinterpret_cast<const unsigned int*>(d + up.bases_at);
    const RiftBatchItem* d_items = reinterpret_cast<const RiftBatchItem*>(d + up.items_at);
    float4* d_pts = reinterpret_cast<float4*>(d + up.pts_at);
    if (!host) {
        if (a.stride % 16 == 0 && reinterpret_cast<uintptr_t>(p0) % 16 == 0)
            hipLaunchKernelGGL((k_fpfh_batch_pack<true>), dim3(blocks_for(total)), dim3(256), 0, s, p0, a.stride, d_src, d_bases, nc, (unsigned int)total, d_pts);
        else
            hipLaunchKernelGGL((k_fpfh_batch_pack<false>), dim3(blocks_for(total)), dim3(256), 0, s, p0, a.stride, d_src, d_bases, nc, (unsigned int)total, d_pts);
        PCC_HIP(hipGetLastError());
    }

    // ---- the CSR at a radius: count, total (the wait), scan, fill, sort (batch_radius_rows) ----------------------------------
    const unsigned int n_items = (unsigned int)plan.items.size();
    *n_csr = 0;
    const RiftRows rows = [&](double radius, const unsigned long long** keys_out, const unsigned int** offsets_out) -> int {
        ++*n_csr;
        return batch_radius_rows(ix, d_items, n_items, d_pts, total, radius2(radius), b->offs, b->keys, keys_out, offsets_out);
    };
    // normal_radius <= fpfh_radius: the plane fit over the prefix of the ONE CSR
    const FpfhNormals prefix = [&](float4* normals, const unsigned long long** keys_out, const unsigned int** offsets_out) -> int {
        PCC_TRY(rows(a.fpfh_radius, keys_out, offsets_out));
        PCC_HIP(hipMemsetAsync(normals, 0xff, total * sizeof(float4), s));
        hipLaunchKernelGGL(k_fpfh_batch_normals, dim3(blocks_for(total)), dim3(256), 0, s, *keys_out, *offsets_out, (const float4*)d_pts,
                           (unsigned int)total, radius2(a.normal_radius), normals);
        PCC_HIP(hipGetLastError());
        return PCC_OK;
    };
    const bool one_csr = a.normal_radius <= a.fpfh_radius;
    const unsigned int* d_pos = nullptr;
    PCC_TRY(fpfh_stages(ix, d_pts, d_pts, gd, total, rows, a.normal_radius, a.fpfh_radius, one_csr ? &prefix : nullptr, hist, index, &d_pos));
    PCC_TRY(b->slice.reserve((n_clusters + 1) * sizeof(unsigned int)));
    hipLaunchKernelGGL(k_fpfh_batch_finish, dim3(blocks_for(std::max(total, n_clusters + 1))), dim3(256), 0, s, d_pos, d_bases, nc, (unsigned int)total,
                       b->slice.as<unsigned int>(), index);
    PCC_HIP(hipGetLastError());
    // the slice bounds in one copy
    PCC_TRY(b->down.reserve((n_clusters + 1) * sizeof(unsigned int)));
    PCC_HIP(hipMemcpyAsync(b->down.p, b->slice.p, (n_clusters + 1) * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
    PCC_HIP(hipStreamSynchronize(s));
    *h_slice = b->down.as<unsigned int>();
    return PCC_OK;
}

int fpfh_descriptors_batch(pcc_index* ix, const FpfhBatchArgs& a) {
    hipStream_t s = ix->stream;
    const size_t n_clusters = a.n_clusters;
    PCC_TRY(sync_info(ix));  // (a pending mirror of the handle's own grid would overwrite stats[2] later)
    FpfhBatchScratch* b = scratch<FpfhBatchScratch>(ix);
    const FpfhBatchPlan plan = fpfh_batch_plan(a.offsets, n_clusters, (size_t)ix->opt.fpfh_batch_brute_max);
    const size_t total = plan.bases[n_clusters];
    const bool host = a.mem == PCC_MEM_HOST;
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
    std::vector<size_t> single_m(n_clusters, 0);
    if (plan.n_large) {
        WorkLease lease;
        PCC_TRY(lease.take(ix, b->work, true));
        pcc_index* w = lease.w;
        size_t at = 0;
        for (size_t c = 0; c < n_clusters; ++c) {
            if (!plan.on_work_handle(c)) { at += h_slice[c + 1] - h_slice[c]; continue; }
            PCC_TRY(pcc_index_set_input(w, a.pts + a.offsets[c] * a.stride, plan.n[c], a.stride, 3, a.mem));
            size_t n_valid = 0;
            PCC_TRY(pcc_index_size(w, &n_valid));
            if (!n_valid) continue;  // (the single path answers PCC_ERR_EMPTY there)
            PCC_TRY(pcc_fpfh_descriptors(w, a.mem, a.normal_radius, a.fpfh_radius, FPFH_F_BINS, FPFH_F_BINS, FPFH_F_BINS,
                                         a.out_hist + at * FPFH_BINS, a.out_index + at, &single_m[c]));
            at += single_m[c];
        }
    }

    // ---- the slices, in cluster order ----------------------------------------------------------------------------------------------
    std::vector<size_t> offsets;
    std::vector<FpfhBatchCopy> copies;
    fpfh_batch_splice(plan, h_slice, single_m.data(), &offsets, &copies);
    for (size_t c = 0; c <= n_clusters; ++c) a.out_offsets[c] = offsets[c];
    if (in_place || copies.empty()) return PCC_OK;
    for (const FpfhBatchCopy& cp : copies) {
        PCC_TRY(copy_out(ix, a.out_hist + cp.dst * FPFH_BINS, b->out_hist.as<float>() + cp.src * FPFH_BINS, cp.count * FPFH_BINS * sizeof(float), a.mem));
        PCC_TRY(copy_out(ix, a.out_index + cp.dst, b->out_index.as<int32_t>() + cp.src, cp.count * sizeof(int32_t), a.mem));
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
    // 1. the memory space
    PCC_TRY(check_mem(mem));
    // 2. null arrays (the clusters' arrays may be null while no cluster holds a point)
    if (!offsets || !out_offsets) { set_error("null argument"); return PCC_ERR_INVALID; }
    const bool any_points = n_clusters && offsets[n_clusters] != offsets[0];
    if (any_points && (!pts || !out_histograms || !out_point_index)) { set_error("null argument"); return PCC_ERR_INVALID; }
    // 3. the stride and the alignment
    PCC_TRY(check_points(nullptr, 0, stride_bytes, mem));  // (the stride alone)
    if (reinterpret_cast<uintptr_t>(pts) % 4 || reinterpret_cast<uintptr_t>(out_histograms) % 4 || reinterpret_cast<uintptr_t>(out_point_index) % 4) {
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
    // 5. the parameters
    PCC_TRY(check_fpfh_params(normal_radius, fpfh_radius, nr_bins_f1, nr_bins_f2, nr_bins_f3));
    if (n_clusters == 0) { out_offsets[0] = 0; return PCC_OK; }  // (no device is touched: not even the handle's)
    // 6. the handle
    PCC_ENTER(ctx);
    ev_next(ctx);
    ev_mark(ctx, EV_CALL0);
    const FpfhBatchArgs a{static_cast<const unsigned char*>(pts), stride_bytes, offsets, n_clusters, mem, normal_radius, fpfh_radius,
                          out_histograms, out_point_index, out_offsets};
    const int st = fpfh_descriptors_batch(ctx, a);
    ev_mark(ctx, EV_CALL1);
    return st;
}
}  // extern "C"
