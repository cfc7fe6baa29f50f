// rift_batch.hip -- the RIFT descriptor pipeline for EVERY cluster of a comparison at once (gfx950): pcc_rift_descriptors_batch.
//
// The reference computes descriptors one cluster at a time (src/comparator.cpp:1224-1272: processRIFT, :590-684, or
// processRIFTwithSIFT ending in it, per cluster of both scenes).  One cluster at a time is set_input + pcc_rift_descriptors on
// a tree of its own: two CSR builds with a wait each, about 25 launches and the final count, never below 0.32 ms however small
// the cluster (EXPERIMENTS.md, "RIFT descriptors").  Here the clouds of a call are ONE concatenated cloud -- point base[c] + i
// is point i of cloud c -- with ONE CSR per radius whose rows hold members of the point's own cloud only, and the stages of
// rift.hip / normals.hip run once over it.  Launches and waits do not depend on the number of clouds.
//
// The rows come from an exhaustive builder (k_rift_batch_rows): the reference sends only clusters of up to 700 points down this
// route, and at that size n^2 distance tests per cloud cost less than any index build.  It is driven by a host-built table of
// work items (rift_batch_plan.hpp: up to 64 queries of one cloud each, fewer while the table is short).  A workgroup stages its cloud in LDS, 2048 points at a time,
// tiles in ascending order; each wave takes one query at a time with its lanes over the candidates of the tile; the test is
// grid_device.hpp's dist2 arithmetic, d < r2 (the grid path's rounding); hits are compacted with a ballot, so a row comes out in
// candidate (index) order, the count pass and the fill pass agreeing because they are the same code.  Non-finite points carry
// their raw coordinates: every distance to or from one is NaN or +inf and fails the comparison, so they are in no row and
// their own rows are empty -- as in the single path.  k_sort_rows (knn.hip) then sorts every row by (d2, index): ascending
// concatenated index within a cloud is ascending local index, so a row is the single path's row with base[c] added.
//
// Clouds above PCC_OPT_RIFT_BATCH_BRUTE_MAX points would make the quadratic builder the bottleneck: they take the single path
// inside the same call, one by one, on a work handle kept in ctx, and their slices are spliced in.  The host scaffold (route
// split, pack, upload layout, lease of the work handle, shared argument checks) is cloud_batch.hpp's and entry.hpp's: DESIGN.md 4.16.
#include <algorithm>
#include <vector>

#include "entry.hpp"
#include "lane_ops.hpp"
#include "grid_device.hpp"
#include "rift_math.hpp"
#include "rift_batch_plan.hpp"
#include "desc_batch.hpp"

namespace pcc {

namespace {

// FILL = false: counts[q] = the row length of every query of the item.  FILL = true: the row's keys at offsets[q], in
// candidate order.  pts: the concatenated cloud, w = bits(concatenated index).
template <bool FILL>
__global__ void __launch_bounds__(256)
k_rift_batch_rows(const RiftBatchItem* __restrict__ items, const float4* __restrict__ pts, float r2, unsigned int* __restrict__ counts,
                  const unsigned int* __restrict__ offsets, unsigned long long* __restrict__ keys) {
    __shared__ float4 tile[RB_TILE];
    __shared__ unsigned int found[RB_QUERIES];  // hits of every query over the tiles so far; a query belongs to one wave
    const unsigned int lane = threadIdx.x & 63;
    const unsigned int wave = (unsigned int)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const RiftBatchItem it = items[blockIdx.x];  // (block-uniform: scalar loads)
    const float4* __restrict__ cloud = pts + it.base;
    if (threadIdx.x < RB_QUERIES) found[threadIdx.x] = 0u;
    for (unsigned int t0 = 0; t0 < it.n; t0 += RB_TILE) {  // block-uniform
        const unsigned int tn = min(RB_TILE, it.n - t0);
        __syncthreads();  // (the tile before has been used up; found[] is cleared)
        for (unsigned int i = threadIdx.x; i < tn; i += 256) tile[i] = cloud[t0 + i];
        __syncthreads();
        for (unsigned int qi = wave; qi < it.nq; qi += 4) {  // wave-uniform
            const unsigned int q = it.base + it.q0 + qi;
            const float4 qv = pts[q];
            unsigned int written = found[qi];
            unsigned int row_beg = 0, row_len = 0;
            if constexpr (FILL) {
                row_beg = offsets[q];
                row_len = offsets[q + 1] - row_beg;
            }
            for (unsigned int c0 = 0; c0 < tn; c0 += 64) {
                const unsigned int c = c0 + lane;
                const float4 r = tile[min(c, tn - 1u)];
                const float d = dist2_nc(qv.x, qv.y, qv.z, r);
                PCC_PAIR(c < tn);
                const bool hit = c < tn && d < r2;
                const unsigned long long mask = __ballot(hit);
                if constexpr (FILL) {
                    // (a fill can only find what the count found -- same arithmetic --; the bound is belt and braces)
                    const unsigned int slot = lanes_below(mask, written);
                    if (hit && slot < row_len) keys[(size_t)row_beg + slot] = make_key(d, r);
                }
                written += (unsigned int)__popcll(mask);
            }
            if (lane == 0) found[qi] = written;
        }
    }
    if constexpr (!FILL) {
        __syncthreads();
        if (threadIdx.x < it.nq) counts[it.base + it.q0 + threadIdx.x] = found[threadIdx.x];
    }
}

// After the stages (pos = the exclusive scan of the keep flags over the concatenation, pos[n] = the kept rows): the rows of
// cloud c are slice[c] .. slice[c + 1], and every kept point index loses its cloud's base.  Shared with fpfh_batch.hip.
__global__ void __launch_bounds__(256)
k_batch_finish(const unsigned int* __restrict__ pos, const unsigned int* __restrict__ bases, unsigned int n_clouds, unsigned int n,
               unsigned int* __restrict__ slice, int32_t* __restrict__ out_index) {
    const unsigned int stride = gridDim.x * blockDim.x, t = blockIdx.x * blockDim.x + threadIdx.x;
    for (unsigned int c = t; c <= n_clouds; c += stride) slice[c] = pos[bases[c]];
    const unsigned int kept = min(pos[n], n);
    for (unsigned int row = t; row < kept; row += stride) {
        const unsigned int i = (unsigned int)out_index[row];
        if (i >= n) continue;  // (cannot happen: the stages wrote a point of the concatenation)
        // the last cloud whose base is <= i (empty clouds share a base with the cloud behind them: never the answer)
        out_index[row] = (int32_t)(i - bases[range_of(bases, n_clouds, i)]);
    }
}

}  // namespace

int launch_batch_finish(hipStream_t s, const unsigned int* pos, const unsigned int* bases, size_t n_clouds, size_t n, unsigned int* slice,
                        int32_t* out_index) {
    hipLaunchKernelGGL(k_batch_finish, dim3(blocks_for(std::max(n, n_clouds + 1))), dim3(256), 0, s, pos, bases, (unsigned int)n_clouds,
                       (unsigned int)n, slice, out_index);
    PCC_HIP(hipGetLastError());
    return PCC_OK;
}

struct RiftBatchScratch : BatchStaging {  // (up: order words + bases + table + points + colour words; down: the slice bounds)
    static constexpr ScratchSlot slot = SCRATCH_RIFT_BATCH;
    DevBuf offs, keys;  // the CSR of the radius in use: uint32 offsets[n + 1] + the same as int64; u64 keys
    DevBuf slice;       // uint32[n_clouds + 1]
};

// The sorted radius rows of a concatenation of clouds as ONE CSR (pcc_internal.hpp): rows of d2 < r2 from the exhaustive builder
// above, driven by a table of work items that never cross a cloud.  offs: uint32 offsets[total + 1] + the same as int64; keys:
// the u64 entries.  One wait (the CSR's total).  Shared with sift_batch.hip, whose octave rounds are such concatenations.
int batch_radius_rows(pcc_index* ix, const RiftBatchItem* d_items, unsigned int n_items, const float4* d_pts, size_t total, float r2,
                      DevBuf& offs, DevBuf& keys_buf, const unsigned long long** keys_out, const unsigned int** offsets_out) {
    hipStream_t s = ix->stream;
    const size_t off32_bytes = align_up((total + 1) * sizeof(unsigned int), 16);
    PCC_TRY(offs.reserve(off32_bytes + (total + 1) * sizeof(int64_t)));
    unsigned int* off32 = offs.as<unsigned int>();
    int64_t* off64 = reinterpret_cast<int64_t*>(offs.as<char>() + off32_bytes);
    PCC_HIP(hipMemsetAsync(off32, 0, (total + 1) * sizeof(unsigned int), s));
    hipLaunchKernelGGL((k_rift_batch_rows<false>), dim3(n_items), dim3(256), 0, s, d_items, d_pts, r2, off32, (const unsigned int*)nullptr,
                       (unsigned long long*)nullptr);
    PCC_HIP(hipGetLastError());
    unsigned long long entries = 0;
    PCC_TRY(csr_offsets(ix, off32, off64, total, &entries));
    PCC_TRY(keys_buf.reserve((size_t)(entries ? entries : 1) * sizeof(unsigned long long)));
    unsigned long long* keys = keys_buf.as<unsigned long long>();
    if (entries) {
        hipLaunchKernelGGL((k_rift_batch_rows<true>), dim3(n_items), dim3(256), 0, s, d_items, d_pts, r2, (unsigned int*)nullptr,
                           (const unsigned int*)off32, keys);
        PCC_HIP(hipGetLastError());
        PCC_TRY(sort_csr_rows(s, off64, total, keys));
    }
    *keys_out = keys;
    *offsets_out = off32;
    return PCC_OK;
}

// ---- the half over a device-resident concatenation (desc_batch.hpp): shared with cluster_desc.hip ---------------------------
int rift_batch_run(pcc_index* ix, const RiftBatchInput& in, double normal_radius, double gradient_radius, double rift_radius,
                   const unsigned int** d_slice) {
    RiftBatchScratch* b = scratch<RiftBatchScratch>(ix);
    const size_t total = in.total, n_clouds = in.n_clouds;
    // ---- the CSR at a radius: count, total (the wait), scan, fill, sort (batch_radius_rows) ------------------------------
    const RiftRows rows = [&](double radius, const unsigned long long** keys_out, const unsigned int** offsets_out) -> int {
        return batch_radius_rows(ix, in.d_items, in.n_items, in.d_pts, total, (float)(radius * radius), b->offs, b->keys, keys_out, offsets_out);
    };
    // ---- the stages of the single call, once over the concatenation -------------------------------------------------------
    RiftScratch* r = scratch<RiftScratch>(ix);
    PCC_TRY(r->out_hist.reserve(total * RIFT_BINS * sizeof(float)));
    PCC_TRY(r->out_index.reserve(total * sizeof(int32_t)));
    PCC_TRY(rift_stages(ix, in.d_pts, in.d_pts, in.gd, total, rows, in.d_rgb, sizeof(uint32_t), normal_radius, gradient_radius, rift_radius,
                        r->out_hist.as<float>(), r->out_index.as<int32_t>()));
    PCC_TRY(b->slice.reserve((n_clouds + 1) * sizeof(unsigned int)));
    PCC_TRY(launch_batch_finish(ix->stream, r->keep.as<unsigned int>(), in.d_bases, n_clouds, total, b->slice.as<unsigned int>(), r->out_index.as<int32_t>()));
    *d_slice = b->slice.as<unsigned int>();
    return PCC_OK;
}

int rift_batch_slices(pcc_index* ix, size_t n_clouds, const unsigned int** h_slice) {
    RiftBatchScratch* b = scratch<RiftBatchScratch>(ix);
    PCC_TRY(b->down.reserve((n_clouds + 1) * sizeof(unsigned int)));
    PCC_HIP(hipMemcpyAsync(b->down.p, b->slice.p, (n_clouds + 1) * sizeof(unsigned int), hipMemcpyDeviceToHost, ix->stream));
    PCC_HIP(hipStreamSynchronize(ix->stream));
    *h_slice = b->down.as<unsigned int>();
    return PCC_OK;
}

int rift_batch_fetch(pcc_index* ix, size_t kept, float* out_hist, int32_t* out_index) {
    if (!kept) return PCC_OK;
    RiftScratch* r = scratch<RiftScratch>(ix);
    PCC_HIP(hipMemcpyAsync(out_hist, r->out_hist.p, kept * RIFT_BINS * sizeof(float), hipMemcpyDeviceToHost, ix->stream));
    PCC_HIP(hipMemcpyAsync(out_index, r->out_index.p, kept * sizeof(int32_t), hipMemcpyDeviceToHost, ix->stream));
    PCC_HIP(hipStreamSynchronize(ix->stream));
    return PCC_OK;
}

// every cloud of the call through the exhaustive builder: out_hist / out_index / offsets (n_clouds + 1) are host arrays
static int rift_batch_brute(pcc_index* ix, const CloudBatch& batch, double normal_radius, double gradient_radius, double rift_radius,
                            float* out_hist, int32_t* out_index, size_t* out_offsets) {
    hipStream_t s = ix->stream;
    RiftBatchScratch* b = scratch<RiftBatchScratch>(ix);
    const size_t n_clouds = batch.n_clouds;
    std::vector<uint32_t> bases;
    std::vector<RiftBatchItem> items;
    rift_batch_plan(batch.n, n_clouds, &bases, &items);
    const size_t total = bases[n_clouds];
    for (size_t c = 0; c <= n_clouds; ++c) out_offsets[c] = 0;
    if (total == 0) return PCC_OK;

    // ---- one pinned buffer, one copy: the order's n_valid word, bases, table, 16 bytes + 4 bytes a point ------------------
    static_assert(sizeof(GridDev) == 112, "tests/cpp/test_cloud_batch.cpp records this upload's offsets for a header of 112 bytes");
    const ConcatLayout up(sizeof(GridDev), 128, n_clouds, items.size(), total);
    PCC_TRY(b->up.reserve(up.bytes));
    PCC_TRY(b->dev.reserve(up.bytes));
    char* u = b->up.as<char>();
    up.fill(u, batch, bases, items, false);
    // (the consumers read nothing of the grid but n_valid: every point of the concatenation is taken, in its order -- the
    // non-finite ones have empty rows and end as the points outside cloud2 do)
    reinterpret_cast<GridDev*>(u)->n_valid = (unsigned int)total;
    PCC_HIP(hipMemcpyAsync(b->dev.p, u, up.bytes, hipMemcpyHostToDevice, s));
    const char* d = b->dev.as<char>();
    const GridDev* gd = reinterpret_cast<const GridDev*>(d);
    const unsigned int* d_bases = reinterpret_cast<const unsigned int*>(d + up.bases_at);
    const RiftBatchItem* d_items = reinterpret_cast<const RiftBatchItem*>(d + up.items_at);
    const float4* d_pts = reinterpret_cast<const float4*>(d + up.pts_at);
    const unsigned char* d_rgb = reinterpret_cast<const unsigned char*>(d + up.rgb_at);

    RiftBatchInput in;
    in.n_clouds = n_clouds;
    in.total = total;
    in.gd = gd;
    in.d_bases = d_bases;
    in.d_items = d_items;
    in.n_items = (unsigned int)items.size();
    in.d_pts = d_pts;
    in.d_rgb = d_rgb;
    const unsigned int* d_slice = nullptr;
    PCC_TRY(rift_batch_run(ix, in, normal_radius, gradient_radius, rift_radius, &d_slice));
    // the slice bounds in one copy, then the rows that were written in one copy each
    const unsigned int* h_slice = nullptr;
    PCC_TRY(rift_batch_slices(ix, n_clouds, &h_slice));
    for (size_t c = 0; c <= n_clouds; ++c) out_offsets[c] = h_slice[c];
    return rift_batch_fetch(ix, h_slice[n_clouds], out_hist, out_index);
}

int rift_descriptors_batch(pcc_index* ix, const CloudBatch& batch, double normal_radius, double gradient_radius, double rift_radius,
                           float* out_hist, int32_t* out_index, size_t* out_offsets) {
    RiftBatchScratch* b = scratch<RiftBatchScratch>(ix);
    const size_t n_clouds = batch.n_clouds, brute_max = (size_t)ix->opt.rift_batch_brute_max;
    const BatchRoutes routes = batch_routes(batch.n, n_clouds, brute_max);
    ix->stats[0] = routes.n_brute;
    ix->stats[1] = routes.n_large;
    ix->stats_pending = false;
    if (routes.n_large == 0) return rift_batch_brute(ix, batch, normal_radius, gradient_radius, rift_radius, out_hist, out_index, out_offsets);

    // ---- some clouds are above the limit: the others as a batch into arrays of their own, these one by one, then the splice --
    CloudBatch small = batch;
    small.n = routes.small_n.data();
    std::vector<size_t> small_off(n_clouds + 1, 0);
    std::vector<float> small_hist(std::max<size_t>(routes.n_brute, 1) * RIFT_BINS);
    std::vector<int32_t> small_index(std::max<size_t>(routes.n_brute, 1));
    PCC_TRY(rift_batch_brute(ix, small, normal_radius, gradient_radius, rift_radius, small_hist.data(), small_index.data(), small_off.data()));
    WorkLease lease;
    PCC_TRY(lease.take(ix, b->work, true));
    pcc_index* w = lease.w;
    size_t at = 0;
    for (size_t c = 0; c < n_clouds; ++c) {
        out_offsets[c] = at;
        if (batch.n[c] <= brute_max) {
            const size_t m = small_off[c + 1] - small_off[c];
            if (m) {
                memcpy(out_hist + at * RIFT_BINS, small_hist.data() + small_off[c] * RIFT_BINS, m * RIFT_BINS * sizeof(float));
                memcpy(out_index + at, small_index.data() + small_off[c], m * sizeof(int32_t));
            }
            at += m;
            continue;
        }
        if (!cloud_any_finite(batch.pts[c], batch.n[c], batch.stride)) continue;  // (the single path answers PCC_ERR_EMPTY there)
        size_t m = 0;
        PCC_TRY(pcc_index_set_input(w, batch.pts[c], batch.n[c], batch.stride, 3, PCC_MEM_HOST));
        PCC_TRY(pcc_rift_descriptors(w, batch.rgb[c], batch.rgb_stride, PCC_MEM_HOST, normal_radius, gradient_radius, rift_radius, RIFT_D_BINS,
                                     RIFT_G_BINS, out_hist + at * RIFT_BINS, out_index + at, &m));
        at += m;
    }
    out_offsets[n_clouds] = at;
    return PCC_OK;
}

PCC_PAIRS_TAKE(rift_batch)

}  // namespace pcc

extern "C" {

int pcc_rift_descriptors_batch(pcc_index* ctx, size_t n_clouds, const void* const* pts, const size_t* n, size_t stride, const void* const* rgb,
                               size_t rgb_stride, int mem, double normal_radius, double gradient_radius, double rift_radius,
                               int nr_distance_bins, int nr_gradient_bins, float* out_hist, int32_t* out_index, size_t* out_offsets) {
    using namespace pcc;
    // the arguments first: all of it host arithmetic, refused before the handle or any device is looked at
    const CloudBatch batch{n_clouds, pts, n, stride, rgb, rgb_stride};
    PCC_TRY(check_cloud_batch("pcc_rift_descriptors_batch", batch, mem));
    if (rgb_stride < 4 || rgb_stride % 4) {
        set_error("colour words must be 4-byte aligned, stride %zu a multiple of 4 and >= 4", rgb_stride);
        return PCC_ERR_INVALID;
    }
    if (!out_offsets) { set_error("null out_offsets"); return PCC_ERR_INVALID; }
    if (n_clouds >= (1ull << 31)) { set_error("more than 2^31 clouds"); return PCC_ERR_UNSUPPORTED; }
    if (n_clouds && (!pts || !n || !rgb || !out_hist || !out_index)) { set_error("null array argument"); return PCC_ERR_INVALID; }
    PCC_TRY(check_rift_params(normal_radius, gradient_radius, rift_radius, nr_distance_bins, nr_gradient_bins));
    PCC_TRY(check_batch_clouds(batch, mem));
    if (n_clouds == 0) { out_offsets[0] = 0; return PCC_OK; }  // (no device is touched: not even the handle's)
    PCC_ENTER(ctx);
    ev_next(ctx);
    ev_mark(ctx, EV_CALL0);
    const int st = rift_descriptors_batch(ctx, batch, normal_radius, gradient_radius, rift_radius, out_hist, out_index, out_offsets);
    ev_mark(ctx, EV_CALL1);
    return st;
}
}  // extern "C"
