// region_rgb_batch.hip -- colour region growing for EVERY cluster of a comparison at once (gfx950): pcc_region_growing_rgb_batch.
//
// The reference runs color_growing_segmentation (src/segmentation.cpp:161-216) twice per accepted match
// (src/comparator.cpp:1456-1495), 120 to 200 times per comparison, no call depending on another.  One cluster at a time is
// pcc_index_set_input + pcc_region_growing_rgb: an index build, a self 100-NN, a dozen launches, a read-back per label sweep
// and four more waits -- per cluster.  Here the clouds of a call are ONE concatenated cloud -- point base[c] + i is point i of
// cloud c, w = bits(concatenated index), negative for a non-finite point -- and every stage runs once over it:
//   rows   : k_rgb_batch_knn, the segmented self k-NN: row stride K = nr_region_neighbours for every point, the
//            min(K, finite points of the point's OWN cloud) nearest in ascending (d2, concatenated index) -- inside a cloud that
//            is local-index order, the tie order of a fresh handle --, the rest of the row and the rows of non-finite points
//            the empty key ~0, which the stage kernels skip.  Distances are dist2_nc: unfused and bitwise symmetric, what the
//            link stage's prefix test rests on.  The work items are rift_batch_plan.hpp's: query blocks of ONE cloud each, so no
//            row can hold a point of another cloud.  A workgroup stages its cloud in LDS tiles of RB_TILE points; a wave takes
//            one query at a time, its lanes over the candidates of the tile; keys not below the current K-th are dropped, the
//            survivors gather 64 at a time and are merged into the running top list (knn_merge.hpp: 64 * KR keys in KR
//            registers per lane, KR = 1 for K <= 64, 2 for K <= 128).  The list lives in registers: the query loop is
//            outermost, and a cloud of more than one tile is staged again for every round of four queries (from L2).
//   stages : region_rgb.hip's kernels over the concatenation in index order (rgb_stages.hpp); segment ids are dense over the
//            whole concatenation, so every cloud owns a contiguous range, whose start comes down with the segment count
//   host   : rgb_batch_split.hpp: the pair list sorted once, cut per cloud, rgb_merge_regions per cloud
//   labels : one upload, one launch, one download.
// Launches and waits do not depend on the number of clouds: the waits are one per label sweep and four more.
//
// Clouds above PCC_OPT_RGB_BATCH_BRUTE_MAX points -- the exhaustive rows are quadratic in the cloud --, and every cloud when
// nr_region_neighbours > 128, take the single path inside the same call, one by one, on a work handle kept in ctx.  The host
// scaffold (route split, pack, upload layout, lease, shared argument checks) is cloud_batch.hpp's and entry.hpp's: DESIGN.md 4.16.
#include <algorithm>
#include <cmath>
#include <vector>

#include "entry.hpp"
#include "grid_device.hpp"
#include "knn_merge.hpp"
#include "rgb_batch_split.hpp"
#include "rgb_stages.hpp"
#include "rift_batch_plan.hpp"

namespace pcc {

namespace {

// register r of a top list, r wave-uniform: selects, so that the list is never indexed by a variable
template <int KR>
__device__ __forceinline__ unsigned long long top_reg(const unsigned long long (&top)[KR], int r) {
    unsigned long long v = top[0];
#pragma unroll
    for (int i = 1; i < KR; ++i) v = r == i ? top[i] : v;
    return v;
}

// keys[q][K] for every query q of the item.  pts: the concatenation, w = bits(concatenated index), negative = non-finite.
template <int KR>
__global__ void __launch_bounds__(256)
k_rgb_batch_knn(const RiftBatchItem* __restrict__ items, const float4* __restrict__ pts, int K, unsigned long long* __restrict__ keys) {
    static_assert(KR == 1 || KR == 2, "top list: 64 * KR keys in KR registers per lane");
    __shared__ float4 tile[RB_TILE];
    __shared__ unsigned long long stage_all[4][128];
    const unsigned int lane = threadIdx.x & 63;
    const unsigned int wave = (unsigned int)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    unsigned long long* stage = stage_all[wave];
    const RiftBatchItem it = items[blockIdx.x];  // (block-uniform: scalar loads)
    const float4* __restrict__ cloud = pts + it.base;
    const bool one_tile = it.n <= RB_TILE;  // block-uniform: the cloud is staged once for all queries
    if (one_tile) {
        for (unsigned int i = threadIdx.x; i < it.n; i += 256) tile[i] = cloud[i];
        __syncthreads();
    }
    for (unsigned int q0 = 0; q0 < it.nq; q0 += 4) {  // block-uniform: every wave passes the barriers of every round
        const unsigned int qi = q0 + wave;
        const bool active = qi < it.nq;  // wave-uniform
        const unsigned int q = it.base + it.q0 + (active ? qi : 0u);
        const float4 qv = pts[q];
        const bool scan = active && __builtin_amdgcn_readfirstlane(__float_as_int(qv.w)) >= 0;  // (a non-finite query: an empty row)
        unsigned long long top[KR];
#pragma unroll
        for (int r = 0; r < KR; ++r) top[r] = ~0ull;
        unsigned long long tau = ~0ull;  // the K-th key so far; ~0 while the list holds fewer
        unsigned int scnt = 0;           // wave-uniform
        auto merge = [&](unsigned long long batch) {
            topk_merge<KR>(top, batch, lane);
            tau = shfl_u64(top_reg<KR>(top, (K - 1) >> 6), (K - 1) & 63);
        };
        for (unsigned int t0 = 0; t0 < it.n; t0 += RB_TILE) {  // block-uniform
            const unsigned int tn = min(RB_TILE, it.n - t0);
            if (!one_tile) {
                __syncthreads();  // (the tile before has been used up)
                for (unsigned int i = threadIdx.x; i < tn; i += 256) tile[i] = cloud[t0 + i];
                __syncthreads();
            }
            if (!scan) continue;
            for (unsigned int c0 = 0; c0 < tn; c0 += 64) {
                const unsigned int c = c0 + lane;
                const float4 r = tile[min(c, tn - 1u)];
                const float d = dist2_nc(qv.x, qv.y, qv.z, r);
                PCC_PAIR(c < tn);
                const unsigned long long key = (c < tn && __float_as_int(r.w) >= 0) ? make_key(d, r) : ~0ull;
                // filter by tau, stage the survivors, merge when 64 have gathered (knn.hip's consume)
                const bool pass = key < tau;
                const unsigned long long mask = __ballot(pass);
                if (mask == 0) continue;
                if (pass) stage[lanes_below(mask, scnt)] = key;
                scnt += (unsigned int)__popcll(mask);
                wave_lds_sync();
                if (scnt >= 64) {
                    const unsigned long long batch = stage[lane];
                    const unsigned int rest = scnt - 64;
                    const unsigned long long carry = lane < rest ? stage[64 + lane] : ~0ull;
                    wave_lds_sync();
                    if (lane < rest) stage[lane] = carry;
                    scnt = rest;
                    merge(batch);
                    wave_lds_sync();
                }
            }
        }
        if (!active) continue;
        if (scnt) {
            const unsigned long long batch = lane < scnt ? stage[lane] : ~0ull;
            wave_lds_sync();
            merge(batch);
            wave_lds_sync();
        }
        unsigned long long* row = keys + (size_t)q * K;
#pragma unroll
        for (int r = 0; r < KR; ++r) {
            const int j = r * 64 + (int)lane;
            if (j < K) row[j] = top[r];  // (ascending over (register, lane); what the cloud could not fill is ~0)
        }
    }
}

}  // namespace

int rgb_batch_rows(pcc_index* ix, const RiftBatchItem* d_items, unsigned int n_items, const float4* d_pts, int K, unsigned long long* keys) {
    if (K <= 64)
        hipLaunchKernelGGL(k_rgb_batch_knn<1>, dim3(n_items), dim3(256), 0, ix->stream, d_items, d_pts, K, keys);
    else
        hipLaunchKernelGGL(k_rgb_batch_knn<2>, dim3(n_items), dim3(256), 0, ix->stream, d_items, d_pts, K, keys);
    PCC_HIP(hipGetLastError());
    return PCC_OK;
}

struct RgbBatchScratch : BatchStaging {  // (up: bases + table + points + colour words; down: the clouds' first ids + labels)
    static constexpr ScratchSlot slot = SCRATCH_RGB_BATCH;
    DevBuf keys;              // u64[total][K]: the rows
    DevBuf id_bases, labels;  // uint32[n_clouds + 1]; int32[total]
};

namespace {

struct RgbParams {
    float distance_threshold, point_color_threshold, region_color_threshold;
    uint32_t min_size, max_size;
    unsigned int nr_neighbours, nr_region_neighbours;
};

// the clouds of sizes batch.n[] (0: not on this route) through the batch kernels: labels at out_labels + off[c], counts for EVERY cloud
int rgb_batch_route(pcc_index* ix, const CloudBatch& batch, const RgbParams& par, const size_t* off, int32_t* out_labels, int32_t* out_n_clusters) {
    hipStream_t s = ix->stream;
    RgbBatchScratch* b = scratch<RgbBatchScratch>(ix);
    const size_t n_clouds = batch.n_clouds;
    std::vector<uint32_t> bases;
    std::vector<RiftBatchItem> items;
    rift_batch_plan(batch.n, n_clouds, &bases, &items);
    const size_t total = bases[n_clouds];
    for (size_t c = 0; c < n_clouds; ++c) out_n_clusters[c] = 0;
    ix->stats[0] = ix->stats[1] = ix->stats[7] = 0;
    if (total == 0) return PCC_OK;
    const int K = (int)par.nr_region_neighbours;
    if (total * (size_t)K >= ((size_t)1 << 32)) {
        set_error("%zu x %d row entries in one batch: 2^32 and more are not built -- split the call", total, K);
        return PCC_ERR_UNSUPPORTED;
    }

    // ---- one pinned buffer, one copy: bases, table, 16 bytes + 4 bytes a point -----------------------------------------------
    const ConcatLayout up(0, 1, n_clouds, items.size(), total);
    PCC_TRY(b->up.reserve(up.bytes));
    PCC_TRY(b->dev.reserve(up.bytes));
    up.fill(b->up.as<char>(), batch, bases, items, true);
    PCC_HIP(hipMemcpyAsync(b->dev.p, b->up.p, up.bytes, hipMemcpyHostToDevice, s));
    const char* d = b->dev.as<char>();
    const unsigned int* d_bases = reinterpret_cast<const unsigned int*>(d + up.bases_at);
    const RiftBatchItem* d_items = reinterpret_cast<const RiftBatchItem*>(d + up.items_at);
    const float4* d_pts = reinterpret_cast<const float4*>(d + up.pts_at);

    // ---- the rows ------------------------------------------------------------------------------------------------------------
    PCC_TRY(b->keys.reserve(total * (size_t)K * sizeof(unsigned long long)));
    unsigned long long* keys = b->keys.as<unsigned long long>();
    PCC_TRY(rgb_batch_rows(ix, d_items, (unsigned int)items.size(), d_pts, K, keys));

    // ---- the stages of the single call, once over the concatenation -------------------------------------------------------
    const size_t ids_bytes = align_up((n_clouds + 1) * sizeof(unsigned int), 16);
    PCC_TRY(b->down.reserve(ids_bytes + total * sizeof(int32_t)));
    PCC_TRY(b->id_bases.reserve((n_clouds + 1) * sizeof(unsigned int)));
    PCC_TRY(b->labels.reserve(total * sizeof(int32_t)));
    RgbRun run;
    run.refs = d_pts;
    run.n = (unsigned int)total;
    run.keys = keys;
    run.K = K;
    run.rgb = reinterpret_cast<const unsigned char*>(d + up.rgb_at);
    run.rgb_stride = sizeof(uint32_t);
    run.point_color_threshold = par.point_color_threshold;
    run.nr_neighbours = par.nr_neighbours;
    run.d_bases = d_bases;
    run.n_clouds = (unsigned int)n_clouds;
    run.d_id_bases = b->id_bases.as<unsigned int>();
    run.h_id_bases = b->down.as<unsigned int>();
    run.labels_dev = b->labels.as<int32_t>();
    run.labels_host = reinterpret_cast<int32_t*>(b->down.as<char>() + ids_bytes);
    const float dist2 = par.distance_threshold * par.distance_threshold, r2r2 = par.region_color_threshold * par.region_color_threshold;
    const int min_pts = (int)std::min<uint32_t>(par.min_size, 0x7fffffffu), max_pts = (int)std::min<uint32_t>(par.max_size, 0x7fffffffu);
    PCC_TRY(rgb_stages(ix, run, [&](const RgbSegment* segs, unsigned int ns, RgbSegmentPair* pairs, unsigned int np, std::vector<int32_t>& cluster_of_segment) {
        if (!rgb_batch_split(segs, ns, pairs, np, run.h_id_bases, n_clouds, dist2, r2r2, par.nr_region_neighbours, min_pts, max_pts,
                             cluster_of_segment, out_n_clusters)) {
            set_error("colour region growing: a segment pair crosses two clouds of the batch");
            return (int)PCC_ERR_DEVICE;
        }
        return (int)PCC_OK;
    }));
    for (size_t c = 0; c < n_clouds; ++c)
        if (batch.n[c]) memcpy(out_labels + off[c], run.labels_host + bases[c], batch.n[c] * sizeof(int32_t));
    return PCC_OK;
}

}  // namespace

// pcc_region_growing_rgb_batch behind its argument checks (both out arrays on the host)
int region_growing_rgb_batch(pcc_index* ix, const CloudBatch& batch, float distance_threshold, float point_color_threshold,
                             float region_color_threshold, uint32_t min_size, uint32_t max_size, unsigned int nr_neighbours,
                             unsigned int nr_region_neighbours, int32_t* out_labels, int32_t* out_n_clusters) {
    PCC_TRY(sync_info(ix));  // (a pending mirror of the handle's own grid would overwrite stats[2] later)
    RgbBatchScratch* b = scratch<RgbBatchScratch>(ix);
    const RgbParams par{distance_threshold, point_color_threshold, region_color_threshold, min_size, max_size, nr_neighbours, nr_region_neighbours};
    const size_t n_clouds = batch.n_clouds;
    const size_t brute_max = nr_region_neighbours <= RGB_BATCH_MAX_K ? (size_t)ix->opt.rgb_batch_brute_max : 0;
    const BatchRoutes routes = batch_routes(batch.n, n_clouds, brute_max);
    std::vector<size_t> off(n_clouds + 1, 0);
    for (size_t c = 0; c < n_clouds; ++c) off[c + 1] = off[c] + batch.n[c];
    CloudBatch small = batch;
    small.n = routes.small_n.data();
    PCC_TRY(rgb_batch_route(ix, small, par, off.data(), out_labels, out_n_clusters));
    ix->stats[2] = routes.n_brute;
    ix->stats[3] = routes.n_large;
    ix->stats_pending = false;
    ix->open_pending = false;
    if (routes.n_large == 0) return PCC_OK;

    // ---- the other clouds: one by one on the work handle ----------------------------------------------------------------------
    WorkLease lease;
    PCC_TRY(lease.take(ix, b->work, true));
    for (size_t c = 0; c < n_clouds; ++c) {
        if (batch.n[c] <= brute_max) continue;
        int32_t* labels = out_labels + off[c];
        if (!cloud_any_finite(batch.pts[c], batch.n[c], batch.stride)) {  // (the single path answers PCC_ERR_EMPTY there)
            std::fill(labels, labels + batch.n[c], (int32_t)-1);
            out_n_clusters[c] = 0;
            continue;
        }
        PCC_TRY(pcc_index_set_input(lease.w, batch.pts[c], batch.n[c], batch.stride, 3, PCC_MEM_HOST));
        PCC_TRY(pcc_region_growing_rgb(lease.w, batch.rgb[c], batch.rgb_stride, PCC_MEM_HOST, distance_threshold, point_color_threshold,
                                       region_color_threshold, min_size, max_size, nr_neighbours, nr_region_neighbours, labels, out_n_clusters + c));
    }
    return PCC_OK;
}

PCC_PAIRS_TAKE(rgb_batch)

}  // namespace pcc

extern "C" {

int pcc_region_growing_rgb_batch(pcc_index* ctx, size_t n_clouds, const void* const* pts, const size_t* n, size_t stride, const void* const* rgb,
                                 size_t rgb_stride, int mem, float distance_threshold, float point_color_threshold,
                                 float region_color_threshold, uint32_t min_size, uint32_t max_size, unsigned int nr_neighbours,
                                 unsigned int nr_region_neighbours, int32_t* out_labels, int32_t* out_n_clusters) {
    using namespace pcc;
    // the arguments first: all of it host arithmetic, refused before the handle or any device is looked at
    const CloudBatch batch{n_clouds, pts, n, stride, rgb, rgb_stride};
    PCC_TRY(check_cloud_batch("pcc_region_growing_rgb_batch", batch, mem));
    if (n_clouds >= (1ull << 31)) { set_error("more than 2^31 clouds"); return PCC_ERR_UNSUPPORTED; }
    if (n_clouds && (!pts || !n || !rgb || !out_labels || !out_n_clusters)) { set_error("null array argument"); return PCC_ERR_INVALID; }
    if (rgb_stride < 4 || rgb_stride % 4 || reinterpret_cast<uintptr_t>(out_labels) % 4 || reinterpret_cast<uintptr_t>(out_n_clusters) % 4) {
        set_error("colour words must be 4-byte aligned, stride %zu a multiple of 4 and >= 4", rgb_stride);
        return PCC_ERR_INVALID;
    }
    PCC_TRY(check_rgb_params(distance_threshold, point_color_threshold, region_color_threshold, nr_neighbours, nr_region_neighbours));
    PCC_TRY(check_batch_clouds(batch, mem));
    if (n_clouds == 0) return PCC_OK;  // (no device is touched: not even the handle's)
    PCC_ENTER(ctx);
    ev_next(ctx);
    ev_mark(ctx, EV_CALL0);
    const int st = region_growing_rgb_batch(ctx, batch, distance_threshold, point_color_threshold, region_color_threshold, min_size, max_size,
                                            nr_neighbours, nr_region_neighbours, out_labels, out_n_clusters);
    ev_mark(ctx, EV_CALL1);
    return st;
}
}  // extern "C"
