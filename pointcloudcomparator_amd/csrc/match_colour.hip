// match_colour.hip -- the colour counts of a comparison's match loop in one call (gfx950): pcc_match_colour_elements.
//
// The reference's match loop (src/comparator.cpp:1379-1509) runs color_growing_segmentation (src/segmentation.cpp:161-216) on both
// clusters of every accepted match and keeps the NUMBER of colour segments of each (:1456-1495).  pcc_region_growing_rgb_batch is
// the batched form of that loop for host clouds, one pointer per cloud, every label brought back.  Here the clusters are what the
// segmentation calls write -- records behind one another with offsets, in host or device memory --, the match table says which
// of them are wanted, and only the counts come back:
//   plan   : match_colour_plan.hpp: every distinct (scene, cluster) the table names ONCE, in first-use order; clusters of up to
//            PCC_OPT_RGB_BATCH_BRUTE_MAX records form the concatenation of the batch route, larger ones take the work handle
//   pack   : k_mc_pack builds the concatenation region_rgb_batch.hip's row kernel and rgb_stages.hpp read -- float4 with
//            w = bits(concatenated index), negative for a non-finite point, the colour word beside it -- from the strided
//            records, one launch for all clusters, and counts the finite points of every cluster (the reference's gate of more
//            than 10 points applies after removeNaNFromPointCloud).  Host memory: the records of the named clusters ride in the
//            one pinned upload that carries the tables, and the same kernel packs them
//   rows   : k_rgb_batch_knn (rgb_batch_rows), unchanged
//   stages : rgb_stages in its counts-only form: no cluster id goes up, no label is written or copied
//   host   : rgb_batch_split per cloud, the gate from the finite counts, the table filled through the plan's map.
// What crosses to the host is what rgb_stages brings (words per sweep, segment records, the pair list, the clouds' first ids)
// and one finite count per cluster, copied behind the pack and complete at the first sweep's wait.  From device memory no point
// or colour crosses in either direction.  Launches and waits depend on the label sweeps, not on clusters or matches.
#include <algorithm>
#include <vector>

#include "entry.hpp"
#include "cloud_batch.hpp"
#include "lane_ops.hpp"
#include "match_colour_plan.hpp"
#include "rgb_batch_split.hpp"
#include "rgb_stages.hpp"

namespace pcc {

namespace {

// cloud `slot` of the concatenation: points base .. base + n are records src0 .. src0 + n of scene `side`'s arrays
struct McCloud {
    uint32_t base, n, side, pad;
    uint64_t src0, pad1;
};

// ---- the pack -------------------------------------------------------------------------------------------------------------------
// One thread per point of the concatenation, consecutive threads on consecutive records: a wave reads 64 records of `stride`
// bytes behind one another (V16: x, y, z in one 16-byte load) and writes 1 KB of points and 256 B of colour words densely.  The
// cloud of point t is the last one with base <= t (an empty cloud shares its base with the next one and is never chosen).
// finite[slot] += the finite points: lanes of a wave that share a cloud add their number with one atomic.
template <bool V16>
__global__ void __launch_bounds__(256)
k_mc_pack(const unsigned char* __restrict__ pts1, const unsigned char* __restrict__ pts2, size_t stride, const unsigned char* __restrict__ rgb1,
          const unsigned char* __restrict__ rgb2, size_t rgb_stride, const McCloud* __restrict__ clouds, unsigned int n_clouds, unsigned int total,
          float4* __restrict__ out, unsigned int* __restrict__ words, unsigned int* __restrict__ finite) {
    const unsigned int lane = threadIdx.x & 63;
    for (unsigned int t0 = blockIdx.x * blockDim.x; t0 < total; t0 += gridDim.x * blockDim.x) {  // block-uniform: whole waves reach the ballots
        const unsigned int t = t0 + threadIdx.x;
        const bool live = t < total;
        unsigned int lo = 0;
        bool fin = false;
        if (live) {
            lo = range_of_by(n_clouds, t, [clouds](unsigned int c) { return clouds[c].base; });
            const McCloud cl = clouds[lo];
            const size_t rec = (size_t)cl.src0 + (t - cl.base);
            const unsigned char* p = (cl.side ? pts2 : pts1) + rec * stride;
            float x, y, z;
            if (V16) {
                const float4 v = *reinterpret_cast<const float4*>(p);
                x = v.x; y = v.y; z = v.z;
            } else {
                const float* f = reinterpret_cast<const float*>(p);
                x = f[0]; y = f[1]; z = f[2];
            }
            fin = finite3(x, y, z);
            out[t] = make_float4(x, y, z, __uint_as_float(fin ? t : 0xffffffffu));
            words[t] = *reinterpret_cast<const unsigned int*>((cl.side ? rgb2 : rgb1) + rec * rgb_stride);
        }
        unsigned long long todo = __ballot(live && fin);  // wave-uniform
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const unsigned int lc = (unsigned int)__shfl((int)lo, leader);
            const unsigned long long same = __ballot(live && fin && lo == lc);
            if ((int)lane == leader) atomicAdd(finite + lc, (unsigned int)__popcll(same));
            todo &= ~same;
        }
    }
}

}  // namespace

// (up: bases + items + cloud table, and from host memory the named clusters' records; down: the clouds' first ids + finite counts)
struct MatchColourScratch : BatchStaging {
    static constexpr ScratchSlot slot = SCRATCH_MATCH_COLOUR;
    DevBuf cat;                       // the concatenation: float4[total], then uint32[total] colour words
    DevBuf keys;                      // u64[total][K]: the rows
    DevBuf id_bases, finite, labels;  // uint32[n_clouds + 1]; uint32[n_clouds]; int32: the labels of a cluster on the work handle
};

namespace {

struct McArgs {
    const unsigned char *pts[2], *rgb[2];
    size_t stride, rgb_stride;
    int mem;
    size_t min_points;
    float distance_threshold, point_color_threshold, region_color_threshold;
    uint32_t min_size, max_size;
    unsigned int nr_neighbours, nr_region_neighbours;
};

// count_of_cluster[e]: the colour elements of P.clusters[e]
int match_colour_elements(pcc_index* ix, const McArgs& a, const MatchColourPlan& P, int32_t* count_of_cluster) {
    hipStream_t s = ix->stream;
    PCC_TRY(sync_info(ix));  // (a pending mirror of the handle's own grid would overwrite stats[2] later)
    MatchColourScratch* sc = scratch<MatchColourScratch>(ix);
    const size_t n_list = P.clusters.size(), n_clouds = P.batch_n.size(), total = P.n_batch_points, n_items = P.items.size();
    const bool host = a.mem == PCC_MEM_HOST;
    const int K = (int)a.nr_region_neighbours;
    if (total * (size_t)K >= ((size_t)1 << 32)) {
        set_error("%zu x %d row entries in one batch: 2^32 and more are not built -- split the call", total, K);
        return PCC_ERR_UNSUPPORTED;
    }

    // ---- one pinned buffer, one copy: bases | items | cloud table | host memory: the named clusters' records, colour words -------
    // The records of the named clusters follow one another at their stride, so a cluster's place is a record index as in the
    // caller's arrays.  Colour words inside the point records (rgb = pts + delta, the same stride) ride with them; else they
    // are staged the same way behind the points.
    const size_t items_at = align_up((n_clouds + 1) * sizeof(uint32_t), 16), table_at = items_at + n_items * sizeof(RiftBatchItem);
    const size_t rec_at = align_up(table_at + n_clouds * sizeof(McCloud), 16);
    bool inside = host && a.rgb_stride == a.stride;
    size_t delta = 0;
    if (inside) {
        bool first = true;
        for (const MatchColourCluster& m : P.clusters) {
            if (m.n == 0) continue;
            const uintptr_t p = reinterpret_cast<uintptr_t>(a.pts[m.scene]), c = reinterpret_cast<uintptr_t>(a.rgb[m.scene]);
            const size_t d = c >= p ? (size_t)(c - p) : a.stride;
            if (d + 4 > a.stride || (!first && d != delta)) { inside = false; break; }
            delta = d;
            first = false;
        }
    }
    std::vector<uint64_t> staged0(n_list, 0);  // host memory: the first staged record of every named cluster
    size_t n_staged = 0;
    if (host)
        for (size_t e = 0; e < n_list; ++e) { staged0[e] = n_staged; n_staged += P.clusters[e].n; }
    const size_t col_at = rec_at + align_up(n_staged * a.stride, 16), up_bytes = !host ? rec_at : (inside ? col_at : col_at + align_up(n_staged * a.rgb_stride, 16));
    PCC_TRY(sc->up.reserve(up_bytes + 16));
    PCC_TRY(sc->dev.reserve(up_bytes + 16));
    char* u = sc->up.as<char>();
    char* d0 = sc->dev.as<char>();
    memcpy(u, P.bases.data(), (n_clouds + 1) * sizeof(uint32_t));
    if (n_items) memcpy(u + items_at, P.items.data(), n_items * sizeof(RiftBatchItem));
    McCloud* table = reinterpret_cast<McCloud*>(u + table_at);
    for (size_t e = 0; e < n_list; ++e) {
        const MatchColourCluster& m = P.clusters[e];
        if (m.route == MC_BATCH) table[m.slot] = McCloud{m.base, m.n, host ? 0u : m.scene, 0u, host ? staged0[e] : m.src0, 0u};
        if (!host || m.n == 0) continue;
        const size_t tail = inside ? std::max<size_t>(12, delta + 4) : 12;  // (the last record of an array need not be a whole stride)
        memcpy(u + rec_at + staged0[e] * a.stride, a.pts[m.scene] + m.src0 * a.stride, (size_t)(m.n - 1) * a.stride + tail);
        if (!inside) memcpy(u + col_at + staged0[e] * a.rgb_stride, a.rgb[m.scene] + m.src0 * a.rgb_stride, (size_t)(m.n - 1) * a.rgb_stride + 4);
    }
    // (nothing but empty clusters: nothing goes up, and no copy is left reading `u` behind the call's back)
    if (total || n_staged) PCC_HIP(hipMemcpyAsync(d0, u, up_bytes, hipMemcpyHostToDevice, s));
    // the arrays the device reads the clusters from: the caller's own, or what has just gone up
    const unsigned char* d_pts[2] = {a.pts[0], a.pts[1]};
    const unsigned char* d_rgb[2] = {a.rgb[0], a.rgb[1]};
    if (host) {
        d_pts[0] = d_pts[1] = reinterpret_cast<const unsigned char*>(d0 + rec_at);
        d_rgb[0] = d_rgb[1] = inside ? d_pts[0] + delta : reinterpret_cast<const unsigned char*>(d0 + col_at);
    }

    // ---- the batch route ---------------------------------------------------------------------------------------------------------
    std::vector<int32_t> n_clusters(n_clouds, 0);
    const unsigned int* h_finite = nullptr;
    ix->stats[0] = ix->stats[1] = ix->stats[7] = 0;
    if (total) {
        const unsigned int* d_bases = reinterpret_cast<const unsigned int*>(d0);
        const RiftBatchItem* d_items = reinterpret_cast<const RiftBatchItem*>(d0 + items_at);
        const McCloud* d_table = reinterpret_cast<const McCloud*>(d0 + table_at);
        const size_t words_at = total * sizeof(float4);
        PCC_TRY(sc->cat.reserve(words_at + total * sizeof(uint32_t)));
        PCC_TRY(sc->finite.reserve(n_clouds * sizeof(unsigned int)));
        PCC_TRY(sc->id_bases.reserve((n_clouds + 1) * sizeof(unsigned int)));
        PCC_TRY(sc->keys.reserve(total * (size_t)K * sizeof(unsigned long long)));
        const size_t ids_bytes = align_up((n_clouds + 1) * sizeof(unsigned int), 16);
        PCC_TRY(sc->down.reserve(ids_bytes + n_clouds * sizeof(unsigned int)));
        float4* d_cat = sc->cat.as<float4>();
        unsigned int* d_words = reinterpret_cast<unsigned int*>(sc->cat.as<char>() + words_at);
        unsigned int* d_finite = sc->finite.as<unsigned int>();
        unsigned int* h_fin = reinterpret_cast<unsigned int*>(sc->down.as<char>() + ids_bytes);
        PCC_HIP(hipMemsetAsync(d_finite, 0, n_clouds * sizeof(unsigned int), s));
        const dim3 grid(blocks_for(total)), wg(256);
        const bool v16 = a.stride % 16 == 0 && reinterpret_cast<uintptr_t>(d_pts[0]) % 16 == 0 && reinterpret_cast<uintptr_t>(d_pts[1]) % 16 == 0;
        if (v16)
            hipLaunchKernelGGL(k_mc_pack<true>, grid, wg, 0, s, d_pts[0], d_pts[1], a.stride, d_rgb[0], d_rgb[1], a.rgb_stride, d_table,
                               (unsigned int)n_clouds, (unsigned int)total, d_cat, d_words, d_finite);
        else
            hipLaunchKernelGGL(k_mc_pack<false>, grid, wg, 0, s, d_pts[0], d_pts[1], a.stride, d_rgb[0], d_rgb[1], a.rgb_stride, d_table,
                               (unsigned int)n_clouds, (unsigned int)total, d_cat, d_words, d_finite);
        PCC_HIP(hipGetLastError());
        // (no wait of its own: the counts are down when the first label sweep's words are)
        PCC_HIP(hipMemcpyAsync(h_fin, d_finite, n_clouds * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
        h_finite = h_fin;
        unsigned long long* keys = sc->keys.as<unsigned long long>();
        PCC_TRY(rgb_batch_rows(ix, d_items, (unsigned int)n_items, d_cat, K, keys));
        RgbRun run;
        run.refs = d_cat;
        run.n = (unsigned int)total;
        run.keys = keys;
        run.K = K;
        run.rgb = reinterpret_cast<const unsigned char*>(d_words);
        run.rgb_stride = sizeof(uint32_t);
        run.point_color_threshold = a.point_color_threshold;
        run.nr_neighbours = a.nr_neighbours;
        run.d_bases = d_bases;
        run.n_clouds = (unsigned int)n_clouds;
        run.d_id_bases = sc->id_bases.as<unsigned int>();
        run.h_id_bases = sc->down.as<unsigned int>();
        run.labels_dev = nullptr;  // counts only
        const float dist2 = a.distance_threshold * a.distance_threshold, r2r2 = a.region_color_threshold * a.region_color_threshold;
        const int min_pts = (int)std::min<uint32_t>(a.min_size, 0x7fffffffu), max_pts = (int)std::min<uint32_t>(a.max_size, 0x7fffffffu);
        PCC_TRY(rgb_stages(ix, run, [&](const RgbSegment* segs, unsigned int ns, RgbSegmentPair* pairs, unsigned int np, std::vector<int32_t>& cluster_of_segment) {
            if (!rgb_batch_split(segs, ns, pairs, np, run.h_id_bases, n_clouds, dist2, r2r2, a.nr_region_neighbours, min_pts, max_pts,
                                 cluster_of_segment, n_clusters.data())) {
                set_error("colour region growing: a segment pair crosses two clusters of the call");
                return (int)PCC_ERR_DEVICE;
            }
            return (int)PCC_OK;
        }));
    }
    for (size_t e = 0; e < n_list; ++e) {
        const MatchColourCluster& m = P.clusters[e];
        if (m.route != MC_BATCH) continue;
        // the reference's gate (src/segmentation.cpp:164-167): more than min_points points after the NaN strip
        count_of_cluster[e] = (h_finite && (size_t)h_finite[m.slot] > a.min_points) ? n_clusters[m.slot] : 0;
    }
    ix->stats[2] = P.n_batch_points;
    ix->stats[3] = P.n_work_points;
    ix->stats[4] = n_list;
    ix->open_pending = false;
    own_counters(ix, P.n_saved);
    if (P.n_work == 0) return PCC_OK;

    // ---- the other clusters: one by one on the work handle, from the device arrays, their labels to device scratch ----------------
    WorkLease lease;
    PCC_TRY(lease.take(ix, sc->work, true));
    for (size_t e = 0; e < n_list; ++e) {
        const MatchColourCluster& m = P.clusters[e];
        if (m.route != MC_WORK) continue;
        const size_t rec = host ? (size_t)staged0[e] : (size_t)m.src0;
        PCC_TRY(sc->labels.reserve((size_t)m.n * sizeof(int32_t)));
        PCC_TRY(pcc_index_set_input(lease.w, d_pts[m.scene] + rec * a.stride, m.n, a.stride, 3, PCC_MEM_DEVICE));
        int32_t found = 0;
        const int st = pcc_region_growing_rgb(lease.w, d_rgb[m.scene] + rec * a.rgb_stride, a.rgb_stride, PCC_MEM_DEVICE, a.distance_threshold,
                                              a.point_color_threshold, a.region_color_threshold, a.min_size, a.max_size, a.nr_neighbours,
                                              a.nr_region_neighbours, sc->labels.as<int32_t>(), &found);
        if (st == PCC_ERR_EMPTY) { count_of_cluster[e] = 0; continue; }  // (no finite point: below every gate)
        PCC_TRY(st);
        count_of_cluster[e] = lease.w->n_valid > a.min_points ? found : 0;
    }
    return PCC_OK;
}

}  // namespace

}  // namespace pcc

extern "C" {

int pcc_match_colour_elements(pcc_index* ctx, const void* pts1, const void* rgb1, const size_t* offsets1, size_t n_clusters1, const void* pts2,
                              const void* rgb2, const size_t* offsets2, size_t n_clusters2, size_t stride_bytes, size_t rgb_stride_bytes, int mem,
                              const int32_t* matches, size_t min_points, float distance_threshold, float point_color_threshold,
                              float region_color_threshold, uint32_t min_size, uint32_t max_size, unsigned int nr_neighbours,
                              unsigned int nr_region_neighbours, int32_t* out_elements) {
    using namespace pcc;
    // the arguments first: all of it host arithmetic, refused before the handle or any device is looked at
    // 1. the memory space
    PCC_TRY(check_mem(mem));
    // 2. null arrays (a scene's offsets may be null while it has no cluster -- matches and the output go with scene 1 --, its points
    //    and colours while no matched cluster of it holds a record)
    if (n_clusters1 && (!offsets1 || !matches || !out_elements)) { set_error("null argument"); return PCC_ERR_INVALID; }
    if (n_clusters2 && !offsets2) { set_error("null argument"); return PCC_ERR_INVALID; }
    for (size_t i = 0; i < n_clusters1; ++i) {
        if (matches[i] < 0 || (size_t)matches[i] >= n_clusters2) continue;  // (5. refuses what lies outside)
        const size_t j = (size_t)matches[i];
        if ((offsets1[i + 1] != offsets1[i] && (!pts1 || !rgb1)) || (offsets2[j + 1] != offsets2[j] && (!pts2 || !rgb2))) {
            set_error("null argument");
            return PCC_ERR_INVALID;
        }
    }
    // 3. the strides and the alignment, by pcc_region_growing_rgb_batch's rules
    PCC_TRY(check_points(nullptr, 0, stride_bytes, mem));  // (the stride alone)
    if (rgb_stride_bytes < 4 || rgb_stride_bytes % 4 || reinterpret_cast<uintptr_t>(out_elements) % 4) {
        set_error("colour words must be 4-byte aligned, stride %zu a multiple of 4 and >= 4", rgb_stride_bytes);
        return PCC_ERR_INVALID;
    }
    for (const void* p : {pts1, pts2, rgb1, rgb2})
        if (reinterpret_cast<uintptr_t>(p) % 4) {
            set_error("points and colour words must be 4-byte aligned, the colour stride %zu a multiple of 4 and >= 4", rgb_stride_bytes);
            return PCC_ERR_INVALID;
        }
    // 4. the offsets
    PCC_TRY(check_cluster_offsets({{offsets1, n_clusters1}, {offsets2, n_clusters2}}, "points in one scene"));
    // 5. the match table
    bool any = false;
    for (size_t i = 0; i < n_clusters1; ++i) {
        if (matches[i] < -1 || (matches[i] >= 0 && (size_t)matches[i] >= n_clusters2)) {
            set_error("matches[%zu] = %d names no cluster of scene 2 (%zu clusters; -1: no match)", i, (int)matches[i], n_clusters2);
            return PCC_ERR_INVALID;
        }
        any = any || matches[i] >= 0;
    }
    // 6. the parameters
    PCC_TRY(check_rgb_params(distance_threshold, point_color_threshold, region_color_threshold, nr_neighbours, nr_region_neighbours));
    if (n_clusters1 == 0) return PCC_OK;  // (nothing to write, no device is touched: not even the handle's)
    if (!any) {                           // (nothing to segment: the same)
        std::fill(out_elements, out_elements + 2 * n_clusters1, (int32_t)-1);
        return PCC_OK;
    }
    // 7. the handle
    PCC_ENTER(ctx);
    const size_t brute_max = nr_region_neighbours <= RGB_BATCH_MAX_K ? (size_t)ctx->opt.rgb_batch_brute_max : 0;
    MatchColourPlan plan;
    if (!mc_plan(matches, n_clusters1, offsets1, n_clusters2, offsets2, brute_max, &plan)) {
        set_error("more than 2^31 - 1 points on the batch route -- split the call");
        return PCC_ERR_UNSUPPORTED;
    }
    const McArgs a{{static_cast<const unsigned char*>(pts1), static_cast<const unsigned char*>(pts2)},
                   {static_cast<const unsigned char*>(rgb1), static_cast<const unsigned char*>(rgb2)},
                   stride_bytes, rgb_stride_bytes, mem, min_points, distance_threshold, point_color_threshold, region_color_threshold,
                   min_size, max_size, nr_neighbours, nr_region_neighbours};
    std::vector<int32_t> count_of_cluster(plan.clusters.size(), 0);
    ev_next(ctx);
    ev_mark(ctx, EV_CALL0);
    const int st = match_colour_elements(ctx, a, plan, count_of_cluster.data());
    ev_mark(ctx, EV_CALL1);
    PCC_TRY(st);
    mc_fill(plan, count_of_cluster.data(), n_clusters1, out_elements);
    return PCC_OK;
}
}  // extern "C"
