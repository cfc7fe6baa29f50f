// cluster_match.hip -- the cluster-matching loop of a comparison in one call (gfx950): pcc_cluster_matching.
//
// The reference walks the clusters of scene 1 (src/comparator.cpp:1296-1366): per cluster the three nearest free centroids of
// scene 2, two gates, matchRIFTFeaturesKnn for every pair that passes them and an acceptance rule on the NUMBER of
// correspondences -- the indices are never read.  Candidates, gates and acceptance are host arithmetic (cluster_match_plan.hpp);
// the searches of all pairs are one pass over the device:
//   1. pack: every cluster of either scene that takes part in a searched pair ONCE, as match_dims_plan.hpp's record (DP = 4, 8,
//      16 or 32 floats, zero padding, an invalid record as (+inf, 0, ...)).  From host memory on the host into the pinned
//      staging buffer (large scenes: by the host pipe's threads), one copy with the tables; from device memory by k_cm_pack
//      from the strided records.
//   2. k_cm_search: the shared search (match_plan.hpp's work items, match_search.hpp's workgroup) tracking the smallest distance
//      alone -- one query per lane with its DP floats in VGPRs, the references through wave-uniform loads, the waves of a
//      workgroup each taking a share of the slice, their minima meeting in LDS, the slices of a query block merging by a 32-bit
//      atomicMin on the distance bits.  No index, no second minimum, no tie order: equal distances are equal bits whichever
//      reference supplied them.
//   3. k_cm_count: one wave per searched pair counts the queries whose minimum is a neighbour below the threshold.
// One upload, one wait, one read-back of 3 * n_clusters1 words; launches and waits do not depend on the clusters or pairs.
//
// Arithmetic: FLANN's L2_Simple in index order, d = d0 * d0; d = d + d1 * d1; ..., every operation rounded on its own
// (-ffp-contract=off); the zero padding adds exact zeros, so DP = 4 at dim = 3 gives k_match_batch's distances.
#include <vector>

#include "entry.hpp"
#include "host_pipe.hpp"
#include "lane_ops.hpp"
#include "cluster_match_plan.hpp"
#include "match_search.hpp"

namespace pcc {

namespace {

constexpr size_t CM_PACK_CREW_MIN = 32768;  // records from which the host pack is shared out among threads (below: they cost more than they save)

// ---- 1. the pack from device memory ---------------------------------------------------------------------------------------------
// Packed record t belongs to the cloud c with clouds[c].rec0 <= t < clouds[c].rec0 + clouds[c].n (no cloud is empty): the first
// `dim` floats of record src0 + (t - rec0) of its scene's array, padded with zeros; not all finite: (+inf, 0, ...).
template <int DP>
__global__ void __launch_bounds__(256)
k_cm_pack(const unsigned char* __restrict__ des1, const unsigned char* __restrict__ des2, size_t stride, int dim,
          const ClusterMatchCloud* __restrict__ clouds, unsigned int n_clouds, unsigned int n_rec, float* __restrict__ out) {
    for (unsigned int t = blockIdx.x * blockDim.x + threadIdx.x; t < n_rec; t += gridDim.x * blockDim.x) {
        const ClusterMatchCloud cl = clouds[range_of_by(n_clouds, t, [clouds](unsigned int c) { return clouds[c].rec0; })];
        const unsigned char* base = cl.side ? des2 : des1;
        const float* __restrict__ src = reinterpret_cast<const float*>(base + (size_t)(cl.src0 + (t - cl.rec0)) * stride);
        float v[DP];
        bool valid = true;
#pragma unroll
        for (int k = 0; k < DP; ++k) {
            v[k] = k < dim ? src[k] : 0.0f;
            valid = valid && (v[k] - v[k]) == 0.0f;  // (finite: neither NaN nor +-inf)
        }
        float4* __restrict__ o = reinterpret_cast<float4*>(out + (size_t)t * DP);
#pragma unroll
        for (int k = 0; k < DP / 4; ++k)
            o[k] = valid ? make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3])
                         : make_float4(k == 0 ? __uint_as_float(0x7f800000u) : 0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// ---- 2. the search ------------------------------------------------------------------------------------------------------------
template <int DP>
__global__ void __launch_bounds__(MATCH_WAVES * 64, 8)
k_cm_search(const MatchItem* __restrict__ items, const float* __restrict__ rec, unsigned int* __restrict__ best) {
    __shared__ unsigned int sk[MATCH_WAVES][64];
    const MatchItem it = items[blockIdx.x];  // (block-uniform: scalar loads; ridx0 is not used: no index is reported)
    const MatchLane me = match_lane(it);
    float q[DP];
    match_load_query<DP>(rec, it, me, q);
    const MatchShare share = match_share(it.nr, me.wave);
    const float* __restrict__ refs = rec + (size_t)it.r0 * DP;
    unsigned int kd = 0xffffffffu;  // this wave's smallest distance bits
    // (a plain minimum is a reduction the compiler would interleave four iterations deep: 65 VGPRs spilled at DP = 32 under
    // these launch bounds; two iterations in order keep every width within 64 registers)
#pragma clang loop unroll_count(2) interleave(disable) vectorize(disable)
    for (unsigned int j = share.b0; j < share.b1; ++j) {  // (wave-uniform: the record arrives by scalar loads)
        const float* __restrict__ r = refs + (size_t)j * DP;
        const float t0 = q[0] - r[0];
        float d = t0 * t0;
#pragma unroll
        for (int k = 1; k < DP; ++k) {
            const float t = q[k] - r[k];
            d = d + t * t;
        }
        // (squares and their sums are never negative: the bits order as the distances do; an invalid record's +inf and a NaN
        // lie above every finite distance and are "no neighbour" to k_cm_count)
        kd = min(kd, __float_as_uint(d));
    }
    sk[me.wave][me.lane] = kd;
    __syncthreads();
    if (me.wave != 0) return;
#pragma unroll 4
    for (int w = 1; w < MATCH_WAVES; ++w) kd = min(kd, sk[w][me.lane]);
    if (me.live && kd != 0xffffffffu) atomicMin(best + it.qslot0 + me.lane, kd);
}

// ---- 3. the count -------------------------------------------------------------------------------------------------------------
// One wave per searched pair: counts[pair.out] = the queries whose minimum is a neighbour (below FLT_MAX: key_none) and
// < threshold.  The sum is wave-uniform (ballots); lane 0 stores it.
__global__ void __launch_bounds__(64)
k_cm_count(const ClusterMatchPair* __restrict__ pairs, unsigned int n_pairs, const unsigned int* __restrict__ best, float threshold,
           unsigned int* __restrict__ counts) {
    const unsigned int lane = threadIdx.x;
    for (unsigned int p = blockIdx.x; p < n_pairs; p += gridDim.x) {  // block-uniform
        const ClusterMatchPair pr = pairs[p];
        unsigned int total = 0;
        for (unsigned int q0 = 0; q0 < pr.nq; q0 += 64) {
            const unsigned int q = q0 + lane;
            bool hit = false;
            if (q < pr.nq) {
                const unsigned int b = best[pr.slot0 + q];
                hit = b < 0x7f7fffffu && __uint_as_float(b) < threshold;
            }
            total += (unsigned int)__popcll(__ballot(hit));
        }
        if (lane == 0) counts[pr.out] = total;
    }
}

struct ClusterMatchArgs {
    const unsigned char *des1, *des2;
    const size_t *offsets1, *offsets2;
    size_t n_clusters1, n_clusters2, stride;
    int dim, mem;
    float threshold;
};

// the searches of the pairs in state CM_SEARCHED: correspondences[e] = 1 + the count of pair e (e = 3 * i + k)
int cluster_match_search(pcc_index* ix, const ClusterMatchArgs& a, const ClusterMatchLayout& L, int dp, uint32_t* correspondences) {
    MatchBatchScratch* mb = scratch<MatchBatchScratch>(ix);
    hipStream_t s = ix->stream;
    const bool host = a.mem == PCC_MEM_HOST;
    const size_t n_items = L.items.size(), n_pairs = L.pairs.size(), n_clouds = L.clouds.size(), n_out = 3 * a.n_clusters1;
    const size_t pairs_at = align_up(n_items * sizeof(MatchItem), 16), clouds_at = pairs_at + align_up(n_pairs * sizeof(ClusterMatchPair), 16);
    const size_t rec_at = clouds_at + align_up(n_clouds * sizeof(ClusterMatchCloud), 16);
    const size_t rec_bytes = L.n_rec * (size_t)dp * sizeof(float), all_bytes = rec_at + rec_bytes;
    const size_t counts_at = align_up(L.n_slots * sizeof(unsigned int), 16), res_bytes = counts_at + n_out * sizeof(unsigned int);
    PCC_TRY(mb->up.reserve((host ? all_bytes : rec_at) + 16));
    PCC_TRY(mb->dev.reserve(all_bytes + 16));
    PCC_TRY(mb->res.reserve(res_bytes + 16));
    PCC_TRY(mb->down.reserve(n_out * sizeof(unsigned int) + 16));
    char* u = mb->up.as<char>();
    memcpy(u, L.items.data(), n_items * sizeof(MatchItem));
    memcpy(u + pairs_at, L.pairs.data(), n_pairs * sizeof(ClusterMatchPair));
    memcpy(u + clouds_at, L.clouds.data(), n_clouds * sizeof(ClusterMatchCloud));
    char* d0 = mb->dev.as<char>();
    const MatchItem* d_items = reinterpret_cast<const MatchItem*>(d0);
    const ClusterMatchPair* d_pairs = reinterpret_cast<const ClusterMatchPair*>(d0 + pairs_at);
    const ClusterMatchCloud* d_clouds = reinterpret_cast<const ClusterMatchCloud*>(d0 + clouds_at);
    float* d_rec = reinterpret_cast<float*>(d0 + rec_at);
    unsigned int* d_best = mb->res.as<unsigned int>();
    unsigned int* d_counts = reinterpret_cast<unsigned int*>(mb->res.as<char>() + counts_at);

    // ---- one upload, the launches, one read-back, one wait ------------------------------------------------------------------------
    if (host) {
        // (the pack reads every strided record -- 100 MB for 800 000 RIFT32 -- and is what a call from host memory spends its time
        // on: from CM_PACK_CREW_MIN records on the clusters are shared out among the host pipe's threads, by their place in the
        // packed array; same bytes)
        float* rec = reinterpret_cast<float*>(u + rec_at);
        auto pack = [&](size_t, int tid, int nthreads) {
            for (const ClusterMatchCloud& c : L.clouds)
                if ((int)((uint64_t)c.rec0 * (uint64_t)nthreads / L.n_rec) == tid)
                    match_dims_pack((c.side ? a.des2 : a.des1) + (size_t)c.src0 * a.stride, c.n, a.stride, a.dim, dp, rec + (size_t)c.rec0 * dp);
        };
        if (L.n_rec >= CM_PACK_CREW_MIN) {
            ChunkCrew crew(pipe_threads(), pack);
            crew.run(0, pack);
        } else {
            pack(0, 0, 1);
        }
        PCC_HIP(hipMemcpyAsync(d0, u, all_bytes, hipMemcpyHostToDevice, s));
    } else {
        PCC_HIP(hipMemcpyAsync(d0, u, rec_at, hipMemcpyHostToDevice, s));
        const dim3 grid(blocks_for(L.n_rec)), wg(256);
        const unsigned int nc = (unsigned int)n_clouds, nr = (unsigned int)L.n_rec;
        dispatch_dp(dp, [&](auto DP) {
            hipLaunchKernelGGL((k_cm_pack<decltype(DP)::value>), grid, wg, 0, s, a.des1, a.des2, a.stride, a.dim, d_clouds, nc, nr, d_rec);
        });
        PCC_HIP(hipGetLastError());
    }
    PCC_HIP(hipMemsetAsync(d_best, 0xff, L.n_slots * sizeof(unsigned int), s));
    dispatch_dp(dp, [&](auto DP) {
        hipLaunchKernelGGL((k_cm_search<decltype(DP)::value>), dim3((unsigned int)n_items), dim3(MATCH_WAVES * 64), 0, s, d_items, d_rec, d_best);
    });
    PCC_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_cm_count, dim3((unsigned int)std::min<size_t>(n_pairs, 4096)), dim3(64), 0, s, d_pairs, (unsigned int)n_pairs, d_best,
                       a.threshold, d_counts);
    PCC_HIP(hipGetLastError());
    PCC_HIP(hipMemcpyAsync(mb->down.p, d_counts, n_out * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
    PCC_HIP(hipStreamSynchronize(s));
    const unsigned int* h_counts = mb->down.as<unsigned int>();
    for (const ClusterMatchPair& p : L.pairs) correspondences[p.out] = 1u + h_counts[p.out];  // (the dummy first element, :568)
    return PCC_OK;
}

void cluster_match_stats(pcc_index* ix, const ClusterMatchLayout& L) {
    ix->stats[0] = L.pairs.size();
    ix->stats[1] = L.n_slots;
    own_counters(ix, 0);
}

}  // namespace

}  // namespace pcc

extern "C" {

int pcc_cluster_matching(pcc_index* ctx, const void* des1, const size_t* offsets1, size_t n_clusters1, const void* des2, const size_t* offsets2,
                         size_t n_clusters2, size_t stride_bytes, int dim, int mem, const float* centroids1, const float* centroids2,
                         const size_t* points1, const size_t* points2, float threshold, int32_t* out_candidates, int32_t* out_state,
                         uint32_t* out_correspondences, int32_t* out_matches) {
    using namespace pcc;
    // the arguments first: all of it host arithmetic, refused before the handle or any device is looked at
    // 1. the width
    if (dim < 1 || dim > MD_DIM_MAX) { set_error("descriptor matching searches 1 ... 32 dimensions, not %d", dim); return PCC_ERR_UNSUPPORTED; }
    // 2. the memory space
    PCC_TRY(check_mem(mem));
    // 3. null arrays (a scene's arrays may be null while it has no cluster, its descriptors while none of its clusters holds a record)
    if (n_clusters1 && (!offsets1 || !centroids1 || !points1 || !out_candidates || !out_state || !out_correspondences || !out_matches)) {
        set_error("null argument");
        return PCC_ERR_INVALID;
    }
    if (n_clusters2 && (!offsets2 || !centroids2 || !points2)) { set_error("null argument"); return PCC_ERR_INVALID; }
    if ((n_clusters1 && offsets1[n_clusters1] != offsets1[0] && !des1) || (n_clusters2 && offsets2[n_clusters2] != offsets2[0] && !des2)) {
        set_error("null argument");
        return PCC_ERR_INVALID;
    }
    // 4. the stride and the alignment
    if (stride_bytes < 4 * (size_t)dim || stride_bytes % 4) {
        set_error("stride %zu must be a multiple of 4 and >= %d", stride_bytes, 4 * dim);
        return PCC_ERR_INVALID;
    }
    if (reinterpret_cast<uintptr_t>(des1) % 4 || reinterpret_cast<uintptr_t>(des2) % 4) { set_error("descriptors must be 4-byte aligned"); return PCC_ERR_INVALID; }
    // 5. the offsets
    PCC_TRY(check_cluster_offsets({{offsets1, n_clusters1}, {offsets2, n_clusters2}}, "descriptors in one scene"));
    // 6. the threshold: pcc_match_knn_batch_dims refuses none (a NaN threshold counts nothing)
    if (n_clusters1 == 0) return PCC_OK;  // (nothing to write, no device is touched: not even the handle's)
    // 7. the handle
    if (!ctx) { set_error("null index"); return PCC_ERR_INVALID; }

    const size_t n_out = 3 * n_clusters1;
    std::vector<int32_t> candidates(n_out), state(n_out), matches(n_clusters1);
    std::vector<uint32_t> correspondences(n_out, 0u);
    cm_candidates(centroids1, n_clusters1, centroids2, n_clusters2, candidates.data());
    cm_states(candidates.data(), n_clusters1, offsets1, offsets2, points1, points2, state.data());
    const int dp = match_dims_padded(dim);
    ClusterMatchLayout L;
    if (!cm_layout(candidates.data(), state.data(), n_clusters1, n_clusters2, offsets1, offsets2, dp, &L)) {
        set_error("more than 2^31 - 1 records, queries or work items in one call");
        return PCC_ERR_UNSUPPORTED;
    }
    if (L.pairs.empty()) {  // (nothing to search: the handle's counters alone, no device)
        HandleLock lock(ctx->mu);
        cluster_match_stats(ctx, L);
    } else {
        PCC_ENTER(ctx);
        ev_next(ctx);
        ev_mark(ctx, EV_CALL0);
        const ClusterMatchArgs a{static_cast<const unsigned char*>(des1), static_cast<const unsigned char*>(des2), offsets1, offsets2, n_clusters1,
                                 n_clusters2, stride_bytes, dim, mem, threshold};
        const int st = cluster_match_search(ctx, a, L, dp, correspondences.data());
        ev_mark(ctx, EV_CALL1);
        PCC_TRY(st);
        cluster_match_stats(ctx, L);
    }
    cm_accept(candidates.data(), state.data(), correspondences.data(), n_clusters1, offsets1, offsets2, matches.data());
    memcpy(out_candidates, candidates.data(), n_out * sizeof(int32_t));
    memcpy(out_state, state.data(), n_out * sizeof(int32_t));
    memcpy(out_correspondences, correspondences.data(), n_out * sizeof(uint32_t));
    memcpy(out_matches, matches.data(), n_clusters1 * sizeof(int32_t));
    return PCC_OK;
}
}  // extern "C"
