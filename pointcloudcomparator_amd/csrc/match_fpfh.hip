// match_fpfh.hip -- pcc_match_fpfh_batch (gfx950): the reference's matchFPFH (src/comparator.cpp:877-910) for every pair of
// descriptor arrays at once, on the 33 bins of a pcl::FPFHSignature33, from host or from device memory.
//
// The search is k_match_dims' (match_dims.hip) on a record of MF_DP = 36 floats (match_fpfh_plan.hpp): match_plan.hpp's work items,
// match_search.hpp's workgroup -- one query per lane with its 36 floats in VGPRs for the length of the item, the references
// through wave-uniform (scalar) loads shared by the 64 lanes, the waves of a workgroup each taking a share of the slice, partial
// minima meeting in LDS, the slices of a query block merging in device memory by
//   best[q] = atomicMin of (bits(d2) << 32 | index),  second[q] = atomicMin of bits(d2) of every loser.
// An invalid record is (+inf, 0, ...): no test on the record in the loop.
//
// From device memory the records are packed on the device (k_match_fpfh_pack) from the caller's strided arrays, driven by a small
// uploaded table of (pointer, n, first packed record) per distinct array; from host memory they are packed on the host into the
// pinned staging buffer and go up with the table of work items.  Either way: one upload, one search launch, one read-back, one
// wait, whatever n_pairs is.
//
// Arithmetic: FLANN's L2_Simple in index order, d = d0 * d0; d = d + d1 * d1; ..., every operation rounded on its own
// (-ffp-contract=off).  The order is part of the result.  Among references at exactly the same distance the lowest index
// wins whatever tie order the handle has, as in match_dims.hip: there is no N-D FLANN tree to check a visit order against.
#include "entry.hpp"
#include "lane_ops.hpp"
#include "match_fpfh_plan.hpp"
#include "match_search.hpp"

namespace pcc {

// ---- the pack from device memory ------------------------------------------------------------------------------------------------
// Packed record t belongs to the source s with sources[s].rec0 <= t < sources[s].rec0 + sources[s].n (no source is empty): the 33
// floats of record t - rec0 of that array, then three zeros; not all finite: (+inf, 0, ...).
__global__ void __launch_bounds__(256)
k_match_fpfh_pack(const MatchFpfhSource* __restrict__ sources, unsigned int n_sources, size_t stride, unsigned int n_rec,
                  float* __restrict__ out) {
    for (unsigned int t = blockIdx.x * blockDim.x + threadIdx.x; t < n_rec; t += gridDim.x * blockDim.x) {
        const MatchFpfhSource sc = sources[range_of_by(n_sources, t, [sources](unsigned int s) { return sources[s].rec0; })];
        const float* __restrict__ src = reinterpret_cast<const float*>(static_cast<const unsigned char*>(sc.p) + (size_t)(t - sc.rec0) * stride);
        float v[MF_DP];
        bool valid = true;
#pragma unroll
        for (int k = 0; k < MF_DP; ++k) {
            v[k] = k < MF_DIM ? src[k] : 0.0f;
            valid = valid && (v[k] - v[k]) == 0.0f;  // (finite: neither NaN nor +-inf)
        }
        float4* __restrict__ o = reinterpret_cast<float4*>(out + (size_t)t * MF_DP);
#pragma unroll
        for (int k = 0; k < MF_DP / 4; ++k)
            o[k] = valid ? make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3])
                         : make_float4(k == 0 ? __uint_as_float(0x7f800000u) : 0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// ---- the search -----------------------------------------------------------------------------------------------------------------
// (8 waves a SIMD, two workgroups a CU, at most 64 VGPRs, as k_match_dims: the compiler's remarks give 60 VGPRs and no scratch
// with the 36 query floats resident -- DESIGN.md 4.27)
__global__ void __launch_bounds__(MATCH_WAVES * 64, 8)
k_match_fpfh(const MatchItem* __restrict__ items, const float* __restrict__ rec, unsigned long long* __restrict__ best,
             unsigned int* __restrict__ second) {
    constexpr int DP = MF_DP;
    __shared__ unsigned long long sk[MATCH_WAVES][64];
    __shared__ unsigned int ss[MATCH_WAVES][64];
    const MatchItem it = items[blockIdx.x];  // (block-uniform: scalar loads)
    const MatchLane me = match_lane(it);
    const unsigned int lane = me.lane, wave = me.wave;
    const bool live = me.live;
    float q[DP];
    match_load_query<DP>(rec, it, me, q);
    const MatchShare share = match_share(it.nr, wave);
    const float* __restrict__ refs = rec + (size_t)it.r0 * DP;
    // this wave's minimum as (distance bits, position) and the second-smallest distance bits it met (with multiplicity)
    unsigned int kd = 0xffffffffu, ki = 0xffffffffu, s2 = 0xffffffffu;
#pragma unroll 2
    for (unsigned int j = share.b0; j < share.b1; ++j) {  // (wave-uniform: the record arrives by scalar loads)
        const float* __restrict__ r = refs + (size_t)j * DP;
        const float t0 = q[0] - r[0];
        float d = t0 * t0;
#pragma unroll
        for (int k = 1; k < DP; ++k) {
            const float t = q[k] - r[k];
            d = d + t * t;
        }
        // (squares and their sums are never negative: the bits order as the distances do; an invalid record's +inf and a
        // NaN lie above every finite distance and are "no neighbour" to the host)
        const unsigned int db = __float_as_uint(d);
        // (positions ascend: an equal distance never replaces the minimum, it becomes the second)
        const bool lt = db < kd;
        s2 = lt ? kd : min(s2, db);
        ki = lt ? j : ki;
        kd = lt ? db : kd;
    }
    // (a wave without a reference keeps position ~0: its key is ~0, "nothing found")
    sk[wave][lane] = ((unsigned long long)kd << 32) | (ki == 0xffffffffu ? 0xffffffffu : it.ridx0 + ki);
    ss[wave][lane] = s2;
    __syncthreads();
    if (wave != 0) return;
    unsigned long long key = sk[0][lane];
#pragma unroll 4
    for (int w = 1; w < MATCH_WAVES; ++w) {
        const unsigned long long k = sk[w][lane];
        const unsigned long long lose = k < key ? key : k;
        s2 = min(min(s2, ss[w][lane]), (unsigned int)(lose >> 32));
        key = k < key ? k : key;
    }
    if (!live || key == ~0ull) return;
    const unsigned int slot = it.qslot0 + lane;
    const unsigned long long old = atomicMin(best + slot, key);
    const unsigned long long lose = old < key ? key : old;
    s2 = min(s2, (unsigned int)(lose >> 32));
    if (s2 != 0xffffffffu) atomicMin(second + slot, s2);
}

int match_fpfh_batch(pcc_index* ix, size_t n_pairs, const void* const* des1, const size_t* n1, const void* const* des2,
                     const size_t* n2, size_t stride, int mem, float threshold, int32_t* out, float* out_d2, size_t* out_offsets) {
    MatchBatchScratch* mb = scratch<MatchBatchScratch>(ix);
    MatchFpfhPlan plan;
    if (!match_fpfh_plan(n_pairs, des1, n1, n2, &plan)) { set_error("more than 2^31 records or work items in one batch"); return PCC_ERR_UNSUPPORTED; }
    const size_t n_items = plan.items.size(), n_slots = plan.n_slots;
    const bool on_device = mem != PCC_MEM_HOST;
    std::vector<MatchFpfhSource> sources;
    if (on_device) match_fpfh_sources(plan, n_pairs, des2, n2, &sources);

    // device: [work items][sources (device memory only)][packed records]; what goes up is everything the host has of it
    const size_t items_bytes = align_up(n_items * sizeof(MatchItem), 16);
    const size_t src_bytes = align_up(sources.size() * sizeof(MatchFpfhSource), 16);
    const size_t rec_bytes = plan.n_rec * (size_t)MF_DP * sizeof(float);
    const size_t up_bytes = items_bytes + src_bytes + (on_device ? 0 : rec_bytes);
    const size_t best_bytes = align_up(n_slots * sizeof(unsigned long long), 16), res_bytes = best_bytes + n_slots * sizeof(unsigned int);
    PCC_TRY(mb->up.reserve(up_bytes + 16));
    PCC_TRY(mb->dev.reserve(items_bytes + src_bytes + rec_bytes + 16));
    PCC_TRY(mb->down.reserve(res_bytes + 16));
    PCC_TRY(mb->res.reserve(res_bytes + 16));
    if (n_items) {
        memcpy(mb->up.p, plan.items.data(), n_items * sizeof(MatchItem));
        if (on_device) {
            memcpy(mb->up.as<char>() + items_bytes, sources.data(), sources.size() * sizeof(MatchFpfhSource));
        } else {
            float* rec = reinterpret_cast<float*>(mb->up.as<char>() + items_bytes);
            for (const MatchFpfhPlan::Cloud& c : plan.clouds) match_fpfh_pack(c.p, c.n, stride, rec + c.rec0 * MF_DP);
            for (size_t p = 0; p < n_pairs; ++p) match_fpfh_pack(des2[p], n2[p], stride, rec + plan.q_rec0[p] * MF_DP);
        }
    }

    // ---- one upload, one pack launch (device memory), one search launch, one read-back, one wait -------------------------------
    ix->stats[0] = 0;
    ix->stats[1] = n_slots;
    own_counters(ix, 0);
    const unsigned long long* h_best = mb->down.as<unsigned long long>();
    const unsigned int* h_second = reinterpret_cast<const unsigned int*>(mb->down.as<char>() + best_bytes);
    if (n_items) {
        const MatchItem* d_items = mb->dev.as<MatchItem>();
        const MatchFpfhSource* d_sources = reinterpret_cast<const MatchFpfhSource*>(mb->dev.as<char>() + items_bytes);
        float* d_rec = reinterpret_cast<float*>(mb->dev.as<char>() + items_bytes + src_bytes);
        unsigned long long* d_best = mb->res.as<unsigned long long>();
        unsigned int* d_second = reinterpret_cast<unsigned int*>(mb->res.as<char>() + best_bytes);
        PCC_HIP(hipMemcpyAsync(mb->dev.p, mb->up.p, up_bytes, hipMemcpyHostToDevice, ix->stream));
        PCC_HIP(hipMemsetAsync(mb->res.p, 0xff, res_bytes, ix->stream));
        if (on_device) {
            const unsigned int n_rec = (unsigned int)plan.n_rec;
            const dim3 grid((unsigned int)std::min<size_t>((plan.n_rec + 255) / 256, 4096)), wg(256);
            hipLaunchKernelGGL(k_match_fpfh_pack, grid, wg, 0, ix->stream, d_sources, (unsigned int)sources.size(), stride, n_rec, d_rec);
            PCC_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(k_match_fpfh, dim3((unsigned int)n_items), dim3(MATCH_WAVES * 64), 0, ix->stream, d_items, d_rec, d_best, d_second);
        PCC_HIP(hipGetLastError());
        PCC_HIP(hipMemcpyAsync(mb->down.p, mb->res.p, res_bytes, hipMemcpyDeviceToHost, ix->stream));
        PCC_HIP(hipStreamSynchronize(ix->stream));
    }

    // ---- rows: the dummy 0 (src/comparator.cpp:889), then one index per query with d2 < threshold (:901) ------------------------
    // (an invalid query, an invalid reference and an overflowed distance all arrive as key_none; a pair without a work item
    // never had its slots written)
    size_t o = 0;
    for (size_t p = 0; p < n_pairs; ++p) {
        out_offsets[p] = o;
        if (out_d2) out_d2[o] = 0.0f;
        out[o++] = 0;
        if (!n_items || !n1[p] || !n2[p]) continue;
        for (size_t i = 0; i < n2[p]; ++i) {
            const size_t s = plan.q_slot0[p] + i;
            const unsigned long long key = h_best[s];
            if (key_none(key)) continue;
            const uint32_t bits = (uint32_t)(key >> 32);
            if (h_second[s] == bits) ++ix->ties_flagged;  // (reported in pcc_index_stats[5]; the lowest index stands)
            float d;
            memcpy(&d, &bits, 4);
            if (!(d < threshold)) continue;
            if (out_d2) out_d2[o] = d;
            out[o++] = (int32_t)(uint32_t)key;
        }
    }
    out_offsets[n_pairs] = o;
    return PCC_OK;
}

}  // namespace pcc
