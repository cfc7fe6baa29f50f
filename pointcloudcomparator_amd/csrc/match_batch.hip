// match_batch.hip -- descriptor matching for EVERY cluster pair of a comparison at once (gfx950): pcc_match_knn_batch, and
// pcc_match_knn_batch_dims, which is this search for dim == 3 and match_dims.hip's for every other dimension.  The entry point
// of pcc_match_fpfh_batch (the 33-bin search of match_fpfh.hip) is here too, beside the argument checks the three share.
//
// The reference calls matchRIFTFeaturesKnn (src/comparator.cpp:560-588) from its cluster-matching loop (:1296-1365, call at
// :1322): per cluster of cloud 1 the three nearest clusters of cloud 2, each behind two size gates.  No call depends on an
// earlier one.  One call at a time is set_input + match_knn on a re-pointed handle, two launches and a wait each (small.hip);
// 88 gated pairs of a recorded run are 88 such round trips.  Here all pairs of a comparison share ONE upload, ONE search
// launch, ONE read-back and ONE wait (and, with PCC_TIES_FLANN and at least one tied query, one more of each for the walk).
//
// Shape of the search (k_match_batch): small.hip's workgroup -- 64 queries, 16 waves that share the references through
// wave-uniform (scalar) loads, partial minima meeting in LDS -- driven by a host-built table of WORK ITEMS
// (pair's query block of 64, slice of the pair's references).  The table and its slice rule are match_plan.hpp's, the
// workgroup's scaffold match_search.hpp's, both shared with match_dims.hip and cluster_match.hip; the slices of a query block
// merge in device memory:
//   best[q]   = atomicMin of (bits(d2) << 32 | index)           -- the smallest distance, the lowest index among equals
//   second[q] = atomicMin of bits(d2) of every LOSER            -- the second-smallest distance, counted with multiplicity
// A slice tracks its own minimum key and the second-smallest distance it saw; atomicMin returns the previous value, and of
// (previous, own) the larger one lost: whichever slice minimum is not the final one has lost exactly once by the end, so
// second[q] is exactly the distance of the second-nearest reference.  A query is TIED iff second[q] == bits(d2) of best[q]:
// no tie is missed whatever slices the equal minima lie in, and none is reported that does not exist.
//
// Same arithmetic as small.hip / nn1_brute.hip: d = dx * dx; d += dy * dy; d += dz * dz, every operation rounded
// (-ffp-contract=off); non-finite references never take part; non-finite queries find nothing; a distance that overflowed
// is no neighbour (key_none).
#include "entry.hpp"
#include "match_search.hpp"
#include <algorithm>
#include <thread>
#include <vector>

namespace pcc {

__global__ void __launch_bounds__(MATCH_WAVES * 64, 8)  // (8 waves a SIMD: two workgroups a CU need at most 64 VGPRs)
k_match_batch(const MatchItem* __restrict__ items, const float4* __restrict__ rec, unsigned long long* __restrict__ best,
              unsigned int* __restrict__ second) {
    __shared__ unsigned long long sk[MATCH_WAVES][64];
    __shared__ unsigned int ss[MATCH_WAVES][64];
    const MatchItem it = items[blockIdx.x];  // (block-uniform: scalar loads)
    const MatchLane me = match_lane(it);
    const unsigned int lane = me.lane, wave = me.wave;
    const bool live = me.live;
    const float4 qv = live ? rec[it.q0 + lane] : make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
    const float qx = qv.x, qy = qv.y, qz = qv.z;
    const MatchShare share = match_share(it.nr, wave);
    const unsigned int b0 = share.b0, b1 = share.b1;
    const float4* __restrict__ refs = rec + it.r0;
    // this wave's minimum as (distance bits, position) and the second-smallest distance bits it met (with multiplicity)
    unsigned int kd = 0xffffffffu, ki = 0xffffffffu, s2 = 0xffffffffu;
#pragma unroll 4
    for (unsigned int j = b0; j < b1; ++j) {  // (wave-uniform: the reference arrives by a scalar load)
        const float4 r = refs[j];
        const float dx = qx - r.x, dy = qy - r.y, dz = qz - r.z;
        float d = dx * dx;
        d = d + dy * dy;
        d = d + dz * dz;
        // (a non-finite reference is packed as (0, 0, 0, -1): its distance is computed and discarded -- no branch on the
        // record, so that the scalar loads of an unrolled step go out together instead of one behind the other's test)
        const unsigned int db = __float_as_uint(d) | (unsigned int)(__float_as_int(r.w) >> 31);  // (~0 for w < 0)
        // (positions ascend: an equal distance never replaces the minimum, it becomes the second)
        const bool lt = db < kd;
        s2 = lt ? kd : min(s2, db);
        ki = lt ? j : ki;
        kd = lt ? db : kd;
    }
    // (a wave that met no valid reference keeps position ~0: its key is ~0, "nothing found")
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
    // non-finite query: nothing found (k_pack's preset); a slice without a valid reference has nothing to say
    if (!live || __float_as_int(qv.w) < 0 || key == ~0ull) return;
    const unsigned int slot = it.qslot0 + lane;
    const unsigned long long old = atomicMin(best + slot, key);
    const unsigned long long lose = old < key ? key : old;
    s2 = min(s2, (unsigned int)(lose >> 32));
    if (s2 != 0xffffffffu) atomicMin(second + slot, s2);
}

// ---- the tied queries through FLANN's trees --------------------------------------------------------------------------------
// every tied pair's tree lies in one buffer; a walk item names its query record, its result slot and its tree
struct MatchTree {
    unsigned int node0, leaf0, n_valid, pad;  // first FlannNode, first leaf float of the tree in the shared arrays
    FlannBox root;
    unsigned int pad1, pad2;
};
struct WalkItem {
    unsigned int qrec, slot, tree, pad;
};

// k_small_tie_walk's walk, statement for statement; found[i] = the reference FLANN's walk names, or -1 when it does not
// vouch for another one than the lowest index (the host then keeps what the search found)
template <int STACK>
__global__ void __launch_bounds__(64)
k_match_batch_walk(const MatchTree* __restrict__ trees, const FlannNode* __restrict__ nodes, const float* __restrict__ leaf_pts,
                   const WalkItem* __restrict__ walk, unsigned int n_walk, const float4* __restrict__ rec,
                   const unsigned long long* __restrict__ best, int32_t* __restrict__ found) {
    const unsigned int i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n_walk) return;
    const WalkItem wi = walk[i];
    const MatchTree t = trees[wi.tree];
    const float4 qv = rec[wi.qrec];
    const unsigned long long key = best[wi.slot];
    const float bd = __uint_as_float((unsigned int)(key >> 32));
    bool unc = true;
    int32_t fi = flann_walk_tied<24>(nodes + t.node0, leaf_pts + t.leaf0, t.root, t.n_valid, qv.x, qv.y, qv.z, bd, &unc);
    float d2 = bd;
    if (unc) fi = flann_walk<STACK>(nodes + t.node0, leaf_pts + t.leaf0, t.root, t.n_valid, qv.x, qv.y, qv.z, &d2);
    found[i] = (fi >= 0 && __float_as_uint(d2) == (unsigned int)(key >> 32)) ? fi : -1;
}

// ---- host side -------------------------------------------------------------------------------------------------------------

// k_pack's record: the first three floats, w = position; non-finite -> (0, 0, 0, -1).  Returns the number of finite records.
static size_t pack_records(const void* raw, size_t n, size_t stride, float* out) {
    const char* p = static_cast<const char*>(raw);
    size_t fin_n = 0;
    for (size_t i = 0; i < n; ++i, out += 4) {
        float v[3];
        memcpy(v, p + i * stride, 12);
        const bool fin = finite3(v[0], v[1], v[2]);
        const int32_t w = fin ? (int32_t)i : -1;
        out[0] = fin ? v[0] : 0.f;
        out[1] = fin ? v[1] : 0.f;
        out[2] = fin ? v[2] : 0.f;
        memcpy(out + 3, &w, 4);
        fin_n += fin ? 1 : 0;
    }
    return fin_n;
}

int match_knn_batch(pcc_index* ix, size_t n_pairs, const void* const* des1, const size_t* n1, const void* const* des2,
                    const size_t* n2, size_t stride, float threshold, int32_t* out, float* out_d2, size_t* out_offsets) {
    const bool flann = ix->tie_mode == PCC_TIES_FLANN;
    MatchBatchScratch* mb = scratch<MatchBatchScratch>(ix);

    // ---- the plan: every DISTINCT reference cloud once, every pair's queries, the table of work items (match_plan.hpp) --------
    MatchPlan plan;
    if (!match_plan(n_pairs, des1, n1, n2, match_slice_max_3d(), &plan)) {
        set_error("more than 2^31 records or work items in one batch");
        return PCC_ERR_UNSUPPORTED;
    }
    const std::vector<MatchPlan::Cloud>& clouds = plan.clouds;
    const std::vector<size_t>&cloud_of = plan.cloud_of, &q_rec0 = plan.q_rec0, &q_slot0 = plan.q_slot0;
    const size_t n_rec = plan.n_rec, n_slots = plan.n_slots, n_items = plan.items.size();

    const size_t items_bytes = align_up(n_items * sizeof(MatchItem), 16);
    const size_t up_bytes = items_bytes + n_rec * sizeof(float4);
    const size_t best_bytes = align_up(n_slots * sizeof(unsigned long long), 16), res_bytes = best_bytes + n_slots * sizeof(unsigned int);
    PCC_TRY(mb->up.reserve(up_bytes + 16));
    PCC_TRY(mb->dev.reserve(up_bytes + 16));
    PCC_TRY(mb->down.reserve(res_bytes + 16));
    PCC_TRY(mb->res.reserve(res_bytes + 16));
    if (n_items) memcpy(mb->up.p, plan.items.data(), n_items * sizeof(MatchItem));
    float* rec = reinterpret_cast<float*>(mb->up.as<char>() + items_bytes);
    std::vector<size_t> finite(clouds.size());  // per cloud: its finite records
    for (size_t c = 0; c < clouds.size(); ++c) finite[c] = pack_records(clouds[c].p, clouds[c].n, stride, rec + clouds[c].rec0 * 4);
    for (size_t p = 0; p < n_pairs; ++p) pack_records(des2[p], n2[p], stride, rec + q_rec0[p] * 4);

    // ---- one upload, one launch, one read-back, one wait --------------------------------------------------------------------
    ix->stats[0] = 0;
    ix->stats[1] = n_slots;
    own_counters(ix, 0);
    const unsigned long long* h_best = mb->down.as<unsigned long long>();
    const unsigned int* h_second = reinterpret_cast<const unsigned int*>(mb->down.as<char>() + best_bytes);
    const float4* d_rec = reinterpret_cast<const float4*>(mb->dev.as<char>() + items_bytes);
    unsigned long long* d_best = mb->res.as<unsigned long long>();
    unsigned int* d_second = reinterpret_cast<unsigned int*>(mb->res.as<char>() + best_bytes);
    if (n_items) {
        PCC_HIP(hipMemcpyAsync(mb->dev.p, mb->up.p, up_bytes, hipMemcpyHostToDevice, ix->stream));
        PCC_HIP(hipMemsetAsync(mb->res.p, 0xff, res_bytes, ix->stream));
        hipLaunchKernelGGL(k_match_batch, dim3((unsigned int)n_items), dim3(MATCH_WAVES * 64), 0, ix->stream, mb->dev.as<MatchItem>(), d_rec,
                           d_best, d_second);
        PCC_HIP(hipGetLastError());
        PCC_HIP(hipMemcpyAsync(mb->down.p, mb->res.p, res_bytes, hipMemcpyDeviceToHost, ix->stream));
        PCC_HIP(hipStreamSynchronize(ix->stream));
    }
    // (pairs without a work item -- no query, or no reference at all -- never had their slots written: nothing found)
    auto searched = [&](size_t p) { return n_items && n1[p] && n2[p]; };

    // ---- PCC_TIES_FLANN: the tied queries, per pair -----------------------------------------------------------------------
    std::vector<int32_t> flann_idx;  // per result slot: the index FLANN's walk names, where it differs; -1 elsewhere
    if (flann) {
        std::vector<WalkItem> walk;
        std::vector<int> tree_of(clouds.size(), -1);
        std::vector<size_t> tree_cloud;
        for (size_t p = 0; p < n_pairs; ++p) {
            if (!searched(p)) continue;
            const float* q = rec + q_rec0[p] * 4;
            for (size_t i = 0; i < n2[p]; ++i) {
                const size_t s = q_slot0[p] + i;
                int32_t w;
                memcpy(&w, q + i * 4 + 3, 4);
                if (w < 0 || key_none(h_best[s]) || h_second[s] != (unsigned int)(h_best[s] >> 32)) continue;
                int& t = tree_of[cloud_of[p]];
                if (t < 0) { t = (int)tree_cloud.size(); tree_cloud.push_back(cloud_of[p]); }
                walk.push_back({(unsigned int)(q_rec0[p] + i), (unsigned int)s, (unsigned int)t, 0});
            }
        }
        ix->ties_flagged = walk.size();
        if (!walk.empty()) {
            // FLANN's tree over every cloud with a tied query, once per distinct cloud, from the packed records
            std::vector<FlannTree> trees(tree_cloud.size());
            unsigned int hw = std::thread::hardware_concurrency();
            hw = hw < 1 ? 1 : (hw > 32 ? 32 : hw);
            size_t n_nodes = 0, n_leaf = 0;
            int deepest = 0;  // among the trees the device walks
            std::vector<MatchTree> mt(trees.size());
            for (size_t t = 0; t < trees.size(); ++t) {
                const MatchPlan::Cloud& c = clouds[tree_cloud[t]];
                trees[t].build(rec + c.rec0 * 4, c.n, ix->opt.flann_split, c.n >= 50000 ? hw : (c.n >= 6000 ? std::min(hw, 4u) : 1u));
                mt[t].node0 = (unsigned int)n_nodes;
                mt[t].leaf0 = (unsigned int)n_leaf;
                mt[t].n_valid = (unsigned int)trees[t].n_valid;
                mt[t].root = trees[t].root;
                mt[t].pad = mt[t].pad1 = mt[t].pad2 = 0;
                if (trees[t].depth <= 128) {  // (a deeper tree stays on the host: its queries are walked there)
                    n_nodes += trees[t].nodes.size();
                    n_leaf += trees[t].leaf_pts.size();
                    deepest = std::max(deepest, trees[t].depth);
                }
            }
            // the walk items of device trees first; those of deeper trees are the host's
            std::stable_partition(walk.begin(), walk.end(), [&](const WalkItem& w) { return trees[w.tree].depth <= 128; });
            size_t n_dev = 0;
            while (n_dev < walk.size() && trees[walk[n_dev].tree].depth <= 128) ++n_dev;
            flann_idx.assign(n_slots, -1);
            const int32_t* found = nullptr;
            if (n_dev) {
                const size_t tb = align_up(mt.size() * sizeof(MatchTree), 16), nb = align_up(n_nodes * sizeof(FlannNode), 16);
                const size_t lb = align_up(n_leaf * sizeof(float), 16), wb = n_dev * sizeof(WalkItem);
                PCC_TRY(mb->tree_up.reserve(tb + nb + lb + wb + 16));
                PCC_TRY(mb->tree_dev.reserve(tb + nb + lb + wb + 16));
                PCC_TRY(mb->tree_down.reserve(n_dev * sizeof(int32_t) + 16));
                PCC_TRY(mb->tree_res.reserve(n_dev * sizeof(int32_t) + 16));
                char* u = mb->tree_up.as<char>();
                memcpy(u, mt.data(), mt.size() * sizeof(MatchTree));
                for (size_t t = 0; t < trees.size(); ++t) {
                    if (trees[t].depth > 128) continue;
                    if (!trees[t].nodes.empty()) memcpy(u + tb + mt[t].node0 * sizeof(FlannNode), trees[t].nodes.data(), trees[t].nodes.size() * sizeof(FlannNode));
                    if (!trees[t].leaf_pts.empty()) memcpy(u + tb + nb + mt[t].leaf0 * sizeof(float), trees[t].leaf_pts.data(), trees[t].leaf_pts.size() * sizeof(float));
                }
                memcpy(u + tb + nb + lb, walk.data(), wb);
                PCC_HIP(hipMemcpyAsync(mb->tree_dev.p, u, tb + nb + lb + wb, hipMemcpyHostToDevice, ix->stream));
                const char* d = mb->tree_dev.as<char>();
                const dim3 wg((unsigned int)((n_dev + 63) / 64));
                const auto* d_trees = reinterpret_cast<const MatchTree*>(d);
                const auto* d_nodes = reinterpret_cast<const FlannNode*>(d + tb);
                const auto* d_leaf = reinterpret_cast<const float*>(d + tb + nb);
                const auto* d_walk = reinterpret_cast<const WalkItem*>(d + tb + nb + lb);
                // the walk defers one far child per level: a stack of the deepest tree's depth always suffices
                if (deepest <= 48)
                    hipLaunchKernelGGL(k_match_batch_walk<48>, wg, dim3(64), 0, ix->stream, d_trees, d_nodes, d_leaf, d_walk, (unsigned int)n_dev,
                                       d_rec, d_best, mb->tree_res.as<int32_t>());
                else
                    hipLaunchKernelGGL(k_match_batch_walk<128>, wg, dim3(64), 0, ix->stream, d_trees, d_nodes, d_leaf, d_walk, (unsigned int)n_dev,
                                       d_rec, d_best, mb->tree_res.as<int32_t>());
                PCC_HIP(hipGetLastError());
                PCC_HIP(hipMemcpyAsync(mb->tree_down.p, mb->tree_res.p, n_dev * sizeof(int32_t), hipMemcpyDeviceToHost, ix->stream));
            }
            // (the host's share runs while the device walks)
            std::vector<int32_t> host_found(walk.size() - n_dev, -1);
            for (size_t i = n_dev; i < walk.size(); ++i) {
                const float* qv = rec + (size_t)walk[i].qrec * 4;
                float d2 = 0.f;
                const int32_t fi = trees[walk[i].tree].nearest(qv, &d2);
                uint32_t bits;
                memcpy(&bits, &d2, 4);
                if (fi >= 0 && bits == (uint32_t)(h_best[walk[i].slot] >> 32)) host_found[i - n_dev] = fi;
            }
            if (n_dev) {
                PCC_HIP(hipStreamSynchronize(ix->stream));
                found = mb->tree_down.as<int32_t>();
            }
            for (size_t i = 0; i < walk.size(); ++i) {
                const int32_t fi = i < n_dev ? found[i] : host_found[i - n_dev];
                if (fi >= 0 && (uint32_t)fi != (uint32_t)h_best[walk[i].slot]) {
                    flann_idx[walk[i].slot] = fi;
                    ++ix->ties_changed;
                }
            }
        }
    }

    // ---- rows: the dummy 0 (src/comparator.cpp:568), then one index per query with d2 < threshold (:579) ----------------------
    size_t o = 0;
    for (size_t p = 0; p < n_pairs; ++p) {
        out_offsets[p] = o;
        if (out_d2) out_d2[o] = 0.0f;
        out[o++] = 0;
        if (!searched(p) || finite[cloud_of[p]] == 0) continue;
        const float* q = rec + q_rec0[p] * 4;
        for (size_t i = 0; i < n2[p]; ++i) {
            const size_t s = q_slot0[p] + i;
            int32_t w;
            memcpy(&w, q + i * 4 + 3, 4);
            const unsigned long long key = h_best[s];
            if (w < 0 || key_none(key)) continue;
            float d;
            const uint32_t bits = (uint32_t)(key >> 32);
            memcpy(&d, &bits, 4);
            if (!(d < threshold)) continue;
            if (out_d2) out_d2[o] = d;  // (FLANN's walk names another reference only AT this distance)
            out[o++] = (!flann_idx.empty() && flann_idx[s] >= 0) ? flann_idx[s] : (int32_t)(uint32_t)key;
        }
    }
    out_offsets[n_pairs] = o;
    return PCC_OK;
}

static int check_batch_stride(size_t stride, int dim) {
    if (stride < 4 * (size_t)dim || stride % 4) { set_error("stride %zu must be a multiple of 4 and >= %d", stride, 4 * dim); return PCC_ERR_INVALID; }
    return PCC_OK;
}

// Everything pcc_match_knn_batch refuses before it looks at the handle, for records of which 4 * dim bytes are read: all of
// it host arithmetic.  (check_points' own stride rule is the 3-D one, so the pairs are checked here.)
static int check_batch_args(size_t n_pairs, const void* const* des1, const size_t* n1, const void* const* des2, const size_t* n2,
                            size_t stride, int dim, int mem, const int32_t* out, const size_t* out_offsets, bool device_ok = false) {
    PCC_TRY(check_mem(mem));
    if (mem != PCC_MEM_HOST && !device_ok) { set_error("pcc_match_knn_batch takes host descriptor arrays only (PCC_MEM_HOST)"); return PCC_ERR_UNSUPPORTED; }
    PCC_TRY(check_batch_stride(stride, dim));
    if (!out_offsets) { set_error("null out_offsets"); return PCC_ERR_INVALID; }
    if (n_pairs >= (1ull << 31)) { set_error("more than 2^31 pairs"); return PCC_ERR_UNSUPPORTED; }
    if (n_pairs && (!des1 || !n1 || !des2 || !n2 || !out)) { set_error("null array argument"); return PCC_ERR_INVALID; }
    size_t total1 = 0, total2 = n_pairs;
    for (size_t p = 0; p < n_pairs; ++p) {
        for (int side = 0; side < 2; ++side) {
            const void* d = side ? des2[p] : des1[p];
            const size_t n = side ? n2[p] : n1[p];
            if (n && !d) { set_error("null point pointer"); return PCC_ERR_INVALID; }
            if (n >= (1ull << 31)) { set_error("more than 2^31 points"); return PCC_ERR_UNSUPPORTED; }
        }
        total1 += n1[p];
        total2 += n2[p];
        if (total1 >= (1ull << 31) || total2 >= (1ull << 31)) { set_error("more than 2^31 - 1 descriptors in one batch"); return PCC_ERR_UNSUPPORTED; }
    }
    return PCC_OK;
}

}  // namespace pcc

extern "C" {

int pcc_match_knn_batch(pcc_index* ctx, size_t n_pairs, const void* const* des1, const size_t* n1, const void* const* des2,
                        const size_t* n2, size_t stride, int mem, float threshold, int32_t* out, size_t* out_offsets) {
    using namespace pcc;
    // the arguments first, refused before any device is looked at
    PCC_TRY(check_batch_args(n_pairs, des1, n1, des2, n2, stride, 3, mem, out, out_offsets));
    if (!ctx) { set_error("null index"); return PCC_ERR_INVALID; }
    if (n_pairs == 0) { out_offsets[0] = 0; return PCC_OK; }
    PCC_ENTER(ctx);
    return match_knn_batch(ctx, n_pairs, des1, n1, des2, n2, stride, threshold, out, nullptr, out_offsets);
}

int pcc_match_knn_batch_dims(pcc_index* ctx, size_t n_pairs, const void* const* des1, const size_t* n1, const void* const* des2,
                             const size_t* n2, size_t stride, int dim, int mem, float threshold, int32_t* out, float* out_d2,
                             size_t* out_offsets) {
    using namespace pcc;
    if (dim < 1 || dim > 32) { set_error("descriptor matching searches 1 ... 32 dimensions, not %d", dim); return PCC_ERR_UNSUPPORTED; }
    PCC_TRY(check_batch_stride(stride, dim));
    PCC_TRY(check_batch_args(n_pairs, des1, n1, des2, n2, stride, dim, mem, out, out_offsets));
    if (!ctx) { set_error("null index"); return PCC_ERR_INVALID; }
    if (n_pairs == 0) { out_offsets[0] = 0; return PCC_OK; }
    PCC_ENTER(ctx);
    // three dimensions: the search of pcc_match_knn_batch itself, tie order and FLANN walk included
    if (dim == 3) return match_knn_batch(ctx, n_pairs, des1, n1, des2, n2, stride, threshold, out, out_d2, out_offsets);
    return match_knn_batch_dims(ctx, n_pairs, des1, n1, des2, n2, stride, dim, threshold, out, out_d2, out_offsets);
}

int pcc_match_fpfh_batch(pcc_index* ctx, size_t n_pairs, const void* const* des1, const size_t* n1, const void* const* des2,
                         const size_t* n2, size_t stride, int mem, float threshold, int32_t* out, float* out_d2, size_t* out_offsets) {
    using namespace pcc;
    // the memory space, the stride, then everything pcc_match_knn_batch refuses: all before the handle is looked at
    PCC_TRY(check_batch_args(n_pairs, des1, n1, des2, n2, stride, 33, mem, out, out_offsets, /*device_ok=*/true));
    if (mem == PCC_MEM_DEVICE)  // (the pack kernel reads the records as floats)
        for (size_t p = 0; p < n_pairs; ++p)
            if ((n1[p] && reinterpret_cast<uintptr_t>(des1[p]) % 4) || (n2[p] && reinterpret_cast<uintptr_t>(des2[p]) % 4)) {
                set_error("descriptor arrays in device memory must be 4-byte aligned (pair %zu)", p);
                return PCC_ERR_INVALID;
            }
    if (!ctx) { set_error("null index"); return PCC_ERR_INVALID; }
    if (n_pairs == 0) { out_offsets[0] = 0; return PCC_OK; }
    PCC_ENTER(ctx);
    return match_fpfh_batch(ctx, n_pairs, des1, n1, des2, n2, stride, mem, threshold, out, out_d2, out_offsets);
}
}  // extern "C"
