// sift_batch.hip -- the SIFT keypoint detector, and the keypoint snap behind it, for EVERY cluster of a comparison at once
// (gfx950): pcc_sift_keypoints_batch.
//
// The reference sends every cluster above 700 points through processRIFTwithSIFT (src/comparator.cpp:1228-1231, :1264-1265, body
// :686-822): SIFT keypoints (:435-469), each snapped to the first cluster point within 0.05 (:696-713), then RIFT -- once per
// cluster of both scenes, no call depending on an earlier one.  One cluster at a time is pcc_sift_keypoints + pcc_index_create +
// pcc_first_within: four to five host waits and a few dozen launches per octave.  Here the clouds of a call are ONE concatenated
// cloud -- point base[c] + i is point i of cloud c -- and every stage runs once per octave ROUND over all clouds still in the
// batch, with neighbourhoods that never cross a cloud boundary.  Launches and waits depend on the octaves, not on the clouds.
//
// A round (sift_batch_plan.hpp holds the tables the host rebuilds for it):
//   1. segmented voxel grid: a workgroup per cloud takes the bounding box of its finite points, derives PCL's lattice from it
//      in voxel.hip's float arithmetic and gives every point a key (voxel id << 32 | concatenated index; non-finite points get
//      voxel ~0 and sort behind the cloud's voxels); the keys, a CSR with one row per cloud, are sorted by sort_csr_rows; head
//      flags, a scan, and the voxel count of every cloud comes back with the status word (WAIT 1).  The host applies the
//      25-point gate -- a cloud below it has left the batch, PCL's `break` -- and uploads the round's table; the centroids are
//      written as the next concatenation, every cloud in ascending voxel order, sums in double over ascending index (the
//      order of the sorted keys), rounded once: tests/cpp/sift_host.cpp's voxel grid.
//   2. sorted radius rows at 3 x the largest scale from rift_batch.hip's exhaustive builder (WAIT 2: the CSR's total).
//   3. intensity and scale space: sift.hip's kernels, unchanged, over the concatenation.
//   4. segmented 25-NN (k_sb_knn25): a point whose sorted radius row holds 25 entries takes the row's first 25 -- the same set
//      in the same order --; the others scan their own cloud exhaustively from LDS tiles, a wave per query keeping the best 25
//      (d2, index) keys across its lanes.
//   5. extrema, scan (sift.hip), the keypoint count of every cloud (WAIT 3), the keypoints behind those of the rounds before.
// Behind the last round the keypoints lie in (round, cloud, point, scale) order on the device; the snap kernel (a wave per
// keypoint over its own cloud's ORIGINAL points in index order, pcc_first_within's double arithmetic) runs over them there, one
// copy brings both down and the host splices them into (cloud, octave, point, scale) order.
//
// Clouds above PCC_OPT_SIFT_BATCH_BRUTE_MAX points would make the quadratic builders the bottleneck: they take the single path
// inside the same call, one by one, on a work handle kept in ctx, and their slices are spliced in.  The host scaffold (route
// split, lease, shared argument checks) is cloud_batch.hpp's and entry.hpp's: DESIGN.md 4.16; the 32-byte record pack is this file's.
#include <algorithm>
#include <cmath>
#include <vector>

#include "entry.hpp"
#include "grid_device.hpp"
#include "sift_stages.hpp"
#include "sift_batch_plan.hpp"
#include "voxel_plan.hpp"
#include "desc_batch.hpp"

namespace pcc {

namespace {

constexpr unsigned int SB_MAX_CELLS = VOXEL_MAX_CELLS;  // voxel.hip's limit
constexpr unsigned int SB_NO_VOXEL = 0xffffffffu;  // the voxel of a non-finite point: behind every voxel of its cloud

// ---- 1. segmented voxel grid ---------------------------------------------------------------------------------------------
// A workgroup per cloud: bounding box of the finite points -> the lattice (voxel_plan.hpp, as voxel.hip: min_b = floor(lo * inv),
// dim = max_b - min_b + 1, x fastest) -> a key per point.  A lattice above 2^26 voxels, or with a bound beyond int32, leaves the
// cloud's number + 1 in *status (the largest such cloud) and the cloud without voxels.
__global__ void __launch_bounds__(256)
k_sb_voxel_keys(const unsigned int* __restrict__ bases, const SiftRec* __restrict__ in, float inv, unsigned long long* __restrict__ keys,
                unsigned int* __restrict__ cloud_of, unsigned int* __restrict__ status) {
    __shared__ float s_lo[3][4], s_hi[3][4];
    __shared__ float s_org[3];
    __shared__ int s_dim[3];
    const unsigned int c = blockIdx.x;
    const unsigned int base = bases[c], n = bases[c + 1] - base;  // block-uniform
    if (n == 0) return;
    const unsigned int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    for (unsigned int i = threadIdx.x; i < n; i += 256) {
        const SiftRec p = in[base + i];
        if (!finite3(p.x, p.y, p.z)) continue;
        lo[0] = fminf(lo[0], p.x); lo[1] = fminf(lo[1], p.y); lo[2] = fminf(lo[2], p.z);
        hi[0] = fmaxf(hi[0], p.x); hi[1] = fmaxf(hi[1], p.y); hi[2] = fmaxf(hi[2], p.z);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], m));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], m));
        }
        if (lane == 0) { s_lo[a][wave] = lo[a]; s_hi[a][wave] = hi[a]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float l[3], h[3];
        for (int a = 0; a < 3; ++a) {
            l[a] = fminf(fminf(s_lo[a][0], s_lo[a][1]), fminf(s_lo[a][2], s_lo[a][3]));
            h[a] = fmaxf(fmaxf(s_hi[a][0], s_hi[a][1]), fmaxf(s_hi[a][2], s_hi[a][3]));
        }
        bool any = l[0] <= h[0];  // (false: no finite point, on every axis alike)
        if (any) {
            const VoxelPlan vp = voxel_plan(l, h, inv);
            if (vp.verdict != VOXEL_PLAN_OK) {  // (the host check of the entry point has refused the first octave's before)
                atomicMax(status, c + 1u);
                any = false;
            }
            for (int a = 0; a < 3; ++a) { s_org[a] = vp.org[a]; s_dim[a] = vp.dim[a]; }
        }
        if (!any) s_dim[0] = s_dim[1] = s_dim[2] = 0;
    }
    __syncthreads();
    const float o0 = s_org[0], o1 = s_org[1], o2 = s_org[2];
    const int d0 = s_dim[0], d1 = s_dim[1], d2 = s_dim[2];
    for (unsigned int i = threadIdx.x; i < n; i += 256) {
        const SiftRec p = in[base + i];
        unsigned int v = SB_NO_VOXEL;
        if (d0 > 0 && finite3(p.x, p.y, p.z)) {
            // (grid_device.hpp's voxel_id, the lattice in registers)
            const int i0 = min(max((int)(floorf(p.x * inv) - o0), 0), d0 - 1);
            const int i1 = min(max((int)(floorf(p.y * inv) - o1), 0), d1 - 1);
            const int i2 = min(max((int)(floorf(p.z * inv) - o2), 0), d2 - 1);
            v = ((unsigned int)i2 * (unsigned int)d1 + (unsigned int)i1) * (unsigned int)d0 + (unsigned int)i0;
        }
        keys[base + i] = ((unsigned long long)v << 32) | (base + i);
        cloud_of[base + i] = c;
    }
}

// flags[t] = 1 where sorted position t starts a voxel of its cloud; flags[n] = 0 (the scan leaves the voxel count there)
__global__ void __launch_bounds__(256)
k_sb_heads(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ cloud_of, unsigned int n, unsigned int* __restrict__ flags) {
    for (unsigned int t = blockIdx.x * blockDim.x + threadIdx.x; t <= n; t += gridDim.x * blockDim.x) {
        unsigned int f = 0;
        if (t < n) {
            const unsigned int v = (unsigned int)(keys[t] >> 32);
            if (v != SB_NO_VOXEL) f = (t == 0 || cloud_of[t - 1] != cloud_of[t] || (unsigned int)(keys[t - 1] >> 32) != v) ? 1u : 0u;
        }
        flags[t] = f;
    }
}

// out[c] = pos[bases[c + 1]] - pos[bases[c]] for c < n_clouds (the voxels of cloud c), out[n_clouds] = *status
__global__ void __launch_bounds__(256)
k_sb_sizes(const unsigned int* __restrict__ pos, const unsigned int* __restrict__ bases, unsigned int n_clouds, const unsigned int* __restrict__ status,
           unsigned int* __restrict__ out) {
    for (unsigned int c = blockIdx.x * blockDim.x + threadIdx.x; c <= n_clouds; c += gridDim.x * blockDim.x)
        out[c] = c < n_clouds ? pos[bases[c + 1]] - pos[bases[c]] : *status;
}

// out[c] = pos[bases[c]] for c <= n_clouds: the keypoints in front of cloud c, out[n_clouds] = all of the round
__global__ void __launch_bounds__(256)
k_sb_gather(const unsigned int* __restrict__ pos, const unsigned int* __restrict__ bases, unsigned int n_clouds, unsigned int* __restrict__ out) {
    for (unsigned int c = blockIdx.x * blockDim.x + threadIdx.x; c <= n_clouds; c += gridDim.x * blockDim.x) out[c] = pos[bases[c]];
}

// One lane per voxel head: the centroid of the voxel's points (voxel.hip's k_vox_centroids over the sorted keys: ascending
// index within a voxel) into the next concatenation -- cloud c's voxels at bases_out[c] in voxel order.  A cloud that left the
// batch in this round (bases_out gives it no room) writes nothing.
__global__ void __launch_bounds__(256)
k_sb_centroids(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ cloud_of, const unsigned int* __restrict__ pos,
               const unsigned int* __restrict__ bases_in, const unsigned int* __restrict__ bases_out, const SiftRec* __restrict__ in, unsigned int n,
               SiftRec* __restrict__ out, float4* __restrict__ out4) {
    for (unsigned int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
        if (pos[t + 1] == pos[t]) continue;  // exclusive scan of 0/1 flags: a head bumps the next entry
        const unsigned int c = cloud_of[t];
        const unsigned int ob = bases_out[c], on = bases_out[c + 1] - ob;
        if (on == 0) continue;
        const unsigned int v = (unsigned int)(keys[t] >> 32), end = bases_in[c + 1];
        double sx = 0, sy = 0, sz = 0;
        unsigned int sr = 0, sg = 0, sb = 0, cnt = 0;
        for (unsigned int u = t; u < end; ++u) {
            const unsigned long long k = keys[u];
            if ((unsigned int)(k >> 32) != v) break;
            const SiftRec p = in[(unsigned int)k];
            sx += p.x; sy += p.y; sz += p.z;
            sr += (p.rgb >> 16) & 0xffu; sg += (p.rgb >> 8) & 0xffu; sb += p.rgb & 0xffu;
            ++cnt;
        }
        const unsigned int slot = pos[t] - pos[bases_in[c]];
        if (slot >= on) continue;  // (cannot happen: on is this very difference of the scan)
        const unsigned int o = ob + slot;
        SiftRec r;
        r.x = (float)(sx / cnt); r.y = (float)(sy / cnt); r.z = (float)(sz / cnt); r.w = 1.0f;
        // PCL: centroid /= float(count); rgb = int(r) << 16 | int(g) << 8 | int(b)
        const float fc = (float)cnt;
        const int cr = (int)((float)sr / fc), cg = (int)((float)sg / fc), cb = (int)((float)sb / fc);
        r.rgb = ((unsigned int)cr << 16) | ((unsigned int)cg << 8) | (unsigned int)cb;
        r.pad[0] = r.pad[1] = r.pad[2] = 0u;
        out[o] = r;
        out4[o] = make_float4(r.x, r.y, r.z, __uint_as_float(o));
    }
}

// ---- 4. segmented 25-NN --------------------------------------------------------------------------------------------------
// The work items of the row builder (a query block of one cloud each).  nbr[q][25]: the 25 smallest (d2, index) of query q
// over its own cloud, itself included, ascending, as concatenated indices; every cloud of a round holds at least 25 points.
// A query whose sorted radius row holds 25 entries copies them.  The others: the cloud staged in LDS tiles in ascending order,
// a wave per query with its lanes over the candidates of the tile; lane l < 25 holds the l-th best key so far (kept in LDS
// between tiles); a ballot lists the candidates below the 25th, and each is inserted by shifting the lanes behind its place.
constexpr unsigned int SB_K = (unsigned int)SIFT_NEIGHBOURS;

__global__ void __launch_bounds__(256)
k_sb_knn25(const RiftBatchItem* __restrict__ items, const float4* __restrict__ pts, const unsigned long long* __restrict__ row_keys,
           const unsigned int* __restrict__ row_off, int32_t* __restrict__ nbr) {
    __shared__ float4 tile[RB_TILE];
    __shared__ unsigned long long best[RB_QUERIES][32];
    __shared__ unsigned int scan_it[RB_QUERIES];  // 1: the query scans its cloud
    const unsigned int lane = threadIdx.x & 63;
    const unsigned int wave = (unsigned int)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const RiftBatchItem it = items[blockIdx.x];  // (block-uniform)
    const float4* __restrict__ cloud = pts + it.base;
    int need = 0;
    for (unsigned int qi = wave; qi < it.nq; qi += 4) {  // wave-uniform
        const unsigned int q = it.base + it.q0 + qi;
        const unsigned int beg = row_off[q], len = row_off[q + 1] - beg;
        if (len >= SB_K) {
            if (lane < SB_K) nbr[(size_t)q * SB_K + lane] = (int32_t)(unsigned int)row_keys[(size_t)beg + lane];
            if (lane == 0) scan_it[qi] = 0u;
        } else {
            if (lane < 32) best[qi][lane] = ~0ull;
            if (lane == 0) scan_it[qi] = 1u;
            need = 1;
        }
    }
    if (!__syncthreads_or(need)) return;  // (also publishes best[] and scan_it[])
    for (unsigned int t0 = 0; t0 < it.n; t0 += RB_TILE) {  // block-uniform
        const unsigned int tn = min(RB_TILE, it.n - t0);
        __syncthreads();  // (the tile before has been used up)
        for (unsigned int i = threadIdx.x; i < tn; i += 256) tile[i] = cloud[t0 + i];
        __syncthreads();
        const bool last = t0 + RB_TILE >= it.n;
        for (unsigned int qi = wave; qi < it.nq; qi += 4) {  // wave-uniform
            if (!scan_it[qi]) continue;
            const unsigned int q = it.base + it.q0 + qi;
            const float4 qv = pts[q];
            unsigned long long mine = lane < 32 ? best[qi][lane] : ~0ull;
            unsigned long long worst = __shfl(mine, (int)SB_K - 1);
            for (unsigned int c0 = 0; c0 < tn; c0 += 64) {
                const unsigned int c = c0 + lane;
                const float4 r = tile[min(c, tn - 1u)];
                const float d = dist2_nc(qv.x, qv.y, qv.z, r);
                const unsigned long long key = c < tn ? make_key(d, r) : ~0ull;
                unsigned long long m = __ballot(key < worst);
                while (m) {  // wave-uniform
                    const int b = __builtin_ctzll(m);
                    m &= m - 1;
                    const unsigned long long ck = __shfl(key, b);
                    if (!(ck < worst)) continue;  // (the 25th has come down since the ballot)
                    const unsigned int at = (unsigned int)__popcll(__ballot(mine < ck));  // < 25: ck is below lane 24's key
                    const unsigned long long up = __shfl_up(mine, 1);
                    mine = lane < at ? mine : (lane == at ? ck : up);
                    if (lane >= SB_K) mine = ~0ull;
                    worst = __shfl(mine, (int)SB_K - 1);
                }
            }
            if (last) {
                if (lane < SB_K) nbr[(size_t)q * SB_K + lane] = (int32_t)(unsigned int)mine;
            } else if (lane < 32) {
                best[qi][lane] = mine;
            }
        }
    }
}

// ---- the snap ------------------------------------------------------------------------------------------------------------
// A wave per keypoint over its own cloud's original points in index order: the lowest index whose distance (differences in
// float, squares, sum and sqrt in double: k_grid_first_within's test) is < radius, or -1.
__global__ void __launch_bounds__(256)
k_sb_snap(const float4* __restrict__ kp, const unsigned int* __restrict__ kp_cloud, const unsigned int* __restrict__ bases0,
          const SiftRec* __restrict__ rec0, double radius, unsigned int m, int32_t* __restrict__ snap) {
    const unsigned int lane = threadIdx.x & 63;
    const unsigned int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (unsigned int k = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; k < m; k += nwaves) {  // wave-uniform
        const float4 q = kp[k];
        const unsigned int c = kp_cloud[k];
        const unsigned int base = bases0[c], n = bases0[c + 1] - base;
        int32_t first = -1;
        for (unsigned int c0 = 0; c0 < n; c0 += 64) {
            const unsigned int i = c0 + lane;
            bool hit = false;
            if (i < n) {
                const SiftRec p = rec0[base + i];
                const double dx = (double)(q.x - p.x), dy = (double)(q.y - p.y), dz = (double)(q.z - p.z);
                hit = sqrt(dx * dx + dy * dy + dz * dz) < radius;
            }
            const unsigned long long mask = __ballot(hit);
            if (mask) { first = (int32_t)(c0 + (unsigned int)__builtin_ctzll(mask)); break; }
        }
        if (lane == 0) snap[k] = first;
    }
}

}  // namespace

// (up: octaves + table + records, then every round's table; down: sizes, counts, keypoints; dev: the first upload, whose records the snap reads)
struct SiftBatchScratch : BatchStaging {
    static constexpr ScratchSlot slot = SCRATCH_SIFT_BATCH;
    DevBuf table[2];             // the tables of the later rounds, in turn
    DevBuf cloud[2], pts4;       // octave concatenations as records (the voxel stage reads one, writes the other); the current one as float4
    DevBuf vkeys, cloud_of;      // voxel keys u64[n]; the cloud of every position uint32[n]
    DevBuf flags, scan_tmp;      // head flags / voxel positions uint32[n + 1]
    DevBuf words;                // uint32: [0] the status word, then n_clouds + 1 sizes or counts of the round
    DevBuf offs, keys;           // the CSR of the round's radius rows
    DevBuf nbr;                  // int32[n][25]
    DevBuf kp_cloud, snap;       // per keypoint: its cloud; the snapped index
};

// ---- the half over a device-resident first concatenation (desc_batch.hpp): shared with cluster_desc.hip ---------------------
int sift_batch_rounds(pcc_index* ix, size_t n_clouds, const SiftBatchInput& in, float min_scale, SiftBatchResult* res) {
    hipStream_t s = ix->stream;
    SiftBatchScratch* b = scratch<SiftBatchScratch>(ix);
    SiftScratch* r = scratch<SiftScratch>(ix);
    SiftBatchRound next;
    const std::vector<SiftOctave>& h_octaves = *in.h_octaves;
    const SiftOctave* d_octaves = in.d_octaves;
    const int nr_octaves = (int)h_octaves.size();
    res->bases0 = in.round0->bases;
    res->d_bases0 = in.d_bases0;
    res->d_rec0 = in.d_rec0;
    size_t cur_total = in.round0->total;
    if (cur_total == 0) return PCC_OK;

    const unsigned int* d_bases_in = in.d_bases0;
    const int64_t* d_bases64_in = in.d_bases64_0;
    const SiftRec* d_in = in.d_rec0;
    PCC_TRY(b->words.reserve((n_clouds + 2) * sizeof(unsigned int)));
    PCC_TRY(b->down.reserve((n_clouds + 2) * sizeof(unsigned int)));
    unsigned int* d_status = b->words.as<unsigned int>();
    unsigned int* d_words = d_status + 1;
    const unsigned int* h_words = b->down.as<unsigned int>();
    const unsigned int cb = blocks_for(n_clouds + 1);
    int flip = 0;
    float scale = min_scale;
    for (int o = 0; o < nr_octaves; ++o, scale *= 2.0f) {
        const size_t n_in = cur_total;
        ++res->rounds;
        // ---- 1. the voxel grid of every cloud at leaf = the octave's scale ----------------------------------------------------
        PCC_TRY(b->vkeys.reserve(n_in * sizeof(unsigned long long)));
        PCC_TRY(b->cloud_of.reserve(n_in * sizeof(unsigned int)));
        PCC_TRY(b->flags.reserve((n_in + 1) * sizeof(unsigned int)));
        PCC_HIP(hipMemsetAsync(d_status, 0, sizeof(unsigned int), s));
        hipLaunchKernelGGL(k_sb_voxel_keys, dim3((unsigned int)n_clouds), dim3(256), 0, s, d_bases_in, d_in, 1.0f / scale,
                           b->vkeys.as<unsigned long long>(), b->cloud_of.as<unsigned int>(), d_status);
        PCC_HIP(hipGetLastError());
        PCC_TRY(sort_csr_rows(s, d_bases64_in, n_clouds, b->vkeys.as<unsigned long long>()));
        hipLaunchKernelGGL(k_sb_heads, dim3(blocks_for(n_in + 1)), dim3(256), 0, s, b->vkeys.as<unsigned long long>(), b->cloud_of.as<unsigned int>(),
                           (unsigned int)n_in, b->flags.as<unsigned int>());
        PCC_HIP(hipGetLastError());
        PCC_TRY(launch_exclusive_scan(ix, s, b->flags.as<unsigned int>(), n_in + 1, b->scan_tmp));
        hipLaunchKernelGGL(k_sb_sizes, dim3(cb), dim3(256), 0, s, b->flags.as<unsigned int>(), d_bases_in, (unsigned int)n_clouds, d_status, d_words);
        PCC_HIP(hipGetLastError());
        PCC_HIP(hipMemcpyAsync(b->down.p, d_words, (n_clouds + 1) * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
        PCC_HIP(hipStreamSynchronize(s));  // WAIT 1: the voxels of every cloud, the status word
        if (h_words[n_clouds]) {
            set_error("cloud %u: leaf size %g too small for this cloud: more than %u voxels", h_words[n_clouds] - 1u, scale, SB_MAX_CELLS);
            return PCC_ERR_UNSUPPORTED;
        }
        // 2. PCL's min_nr_points: a cloud below it has left the batch
        sift_batch_round(h_words, n_clouds, (size_t)SIFT_MIN_POINTS, &next);
        const size_t n_oct = next.total;
        if (n_oct == 0) break;
        const TableLayout tl(n_clouds, next.items.size());
        PCC_TRY(b->up.reserve(tl.bytes));  // (nothing is in flight from it: the wait above)
        PCC_TRY(b->table[flip].reserve(tl.bytes));
        tl.fill(b->up.as<char>(), next);
        PCC_HIP(hipMemcpyAsync(b->table[flip].p, b->up.p, tl.bytes, hipMemcpyHostToDevice, s));
        const char* dt = b->table[flip].as<char>();
        const unsigned int* d_bases_out = reinterpret_cast<const unsigned int*>(dt + tl.bases_at);
        const RiftBatchItem* d_items = reinterpret_cast<const RiftBatchItem*>(dt + tl.items_at);
        PCC_TRY(b->cloud[flip].reserve(n_oct * sizeof(SiftRec)));
        PCC_TRY(b->pts4.reserve(n_oct * sizeof(float4)));
        SiftRec* d_cloud = b->cloud[flip].as<SiftRec>();
        hipLaunchKernelGGL(k_sb_centroids, dim3(blocks_for(n_in)), dim3(256), 0, s, b->vkeys.as<unsigned long long>(), b->cloud_of.as<unsigned int>(),
                           b->flags.as<unsigned int>(), d_bases_in, d_bases_out, d_in, (unsigned int)n_in, d_cloud, b->pts4.as<float4>());
        PCC_HIP(hipGetLastError());
        // ---- 3. to 6. over the concatenation ----------------------------------------------------------------------------------
        const SiftOctave& h_oc = h_octaves[(size_t)o];
        const int S = h_oc.n_scales;
        const SiftOctave* oc = d_octaves + o;
        PCC_TRY(sift_intensity_stage(ix, d_cloud, n_oct));
        const float radius = 3.0f * h_oc.scales[S - 1];
        const unsigned long long* keys = nullptr;
        const unsigned int* off32 = nullptr;
        PCC_TRY(batch_radius_rows(ix, d_items, (unsigned int)next.items.size(), b->pts4.as<float4>(), n_oct, radius2((double)radius), b->offs, b->keys,
                                  &keys, &off32));  // WAIT 2: the CSR's total
        PCC_TRY(sift_space_stage(ix, n_oct, keys, off32, oc, S));
        PCC_TRY(b->nbr.reserve(n_oct * (size_t)SB_K * sizeof(int32_t)));
        hipLaunchKernelGGL(k_sb_knn25, dim3((unsigned int)next.items.size()), dim3(256), 0, s, d_items, b->pts4.as<float4>(), keys, off32,
                           b->nbr.as<int32_t>());
        PCC_HIP(hipGetLastError());
        PCC_TRY(sift_extrema_stage(ix, n_oct, b->nbr.as<int32_t>(), (int)SB_K, oc));
        hipLaunchKernelGGL(k_sb_gather, dim3(cb), dim3(256), 0, s, r->count.as<unsigned int>(), d_bases_out, (unsigned int)n_clouds, d_words);
        PCC_HIP(hipGetLastError());
        PCC_HIP(hipMemcpyAsync(b->down.p, d_words, (n_clouds + 1) * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
        PCC_HIP(hipStreamSynchronize(s));  // WAIT 3: the keypoints in front of every cloud, and their number
        // ---- 7. behind the keypoints of the rounds before ---------------------------------------------------------------------
        const size_t found = h_words[n_clouds];
        std::vector<uint32_t> per_cloud(n_clouds);
        for (size_t c = 0; c < n_clouds; ++c) per_cloud[c] = h_words[c + 1] - h_words[c];
        res->counts.push_back(per_cloud);
        PCC_TRY(sift_write_stage(ix, d_cloud, n_oct, oc, res->total, found));
        res->total += found;
        // the next round reads what this one wrote
        cur_total = next.total;
        d_bases_in = d_bases_out;
        d_bases64_in = reinterpret_cast<const int64_t*>(dt + tl.bases64_at);
        d_in = d_cloud;
        flip ^= 1;
    }
    return PCC_OK;
}

// d_snap[k] for the keypoints of the rounds (round-major): the cloud of every keypoint goes up, then a wave per keypoint
int sift_batch_snap(pcc_index* ix, const SiftBatchResult& res, size_t n_clouds, double snap_radius, int32_t* d_snap) {
    hipStream_t s = ix->stream;
    SiftBatchScratch* b = scratch<SiftBatchScratch>(ix);
    const size_t m = res.total;
    if (!m) return PCC_OK;
    // the cloud of every keypoint, in the device's (round, cloud) order
    PCC_TRY(b->up.reserve(m * sizeof(uint32_t)));
    PCC_TRY(b->kp_cloud.reserve(m * sizeof(uint32_t)));
    uint32_t* kc = b->up.as<uint32_t>();
    size_t at = 0;
    for (const std::vector<uint32_t>& round : res.counts)
        for (size_t c = 0; c < n_clouds; ++c)
            for (uint32_t i = 0; i < round[c]; ++i) kc[at++] = (uint32_t)c;
    PCC_HIP(hipMemcpyAsync(b->kp_cloud.p, kc, m * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    const unsigned int wb = (unsigned int)std::min<size_t>((m + 3) / 4, 8192);
    hipLaunchKernelGGL(k_sb_snap, dim3(wb), dim3(256), 0, s, scratch<SiftScratch>(ix)->kp.as<float4>(), b->kp_cloud.as<unsigned int>(), res.d_bases0, res.d_rec0,
                       snap_radius, (unsigned int)m, d_snap);
    PCC_HIP(hipGetLastError());
    return PCC_OK;
}

namespace {

// the host clouds of sizes batch.n[] (0: not part of the batch) staged as the first concatenation, then through the rounds
int sift_batch_rounds_host(pcc_index* ix, const CloudBatch& batch, float min_scale, int nr_octaves, int nr_scales_per_octave, float min_contrast,
                           SiftBatchResult* res) {
    hipStream_t s = ix->stream;
    const size_t n_clouds = batch.n_clouds;
    SiftBatchScratch* b = scratch<SiftBatchScratch>(ix);
    SiftBatchRound cur;
    sift_batch_round(batch.n, n_clouds, 0, &cur);
    res->bases0 = cur.bases;
    if (cur.total == 0) return PCC_OK;
    const std::vector<SiftOctave> h_octaves = sift_batch_octaves(min_scale, nr_octaves, nr_scales_per_octave, min_contrast);

    // ---- one pinned buffer, one copy: the octaves' scales, the first table, 32 bytes a point ---------------------------------
    const size_t oct_bytes = align_up(h_octaves.size() * sizeof(SiftOctave), 16);
    const TableLayout t0(n_clouds, 0, oct_bytes);  // (the first round needs no items: the voxel stage works by cloud)
    const size_t rec_at = align_up(t0.bytes, 32), up_bytes = rec_at + cur.total * sizeof(SiftRec);
    PCC_TRY(b->up.reserve(up_bytes));
    PCC_TRY(b->dev.reserve(up_bytes));
    char* u = b->up.as<char>();
    memcpy(u, h_octaves.data(), h_octaves.size() * sizeof(SiftOctave));
    cur.items.clear();
    t0.fill(u, cur);
    SiftRec* rec = reinterpret_cast<SiftRec*>(u + rec_at);
    for (size_t c = 0; c < n_clouds; ++c) {
        if (!cur.n[c]) continue;
        const char* src = static_cast<const char*>(batch.pts[c]);
        const char* col = static_cast<const char*>(batch.rgb[c]);
        for (size_t i = 0; i < cur.n[c]; ++i) {
            SiftRec& p = rec[cur.bases[c] + i];
            memcpy(&p.x, src + i * batch.stride, 12);
            p.w = 1.0f;
            memcpy(&p.rgb, col + i * batch.rgb_stride, 4);
            p.pad[0] = p.pad[1] = p.pad[2] = 0u;
        }
    }
    PCC_HIP(hipMemcpyAsync(b->dev.p, u, up_bytes, hipMemcpyHostToDevice, s));
    const char* d0 = b->dev.as<char>();
    SiftBatchInput in;
    in.round0 = &cur;
    in.h_octaves = &h_octaves;
    in.d_octaves = reinterpret_cast<const SiftOctave*>(d0);
    in.d_bases0 = reinterpret_cast<const unsigned int*>(d0 + t0.bases_at);
    in.d_bases64_0 = reinterpret_cast<const int64_t*>(d0 + t0.bases64_at);
    in.d_rec0 = reinterpret_cast<const SiftRec*>(d0 + rec_at);
    return sift_batch_rounds(ix, n_clouds, in, min_scale, res);
}

// the single path for cloud c, which is above the brute limit, on the work handle: its keypoints into kp (host)
int sift_single(pcc_index* w, const CloudBatch& batch, size_t c, float min_scale, int nr_octaves, int nr_scales_per_octave, float min_contrast,
                std::vector<float>* kp) {
    const size_t n = batch.n[c], stride = batch.stride, rgb_stride = batch.rgb_stride;
    SiftScratch* r = scratch<SiftScratch>(w);
    entered(w);
    const unsigned char *dpts = nullptr, *drgb = nullptr;
    PCC_TRY(stage_in(w, static_cast<const unsigned char*>(batch.pts[c]), (n - 1) * stride + 12, PCC_MEM_HOST, r->pts, &dpts));
    PCC_TRY(stage_in(w, static_cast<const unsigned char*>(batch.rgb[c]), (n - 1) * rgb_stride + 4, PCC_MEM_HOST, r->rgb, &drgb));
    size_t found = 0;
    PCC_TRY(sift_keypoints(w, dpts, n, stride, drgb, rgb_stride, min_scale, nr_octaves, nr_scales_per_octave, min_contrast, &found));
    kp->resize(found * 4);
    if (found) {
        PCC_HIP(hipMemcpyAsync(kp->data(), r->kp.p, found * 4 * sizeof(float), hipMemcpyDeviceToHost, w->stream));
        PCC_HIP(hipStreamSynchronize(w->stream));
    }
    return PCC_OK;
}

}  // namespace

// pcc_sift_keypoints_batch behind its argument checks (every out array on the host; out_snap nullable)
int sift_keypoints_batch(pcc_index* ix, const CloudBatch& batch, float min_scale, int nr_octaves, int nr_scales_per_octave, float min_contrast,
                         double snap_radius, float* out_kp, int32_t* out_snap, size_t capacity, size_t* out_offsets) {
    hipStream_t s = ix->stream;
    const size_t n_clouds = batch.n_clouds;
    PCC_TRY(sync_info(ix));  // (a pending mirror of the handle's own grid would overwrite stats[2] later)
    SiftBatchScratch* b = scratch<SiftBatchScratch>(ix);
    const size_t brute_max = (size_t)ix->opt.sift_batch_brute_max;
    const BatchRoutes routes = batch_routes(batch.n, n_clouds, brute_max);
    CloudBatch small = batch;
    small.n = routes.small_n.data();
    SiftBatchResult res;
    PCC_TRY(sift_batch_rounds_host(ix, small, min_scale, nr_octaves, nr_scales_per_octave, min_contrast, &res));
    ix->stats[0] = routes.n_brute;
    ix->stats[1] = routes.n_large;
    ix->stats[2] = res.rounds;
    ix->stats_pending = false;

    // ---- clouds above the limit: one by one on the work handle ----------------------------------------------------------------
    std::vector<std::vector<float>> large_kp(n_clouds);
    WorkLease lease;
    if (routes.n_large) {
        PCC_TRY(lease.take(ix, b->work, true));
        for (size_t c = 0; c < n_clouds; ++c)
            if (batch.n[c] > brute_max)
                PCC_TRY(sift_single(lease.w, batch, c, min_scale, nr_octaves, nr_scales_per_octave, min_contrast, &large_kp[c]));
    }

    // ---- the slices: (cloud, octave, point, scale) ----------------------------------------------------------------------------
    std::vector<size_t> batch_off;
    std::vector<SiftBatchCopy> copies;
    sift_batch_splice(res.counts, n_clouds, &batch_off, &copies);
    std::vector<size_t> shift(n_clouds + 1, 0);  // keypoints of the large clouds in front of cloud c
    for (size_t c = 0; c < n_clouds; ++c) shift[c + 1] = shift[c] + large_kp[c].size() / 4;
    for (size_t c = 0; c <= n_clouds; ++c) out_offsets[c] = batch_off[c] + shift[c];
    const size_t total = out_offsets[n_clouds];
    if (total > capacity) {
        set_error("%zu keypoints, room for %zu", total, capacity);
        return PCC_ERR_OVERFLOW;
    }
    if (res.total) {
        const size_t m = res.total;
        const size_t snap_at = align_up(m * sizeof(float4), 16);
        PCC_TRY(b->down.reserve(snap_at + m * sizeof(int32_t)));
        if (out_snap) {
            PCC_TRY(b->snap.reserve(m * sizeof(int32_t)));
            PCC_TRY(sift_batch_snap(ix, res, n_clouds, snap_radius, b->snap.as<int32_t>()));
            PCC_HIP(hipMemcpyAsync(b->down.as<char>() + snap_at, b->snap.p, m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        }
        PCC_HIP(hipMemcpyAsync(b->down.p, scratch<SiftScratch>(ix)->kp.p, m * sizeof(float4), hipMemcpyDeviceToHost, s));
        PCC_HIP(hipStreamSynchronize(s));  // the call's last wait: keypoints and snapped indices
        const float* h_kp = b->down.as<float>();
        const int32_t* h_snap = reinterpret_cast<const int32_t*>(b->down.as<char>() + snap_at);
        // (copies are in cloud order: dst grows with the cloud, so the shift of the large clouds in front is looked up in step)
        size_t c = 0;
        for (const SiftBatchCopy& cp : copies) {
            while (batch_off[c + 1] <= cp.dst) ++c;
            const size_t dst = cp.dst + shift[c];
            memcpy(out_kp + dst * 4, h_kp + cp.src * 4, cp.count * 4 * sizeof(float));
            if (out_snap) memcpy(out_snap + dst, h_snap + cp.src, cp.count * sizeof(int32_t));
        }
    }
    for (size_t c = 0; c < n_clouds; ++c) {
        const size_t m = large_kp[c].size() / 4;
        if (!m) continue;
        memcpy(out_kp + out_offsets[c] * 4, large_kp[c].data(), m * 4 * sizeof(float));
        if (out_snap) {
            PCC_TRY(pcc_index_set_input(lease.w, batch.pts[c], batch.n[c], batch.stride, 3, PCC_MEM_HOST));
            PCC_TRY(pcc_first_within(lease.w, large_kp[c].data(), m, 4 * sizeof(float), PCC_MEM_HOST, snap_radius, out_snap + out_offsets[c]));
        }
    }
    return PCC_OK;
}

}  // namespace pcc

extern "C" {

int pcc_sift_keypoints_batch(pcc_index* ctx, size_t n_clouds, const void* const* pts, const size_t* n, size_t stride, const void* const* rgb,
                             size_t rgb_stride, int mem, float min_scale, int nr_octaves, int nr_scales_per_octave, float min_contrast,
                             double snap_radius, float* out_keypoints, int32_t* out_snap_index, size_t capacity, size_t* out_offsets) {
    using namespace pcc;
    // the arguments first: all of it host arithmetic, refused before the handle or any device is looked at
    const CloudBatch batch{n_clouds, pts, n, stride, rgb, rgb_stride};
    PCC_TRY(check_cloud_batch("pcc_sift_keypoints_batch", batch, mem));
    if (!out_offsets) { set_error("null out_offsets"); return PCC_ERR_INVALID; }
    if (n_clouds >= (1ull << 31)) { set_error("more than 2^31 clouds"); return PCC_ERR_UNSUPPORTED; }
    if ((n_clouds && (!pts || !n || !rgb)) || (capacity && !out_keypoints)) { set_error("null argument"); return PCC_ERR_INVALID; }
    if (rgb_stride < 4 || rgb_stride % 4 || (capacity && (reinterpret_cast<uintptr_t>(out_keypoints) % 4 || reinterpret_cast<uintptr_t>(out_snap_index) % 4))) {
        set_error("points, colour words and keypoints must be 4-byte aligned, the colour stride %zu a multiple of 4 and >= 4", rgb_stride);
        return PCC_ERR_INVALID;
    }
    PCC_TRY(check_sift_params(min_scale, nr_octaves, nr_scales_per_octave, min_contrast));
    if (out_snap_index && (!(snap_radius > 0) || !std::isfinite(snap_radius))) { set_error("bad radius"); return PCC_ERR_INVALID; }
    PCC_TRY(check_batch_clouds(batch, mem));
    // the first octave's lattice of every cloud (voxel_plan.hpp, as voxel.hip sizes it; the later octaves' leaves are larger)
    const float inv = 1.0f / min_scale;
    for (size_t c = 0; c < n_clouds; ++c) {
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        const char* p = static_cast<const char*>(pts[c]);
        bool any = false;
        for (size_t i = 0; i < n[c]; ++i) {
            float v[3];
            memcpy(v, p + i * stride, 12);
            if (!finite3(v[0], v[1], v[2])) continue;
            any = true;
            for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], v[a]); hi[a] = std::max(hi[a], v[a]); }
        }
        if (!any) continue;
        const VoxelPlan vp = voxel_plan(lo, hi, inv);
        if (vp.verdict == VOXEL_PLAN_RANGE) {
            set_error("cloud %zu: leaf size %g too small for this cloud: a voxel coordinate of its bounding box is beyond int32", c, min_scale);
            return PCC_ERR_UNSUPPORTED;
        }
        if (vp.verdict == VOXEL_PLAN_CELLS) {
            set_error("cloud %zu: leaf size %g too small for this cloud: %.0f voxels (limit %u)", c, min_scale, vp.cells, VOXEL_MAX_CELLS);
            return PCC_ERR_UNSUPPORTED;
        }
    }
    if (n_clouds == 0) { out_offsets[0] = 0; return PCC_OK; }  // (no device is touched: not even the handle's)
    PCC_ENTER(ctx);
    ev_next(ctx);
    ev_mark(ctx, EV_CALL0);
    const int st = sift_keypoints_batch(ctx, batch, min_scale, nr_octaves, nr_scales_per_octave, min_contrast, snap_radius, out_keypoints,
                                        out_snap_index, capacity, out_offsets);
    ev_mark(ctx, EV_CALL1);
    return st;
}
}  // extern "C"
