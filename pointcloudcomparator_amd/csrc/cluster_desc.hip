// cluster_desc.hip -- the per-cluster descriptor loop of a comparison in one call (gfx950): pcc_cluster_descriptors.
//
// The reference walks the clusters of both scenes (src/comparator.cpp:1224-1290): a cluster above 700 points takes
// processRIFTwithSIFT (SIFT keypoints, each snapped to the first cluster point within 0.05, RIFT over the snapped points), the
// others processRIFT over all their points, and every cluster's centroid is taken on the way.  With the batch calls that was
// pcc_sift_keypoints_batch, a host gather of the snapped clouds, pcc_rift_descriptors_batch and a host loop for the centroids --
// from host memory only.  Here the clusters, in host or device memory, are staged ONCE as 32-byte records (cluster_desc_plan.hpp:
// the SIFT batch route's clusters first, so that the staged prefix IS the first concatenation of the octave rounds) and stay on
// the device:
//   1. pack: from host memory on the host into one pinned buffer, one copy; from device memory by k_cd_pack from the strided
//      records, 16-byte loads where stride and alignment allow.  Every record carries its cluster and its local index.
//   2. k_cd_centroids: one wave per cluster, its points loaded coalesced 64 at a time and parked in LDS, three lanes each adding
//      one coordinate in index order -- the reference's float accumulation, bit for bit: no tree, no atomics, no double.
//   3. the octave rounds of sift_batch.hip and k_sb_snap as they are (desc_batch.hpp); clusters above
//      PCC_OPT_SIFT_BATCH_BRUTE_MAX take pcc_sift_keypoints' path and pcc_first_within on the work handle, from the staged
//      records.  Neither keypoints nor snap indices cross to the host: the host knows only how many each round found per cluster.
//   4. the snapped clouds: the host uploads where keypoint k of the (cluster, round, point, scale) order lies; the hits are
//      flagged, scanned, and counted per cluster (THE wait this stage adds); k_cd_assemble then writes every cluster's RIFT cloud
//      -- its own records on the dense route, the records at its snap indices, duplicates kept and misses dropped, on the SIFT
//      route -- as float4 (w = bits(position)) + colour word + the cluster-local index of the source point.
//   5. rift_batch.hip's stages over the concatenation of the clouds up to PCC_OPT_RIFT_BATCH_BRUTE_MAX; larger ones lie behind
//      the concatenation and take pcc_rift_descriptors on the work handle, in device memory.  k_cd_compose turns the point index
//      of every descriptor into the cluster-local index of the point it was computed at (S[J] on the SIFT route).
// Launches and host waits depend on nr_octaves, on the clusters above the limits and on buffer growth, never on n_clusters.
#include <algorithm>
#include <cmath>
#include <vector>

#include "entry.hpp"
#include "lane_ops.hpp"
#include "rift_math.hpp"
#include "desc_batch.hpp"
#include "cluster_desc_plan.hpp"

namespace pcc {

namespace {

// ---- 1. the pack from device memory ---------------------------------------------------------------------------------------------
// Point e of the caller's range (cl_off[c] <= e < cl_off[c + 1] for its cluster c) -> record stage_base[c] + (e - cl_off[c]).
// V16: the records are 16-byte aligned and a multiple of 16 bytes apart: x, y, z in one load.
template <bool V16>
__global__ void __launch_bounds__(256)
k_cd_pack(const unsigned char* __restrict__ pts, size_t stride, const unsigned char* __restrict__ rgb, size_t rgb_stride,
          const unsigned int* __restrict__ cl_off, const unsigned int* __restrict__ stage_base, unsigned int n_clusters, unsigned int total,
          SiftRec* __restrict__ out) {
    for (unsigned int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const unsigned int c = range_of(cl_off, n_clusters, e);
        const unsigned int j = e - cl_off[c];
        SiftRec r;
        if constexpr (V16) {
            const float4 v = *reinterpret_cast<const float4*>(pts + (size_t)e * stride);
            r.x = v.x; r.y = v.y; r.z = v.z;
        } else {
            const float* v = reinterpret_cast<const float*>(pts + (size_t)e * stride);
            r.x = v[0]; r.y = v[1]; r.z = v[2];
        }
        r.w = 1.0f;
        r.rgb = *reinterpret_cast<const uint32_t*>(rgb + (size_t)e * rgb_stride);
        r.pad[0] = c; r.pad[1] = j; r.pad[2] = 0u;
        out[stage_base[c] + j] = r;
    }
}

// ---- 2. centroids ---------------------------------------------------------------------------------------------------------------
// One wave (one 64-lane workgroup) per cluster: out[c] = (sum of x, sum of y, sum of z) / float(n), every sum a float chain
// from 0.0f over the points in index order, non-finite points included; n == 0 gives 0.0f / 0.0f = NaN.  The wave loads its
// points 64 at a time, coalesced, CD_CENT_ROWS such rows in flight, and parks them in LDS; lanes 0, 1 and 2 then each carry one
// serial chain over the parked tile while the loads of the NEXT tile are under way: a tile's 512 dependent additions take about
// as long as its loads do to arrive (a row at a time the chain would wait for memory after every 64 links -- measured, 11.6 ms
// for 250 000 points: EXPERIMENTS.md).
constexpr unsigned int CD_CENT_ROWS = 8;
constexpr unsigned int CD_CENT_TILE = 64 * CD_CENT_ROWS;

__global__ void __launch_bounds__(64)
k_cd_centroids(const SiftRec* __restrict__ rec, const unsigned int* __restrict__ stage_base, const unsigned int* __restrict__ cl_off,
               unsigned int n_clusters, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float park[3][CD_CENT_TILE];
    const unsigned int lane = threadIdx.x;
    for (unsigned int c = blockIdx.x; c < n_clusters; c += gridDim.x) {  // block-uniform
        const unsigned int n = cl_off[c + 1] - cl_off[c];
        const SiftRec* __restrict__ cloud = rec + stage_base[c];
        float4 next[CD_CENT_ROWS];  // (x, y, z, w: the first half of a record)
        auto load = [&](unsigned int t0) {
#pragma unroll
            for (unsigned int r = 0; r < CD_CENT_ROWS; ++r) {
                const unsigned int i = t0 + r * 64 + lane;
                next[r] = i < n ? *reinterpret_cast<const float4*>(cloud + i) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        };
        float acc = 0.0f;
        if (n) load(0);
        for (unsigned int t0 = 0; t0 < n; t0 += CD_CENT_TILE) {
            const unsigned int tn = min(CD_CENT_TILE, n - t0);
            __syncthreads();  // (the tile before has been added up)
#pragma unroll
            for (unsigned int r = 0; r < CD_CENT_ROWS; ++r) {
                park[0][r * 64 + lane] = next[r].x; park[1][r * 64 + lane] = next[r].y; park[2][r * 64 + lane] = next[r].z;
            }
            __syncthreads();
            if (t0 + CD_CENT_TILE < n) load(t0 + CD_CENT_TILE);
            if (lane < 3) {
                // the chain, 32 links at a time: eight 16-byte LDS reads in flight, then their additions in index order (one
                // read per link would put the LDS latency into every link)
                const float* __restrict__ row = park[lane];
                unsigned int j = 0;
                for (; j + 32 <= tn; j += 32) {
                    float4 q[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) q[k] = *reinterpret_cast<const float4*>(row + j + 4 * k);
#pragma unroll
                    for (int k = 0; k < 8; ++k) { acc += q[k].x; acc += q[k].y; acc += q[k].z; acc += q[k].w; }
                }
                for (; j < tn; ++j) acc += row[j];  // (entries at tn and beyond are not added)
            }
        }
        if (lane < 3) out[(size_t)c * 3 + lane] = acc / (float)n;
    }
}

// ---- 4. the snapped clouds ------------------------------------------------------------------------------------------------------
// flags[k] = 1 where keypoint k of the cluster-major order (order[k]: its place on the device) found a point; flags[m] = 0
__global__ void __launch_bounds__(256)
k_cd_flags(const int32_t* __restrict__ snap, const unsigned int* __restrict__ order, unsigned int m, unsigned int* __restrict__ flags) {
    for (unsigned int k = blockIdx.x * blockDim.x + threadIdx.x; k <= m; k += gridDim.x * blockDim.x)
        flags[k] = k < m && snap[order[k]] >= 0 ? 1u : 0u;
}

// hits[c] = pos[kbase[c + 1]] - pos[kbase[c]]: the snapped points of cluster c (pos: the exclusive scan of the flags)
__global__ void __launch_bounds__(256)
k_cd_hits(const unsigned int* __restrict__ pos, const unsigned int* __restrict__ kbase, unsigned int n_clusters, unsigned int* __restrict__ hits) {
    for (unsigned int c = blockIdx.x * blockDim.x + threadIdx.x; c < n_clusters; c += gridDim.x * blockDim.x)
        hits[c] = pos[kbase[c + 1]] - pos[kbase[c]];
}

// Every cluster's RIFT cloud at dst[c]: threads [0, n_staged) take a staged record each (a dense-route cluster copies it to
// dst[c] + local index), threads [n_staged, n_staged + m) a keypoint of the cluster-major order each (a hit of rank r among its
// cluster's hits puts the record at its snap index to dst[c] + r).  src[d]: the cluster-local index of the point at d.
__global__ void __launch_bounds__(256)
k_cd_assemble(const SiftRec* __restrict__ rec, unsigned int n_staged, const unsigned int* __restrict__ stage_base, const unsigned int* __restrict__ cl_off,
              const unsigned int* __restrict__ route, const unsigned int* __restrict__ dst, unsigned int n_clusters, unsigned int n_out,
              const int32_t* __restrict__ snap, const unsigned int* __restrict__ order, const unsigned int* __restrict__ pos,
              const unsigned int* __restrict__ kbase, unsigned int m, float4* __restrict__ out_pts, uint32_t* __restrict__ out_rgb,
              int32_t* __restrict__ out_src) {
    const unsigned int all = n_staged + m;
    for (unsigned int t = blockIdx.x * blockDim.x + threadIdx.x; t < all; t += gridDim.x * blockDim.x) {
        SiftRec p;
        unsigned int d, j;
        if (t < n_staged) {
            p = rec[t];
            const unsigned int c = p.pad[0];
            j = p.pad[1];
            if (c >= n_clusters || route[c] != CD_DENSE) continue;
            d = dst[c] + j;
        } else {
            const unsigned int k = t - n_staged;
            if (pos[k + 1] == pos[k]) continue;  // a miss
            const unsigned int c = range_of(kbase, n_clusters, k);
            j = (unsigned int)snap[order[k]];
            if (j >= cl_off[c + 1] - cl_off[c]) continue;  // (cannot happen: the snap answers a local index of its cluster)
            p = rec[stage_base[c] + j];
            d = dst[c] + (pos[k] - pos[kbase[c]]);
        }
        if (d >= n_out) continue;  // (cannot happen: dst was sized from these very counts)
        out_pts[d] = make_float4(p.x, p.y, p.z, __uint_as_float(d));
        out_rgb[d] = p.rgb;
        out_src[d] = (int32_t)j;
    }
}

// ---- 5. the point index of every descriptor ---------------------------------------------------------------------------------------
// Behind k_batch_finish: row r of the kept rows belongs to the cloud c with slice[c] <= r < slice[c + 1] and holds the
// index of its point within that cloud; src[bases[c] + that] is the cluster-local index the caller is told.
__global__ void __launch_bounds__(256)
k_cd_compose(const unsigned int* __restrict__ slice, const unsigned int* __restrict__ bases, unsigned int n_clusters, const int32_t* __restrict__ src,
             int32_t* __restrict__ index) {
    const unsigned int kept = slice[n_clusters];
    for (unsigned int r = blockIdx.x * blockDim.x + threadIdx.x; r < kept; r += gridDim.x * blockDim.x) {
        const unsigned int c = range_of(slice, n_clusters, r);
        index[r] = src[bases[c] + (unsigned int)index[r]];
    }
}
// the same for the m rows of ONE cloud off the batch route (src: its part of the source indices)
__global__ void __launch_bounds__(256)
k_cd_remap(const int32_t* __restrict__ src, unsigned int m, int32_t* __restrict__ index) {
    for (unsigned int r = blockIdx.x * blockDim.x + threadIdx.x; r < m; r += gridDim.x * blockDim.x) index[r] = src[(unsigned int)index[r]];
}

}  // namespace

// (up: octaves + tables + records; up2: the keypoint order, then the RIFT tables; down: hits per cluster, centroids; dev: what `up` holds)
struct ClusterDescScratch : BatchStaging {
    static constexpr ScratchSlot slot = SCRATCH_CLUSTER_DESC;
    HostBuf up2;
    DevBuf korder, tab;           // what up2 holds on the device: kbase + keypoint order; GridDev + bases + items + dst
    DevBuf snap;                  // int32 per keypoint: the rounds' (round-major), then the work handle's cluster by cluster
    DevBuf flags, scan_tmp, hits; // hit flags / positions uint32[m + 1]; uint32[n_clusters]
    DevBuf cat_pts, cat_rgb, cat_src;  // every cluster's RIFT cloud: float4, colour word, cluster-local source index
    DevBuf lhist, lindex;         // the rows of one cloud off the batch route
    DevBuf cent;                  // float[n_clusters][3]
};

namespace {

struct ClusterDescArgs {
    const unsigned char* pts;
    size_t stride;
    const unsigned char* rgb;
    size_t rgb_stride;
    const size_t* offsets;
    size_t n_clusters;
    int mem;
    size_t sift_above;
    float min_scale;
    int nr_octaves, nr_scales_per_octave;
    float min_contrast;
    double snap_radius, normal_radius, gradient_radius, rift_radius;
    float* out_hist;
    int32_t* out_index;
    size_t capacity;
    size_t* out_offsets;
    uint32_t* out_n_keypoints;
    float* out_centroids;
};

int cluster_descriptors(pcc_index* ix, const ClusterDescArgs& a) {
    hipStream_t s = ix->stream;
    const size_t n_clusters = a.n_clusters;
    PCC_TRY(sync_info(ix));  // (a pending mirror of the handle's own grid would overwrite stats[2] later)
    ClusterDescScratch* sc = scratch<ClusterDescScratch>(ix);
    const size_t sift_max = (size_t)ix->opt.sift_batch_brute_max, rift_max = (size_t)ix->opt.rift_batch_brute_max;
    const ClusterDescRoutes routes = cd_routes(a.offsets, n_clusters, a.sift_above, sift_max);
    const size_t total = routes.stage_base[n_clusters], off0 = a.offsets[0];
    const unsigned int nc = (unsigned int)n_clusters;

    // ---- 1. one staging: octaves | the rounds' first table | cluster offsets | stage bases | routes | 32 bytes a point ----------
    SiftBatchRound round0;
    sift_batch_round(routes.sift_n.data(), n_clusters, 0, &round0);
    round0.items.clear();  // (the first round needs no items: the voxel stage works by cloud)
    const std::vector<SiftOctave> h_octaves = sift_batch_octaves(a.min_scale, a.nr_octaves, a.nr_scales_per_octave, a.min_contrast);
    const size_t oct_bytes = align_up(h_octaves.size() * sizeof(SiftOctave), 16);
    const TableLayout t0(n_clusters, 0, oct_bytes);
    const size_t words = align_up((n_clusters + 1) * sizeof(uint32_t), 16);
    const size_t cl_at = t0.bytes, stage_at = cl_at + words, route_at = stage_at + words, rec_at = align_up(route_at + words, 32);
    const size_t all_bytes = rec_at + total * sizeof(SiftRec);
    const bool host = a.mem == PCC_MEM_HOST;
    PCC_TRY(sc->up.reserve(host ? all_bytes : rec_at));
    PCC_TRY(sc->dev.reserve(all_bytes));
    char* u = sc->up.as<char>();
    memset(u, 0, rec_at);
    memcpy(u, h_octaves.data(), h_octaves.size() * sizeof(SiftOctave));
    t0.fill(u, round0);
    uint32_t* h_cl = reinterpret_cast<uint32_t*>(u + cl_at);
    for (size_t c = 0; c <= n_clusters; ++c) h_cl[c] = (uint32_t)(a.offsets[c] - off0);
    memcpy(u + stage_at, routes.stage_base.data(), (n_clusters + 1) * sizeof(uint32_t));
    memcpy(u + route_at, routes.route.data(), n_clusters * sizeof(uint32_t));
    char* d0 = sc->dev.as<char>();
    SiftRec* d_rec = reinterpret_cast<SiftRec*>(d0 + rec_at);
    const unsigned int* d_cl = reinterpret_cast<const unsigned int*>(d0 + cl_at);
    const unsigned int* d_stage = reinterpret_cast<const unsigned int*>(d0 + stage_at);
    const unsigned int* d_route = reinterpret_cast<const unsigned int*>(d0 + route_at);
    const unsigned char* p0 = a.pts + off0 * a.stride;
    const unsigned char* c0 = a.rgb + off0 * a.rgb_stride;
    if (host) {
        SiftRec* rec = reinterpret_cast<SiftRec*>(u + rec_at);
        for (size_t c = 0; c < n_clusters; ++c) {
            const unsigned char* src = p0 + (size_t)h_cl[c] * a.stride;
            const unsigned char* col = c0 + (size_t)h_cl[c] * a.rgb_stride;
            for (size_t i = 0; i < routes.n[c]; ++i) {
                SiftRec& p = rec[routes.stage_base[c] + i];
                memcpy(&p.x, src + i * a.stride, 12);
                p.w = 1.0f;
                memcpy(&p.rgb, col + i * a.rgb_stride, 4);
                p.pad[0] = (uint32_t)c; p.pad[1] = (uint32_t)i; p.pad[2] = 0u;
            }
        }
        PCC_HIP(hipMemcpyAsync(d0, u, all_bytes, hipMemcpyHostToDevice, s));
    } else {
        PCC_HIP(hipMemcpyAsync(d0, u, rec_at, hipMemcpyHostToDevice, s));
        if (total) {
            const bool v16 = a.stride % 16 == 0 && reinterpret_cast<uintptr_t>(p0) % 16 == 0;
            if (v16)
                hipLaunchKernelGGL((k_cd_pack<true>), dim3(blocks_for(total)), dim3(256), 0, s, p0, a.stride, c0, a.rgb_stride, d_cl, d_stage, nc,
                                   (unsigned int)total, d_rec);
            else
                hipLaunchKernelGGL((k_cd_pack<false>), dim3(blocks_for(total)), dim3(256), 0, s, p0, a.stride, c0, a.rgb_stride, d_cl, d_stage, nc,
                                   (unsigned int)total, d_rec);
            PCC_HIP(hipGetLastError());
        }
    }

    // ---- 2. centroids ------------------------------------------------------------------------------------------------------------
    if (a.out_centroids) {
        PCC_TRY(sc->cent.reserve(n_clusters * 3 * sizeof(float)));
        hipLaunchKernelGGL(k_cd_centroids, dim3((unsigned int)std::min<size_t>(n_clusters, 4096)), dim3(64), 0, s, d_rec, d_stage, d_cl, nc,
                           sc->cent.as<float>());
        PCC_HIP(hipGetLastError());
    }

    // ---- 3. SIFT keypoints and their snap: the rounds, then the clusters above the limit on the work handle ------------------------
    SiftBatchResult res;
    if (routes.sift_batch_total) {
        SiftBatchInput in;
        in.round0 = &round0;
        in.h_octaves = &h_octaves;
        in.d_octaves = reinterpret_cast<const SiftOctave*>(d0);
        in.d_bases0 = reinterpret_cast<const unsigned int*>(d0 + t0.bases_at);
        in.d_bases64_0 = reinterpret_cast<const int64_t*>(d0 + t0.bases64_at);
        in.d_rec0 = d_rec;
        PCC_TRY(sift_batch_rounds(ix, n_clusters, in, a.min_scale, &res));
    }
    const size_t m_batch = res.total;
    if (m_batch) {
        PCC_TRY(sc->snap.reserve(m_batch * sizeof(int32_t)));
        PCC_TRY(sift_batch_snap(ix, res, n_clusters, a.snap_radius, sc->snap.as<int32_t>()));
    }
    WorkLease lease;
    uint64_t work_points = 0;
    std::vector<uint32_t> work_counts(n_clusters, 0u);
    size_t m_all = m_batch;
    for (size_t c = 0; c < n_clusters; ++c) {
        if (routes.route[c] != CD_SIFT_WORK) continue;
        if (!lease.w) PCC_TRY(lease.take(ix, sc->work, true));
        pcc_index* w = lease.w;
        const size_t n = routes.n[c];
        const unsigned char* rp = reinterpret_cast<const unsigned char*>(d_rec + routes.stage_base[c]);
        work_points += n;
        entered(w);
        size_t found = 0;
        PCC_TRY(sift_keypoints(w, rp, n, sizeof(SiftRec), rp + 16, sizeof(SiftRec), a.min_scale, a.nr_octaves, a.nr_scales_per_octave, a.min_contrast,
                               &found));
        if (!found) continue;
        PCC_TRY(sc->snap.grow_keep(ix->stream, m_all * sizeof(int32_t), (m_all + found) * sizeof(int32_t)));
        PCC_TRY(pcc_index_set_input(w, rp, n, sizeof(SiftRec), 3, PCC_MEM_DEVICE));
        PCC_TRY(pcc_first_within(w, scratch<SiftScratch>(w)->kp.p, found, sizeof(float4), PCC_MEM_DEVICE, a.snap_radius, sc->snap.as<int32_t>() + m_all));
        work_counts[c] = (uint32_t)found;
        m_all += found;
    }

    // ---- 4. the snapped points of every cluster: flags, scan, counts (the wait), then every cluster's RIFT cloud -------------------
    std::vector<uint32_t> kbase, korder;
    cd_keypoint_order(res.counts, work_counts, n_clusters, &kbase, &korder);
    std::vector<size_t> q_n(routes.n);
    const unsigned int *d_kbase = nullptr, *d_korder = nullptr;
    uint64_t snapped = 0;
    if (m_all) {
        const size_t order_at = align_up((n_clusters + 1) * sizeof(uint32_t), 16), bytes = order_at + m_all * sizeof(uint32_t);
        PCC_TRY(sc->up2.reserve(bytes));
        PCC_TRY(sc->korder.reserve(bytes));
        char* u2 = sc->up2.as<char>();
        memcpy(u2, kbase.data(), (n_clusters + 1) * sizeof(uint32_t));
        memcpy(u2 + order_at, korder.data(), m_all * sizeof(uint32_t));
        PCC_HIP(hipMemcpyAsync(sc->korder.p, u2, bytes, hipMemcpyHostToDevice, s));
        d_kbase = sc->korder.as<unsigned int>();
        d_korder = reinterpret_cast<const unsigned int*>(sc->korder.as<char>() + order_at);
        PCC_TRY(sc->flags.reserve((m_all + 1) * sizeof(unsigned int)));
        PCC_TRY(sc->hits.reserve(n_clusters * sizeof(unsigned int)));
        PCC_TRY(sc->down.reserve(n_clusters * sizeof(unsigned int)));
        hipLaunchKernelGGL(k_cd_flags, dim3(blocks_for(m_all + 1)), dim3(256), 0, s, sc->snap.as<int32_t>(), d_korder, (unsigned int)m_all,
                           sc->flags.as<unsigned int>());
        PCC_HIP(hipGetLastError());
        PCC_TRY(launch_exclusive_scan(ix, s, sc->flags.as<unsigned int>(), m_all + 1, sc->scan_tmp));
        hipLaunchKernelGGL(k_cd_hits, dim3(blocks_for(n_clusters)), dim3(256), 0, s, sc->flags.as<unsigned int>(), d_kbase, nc, sc->hits.as<unsigned int>());
        PCC_HIP(hipGetLastError());
        PCC_HIP(hipMemcpyAsync(sc->down.p, sc->hits.p, n_clusters * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
        PCC_HIP(hipStreamSynchronize(s));  // THE wait of this stage: the snapped points of every cluster
        const unsigned int* h_hits = sc->down.as<unsigned int>();
        for (size_t c = 0; c < n_clusters; ++c)
            if (routes.route[c] != CD_DENSE) { q_n[c] = h_hits[c]; snapped += h_hits[c]; }
    } else {
        for (size_t c = 0; c < n_clusters; ++c)
            if (routes.route[c] != CD_DENSE) q_n[c] = 0;
    }
    const ClusterDescClouds clouds = cd_clouds(q_n.data(), n_clusters, rift_max);
    const size_t cat_total = clouds.dst[n_clusters], batch_total = clouds.bases[n_clusters];

    ix->stats[0] = routes.n_dense;
    ix->stats[1] = routes.n_sift;
    ix->stats[2] = res.rounds;
    ix->stats[3] = kbase[n_clusters];
    ix->stats[4] = snapped;
    own_counters(ix, work_points + clouds.n_single);

    const unsigned int* h_slice = nullptr;
    std::vector<unsigned int> no_slice(n_clusters + 1, 0u);
    const char* dt = nullptr;
    if (cat_total) {
        // the RIFT tables in one copy: the order's n_valid word, bases, work items, dst
        const ConcatLayout L(sizeof(GridDev), 128, n_clusters, clouds.items.size(), 0);
        const size_t dst_at = align_up(L.pts_at, 16), bytes = dst_at + (n_clusters + 1) * sizeof(uint32_t);
        PCC_TRY(sc->up2.reserve(bytes));  // (nothing is in flight from it: the wait above, or it has not been used)
        PCC_TRY(sc->tab.reserve(bytes));
        char* u3 = sc->up2.as<char>();
        memset(u3, 0, L.items_at);
        reinterpret_cast<GridDev*>(u3)->n_valid = (unsigned int)batch_total;
        memcpy(u3 + L.bases_at, clouds.bases.data(), (n_clusters + 1) * sizeof(uint32_t));
        if (!clouds.items.empty()) memcpy(u3 + L.items_at, clouds.items.data(), clouds.items.size() * sizeof(RiftBatchItem));
        memcpy(u3 + dst_at, clouds.dst.data(), (n_clusters + 1) * sizeof(uint32_t));
        PCC_HIP(hipMemcpyAsync(sc->tab.p, u3, bytes, hipMemcpyHostToDevice, s));
        dt = sc->tab.as<char>();
        PCC_TRY(sc->cat_pts.reserve(cat_total * sizeof(float4)));
        PCC_TRY(sc->cat_rgb.reserve(cat_total * sizeof(uint32_t)));
        PCC_TRY(sc->cat_src.reserve(cat_total * sizeof(int32_t)));
        hipLaunchKernelGGL(k_cd_assemble, dim3(blocks_for(total + m_all)), dim3(256), 0, s, d_rec, (unsigned int)total, d_stage, d_cl, d_route,
                           reinterpret_cast<const unsigned int*>(dt + dst_at), nc, (unsigned int)cat_total, sc->snap.as<int32_t>(), d_korder,
                           sc->flags.as<unsigned int>(), d_kbase, (unsigned int)m_all, sc->cat_pts.as<float4>(), sc->cat_rgb.as<uint32_t>(),
                           sc->cat_src.as<int32_t>());
        PCC_HIP(hipGetLastError());

        // ---- 5. RIFT over the concatenation ----------------------------------------------------------------------------------------
        if (batch_total) {
            RiftBatchInput in;
            in.n_clouds = n_clusters;
            in.total = batch_total;
            in.gd = reinterpret_cast<const GridDev*>(dt);
            in.d_bases = reinterpret_cast<const unsigned int*>(dt + L.bases_at);
            in.d_items = reinterpret_cast<const RiftBatchItem*>(dt + L.items_at);
            in.n_items = (unsigned int)clouds.items.size();
            in.d_pts = sc->cat_pts.as<float4>();
            in.d_rgb = sc->cat_rgb.as<unsigned char>();
            const unsigned int* d_slice = nullptr;
            PCC_TRY(rift_batch_run(ix, in, a.normal_radius, a.gradient_radius, a.rift_radius, &d_slice));
            hipLaunchKernelGGL(k_cd_compose, dim3(blocks_for(batch_total)), dim3(256), 0, s, d_slice, in.d_bases, nc,
                               sc->cat_src.as<int32_t>(), scratch<RiftScratch>(ix)->out_index.as<int32_t>());
            PCC_HIP(hipGetLastError());
            PCC_TRY(rift_batch_slices(ix, n_clusters, &h_slice));
        }
    }
    if (!h_slice) h_slice = no_slice.data();

    // ---- the clouds above the limit: the single path on the work handle, from the device ------------------------------------------
    std::vector<size_t> single_m(n_clusters, 0);
    std::vector<std::vector<float>> single_hist(n_clusters);
    std::vector<std::vector<int32_t>> single_index(n_clusters);
    for (size_t c = 0; c < n_clusters; ++c) {
        if (q_n[c] <= rift_max) continue;
        if (!lease.w) PCC_TRY(lease.take(ix, sc->work, true));
        pcc_index* w = lease.w;
        const size_t n = q_n[c], at = clouds.dst[c];
        PCC_TRY(pcc_index_set_input(w, sc->cat_pts.as<float4>() + at, n, sizeof(float4), 3, PCC_MEM_DEVICE));
        size_t n_valid = 0;
        PCC_TRY(pcc_index_size(w, &n_valid));
        if (!n_valid) continue;  // (the single path answers PCC_ERR_EMPTY there)
        PCC_TRY(sc->lhist.reserve(n * RIFT_BINS * sizeof(float)));
        PCC_TRY(sc->lindex.reserve(n * sizeof(int32_t)));
        size_t m = 0;
        PCC_TRY(pcc_rift_descriptors(w, sc->cat_rgb.as<uint32_t>() + at, sizeof(uint32_t), PCC_MEM_DEVICE, a.normal_radius, a.gradient_radius,
                                     a.rift_radius, RIFT_D_BINS, RIFT_G_BINS, sc->lhist.as<float>(), sc->lindex.as<int32_t>(), &m));
        single_m[c] = m;
        if (!m) continue;
        hipLaunchKernelGGL(k_cd_remap, dim3(blocks_for(m)), dim3(256), 0, s, sc->cat_src.as<int32_t>() + at, (unsigned int)m, sc->lindex.as<int32_t>());
        PCC_HIP(hipGetLastError());
        single_hist[c].resize(m * RIFT_BINS);
        single_index[c].resize(m);
        PCC_HIP(hipMemcpyAsync(single_hist[c].data(), sc->lhist.p, m * RIFT_BINS * sizeof(float), hipMemcpyDeviceToHost, s));
        PCC_HIP(hipMemcpyAsync(single_index[c].data(), sc->lindex.p, m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        PCC_HIP(hipStreamSynchronize(s));
    }

    // ---- the slices, in cluster order ----------------------------------------------------------------------------------------------
    std::vector<size_t> offsets;
    std::vector<ClusterDescCopy> copies;
    cd_splice(h_slice, q_n.data(), single_m.data(), n_clusters, rift_max, &offsets, &copies);
    for (size_t c = 0; c <= n_clusters; ++c) a.out_offsets[c] = offsets[c];
    const size_t n_out = offsets[n_clusters], kept = h_slice[n_clusters];
    if (n_out > a.capacity) {
        set_error("%zu descriptors, room for %zu", n_out, a.capacity);
        return PCC_ERR_OVERFLOW;
    }
    if (a.out_centroids) {
        PCC_TRY(sc->down.reserve(n_clusters * 3 * sizeof(float)));  // (the hits have been read)
        PCC_HIP(hipMemcpyAsync(sc->down.p, sc->cent.p, n_clusters * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
    }
    if (clouds.n_single == 0) {
        PCC_TRY(rift_batch_fetch(ix, kept, a.out_hist, a.out_index));  // (the slices are the caller's: one copy each, in place)
    } else {
        std::vector<float> bh(std::max<size_t>(kept, 1) * RIFT_BINS);
        std::vector<int32_t> bi(std::max<size_t>(kept, 1));
        PCC_TRY(rift_batch_fetch(ix, kept, bh.data(), bi.data()));
        for (const ClusterDescCopy& cp : copies) {
            memcpy(a.out_hist + cp.dst * RIFT_BINS, bh.data() + cp.src * RIFT_BINS, cp.count * RIFT_BINS * sizeof(float));
            memcpy(a.out_index + cp.dst, bi.data() + cp.src, cp.count * sizeof(int32_t));
        }
        for (size_t c = 0; c < n_clusters; ++c) {
            if (!single_m[c]) continue;
            memcpy(a.out_hist + offsets[c] * RIFT_BINS, single_hist[c].data(), single_m[c] * RIFT_BINS * sizeof(float));
            memcpy(a.out_index + offsets[c], single_index[c].data(), single_m[c] * sizeof(int32_t));
        }
    }
    PCC_HIP(hipStreamSynchronize(s));  // (the centroids; the staging buffers are free again)
    if (a.out_centroids) memcpy(a.out_centroids, sc->down.p, n_clusters * 3 * sizeof(float));
    if (a.out_n_keypoints)
        for (size_t c = 0; c < n_clusters; ++c) a.out_n_keypoints[c] = kbase[c + 1] - kbase[c];
    return PCC_OK;
}

}  // namespace

}  // namespace pcc

extern "C" {

int pcc_cluster_descriptors(pcc_index* ctx, const void* pts, size_t stride_bytes, const void* rgb, size_t rgb_stride_bytes, const size_t* offsets,
                            size_t n_clusters, int mem, size_t sift_above, float min_scale, int nr_octaves, int nr_scales_per_octave,
                            float min_contrast, double snap_radius, double normal_radius, double gradient_radius, double rift_radius,
                            int nr_distance_bins, int nr_gradient_bins, float* out_histograms, int32_t* out_point_index, size_t capacity,
                            size_t* out_offsets, uint32_t* out_n_keypoints, float* out_centroids) {
    using namespace pcc;
    // the arguments first: all of it host arithmetic, refused before the handle or any device is looked at
    // 1. the memory space
    PCC_TRY(check_mem(mem));
    // 2. null arrays (the clusters' arrays may be null while no cluster holds a point)
    if (!offsets || !out_offsets) { set_error("null argument"); return PCC_ERR_INVALID; }
    const bool any_points = n_clusters && offsets[n_clusters] != offsets[0];
    if ((any_points && (!pts || !rgb)) || (capacity && (!out_histograms || !out_point_index))) { set_error("null argument"); return PCC_ERR_INVALID; }
    // 3. strides and alignment
    PCC_TRY(check_points(nullptr, 0, stride_bytes, mem));  // (the stride alone)
    if (rgb_stride_bytes < 4 || rgb_stride_bytes % 4 || reinterpret_cast<uintptr_t>(pts) % 4 || reinterpret_cast<uintptr_t>(rgb) % 4 ||
        (capacity && (reinterpret_cast<uintptr_t>(out_histograms) % 4 || reinterpret_cast<uintptr_t>(out_point_index) % 4))) {
        set_error("points, colour words and descriptors must be 4-byte aligned, the colour stride %zu a multiple of 4 and >= 4", rgb_stride_bytes);
        return PCC_ERR_INVALID;
    }
    // 4. the offsets
    PCC_TRY(check_cluster_offsets({{offsets, n_clusters}}, "points in one batch"));
    // 5. to 7. the parameters
    PCC_TRY(check_sift_params(min_scale, nr_octaves, nr_scales_per_octave, min_contrast));
    PCC_TRY(check_rift_params(normal_radius, gradient_radius, rift_radius, nr_distance_bins, nr_gradient_bins));
    if (!(snap_radius > 0) || !std::isfinite(snap_radius)) { set_error("bad radius"); return PCC_ERR_INVALID; }
    if (n_clusters == 0) { out_offsets[0] = 0; return PCC_OK; }  // (no device is touched: not even the handle's)
    // 8. the handle
    PCC_ENTER(ctx);
    ev_next(ctx);
    ev_mark(ctx, EV_CALL0);
    const ClusterDescArgs a{static_cast<const unsigned char*>(pts), stride_bytes, static_cast<const unsigned char*>(rgb), rgb_stride_bytes, offsets,
                            n_clusters, mem, sift_above, min_scale, nr_octaves, nr_scales_per_octave, min_contrast, snap_radius, normal_radius,
                            gradient_radius, rift_radius, out_histograms, out_point_index, capacity, out_offsets, out_n_keypoints, out_centroids};
    const int st = cluster_descriptors(ctx, a);
    ev_mark(ctx, EV_CALL1);
    return st;
}
}  // extern "C"
