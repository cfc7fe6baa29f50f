// segment.hip -- the reference's DEFAULT segmentation path in one call (gfx950), and its last step as a kernel.
//
// pcc_extract_clusters: "labels -> one cloud per cluster", the step both segmentation paths of the reference end with
// (src/segmentation.cpp:133-152 and :290-318: for every cluster, in order, cloud[j] for every index j of the cluster).  With
// the clusters given as labels this is a STABLE partition of the point indices by label -- np.argsort(labels, kind="stable")
// without the -1 entries.  cell_sort does not give that (its order inside a cell is unspecified, voxel.hip), and neither does a
// rank taken from an atomicAdd's return value.  Here: LSD radix passes over 8-bit digits of the key (the label; a point that
// is left out carries the key n_clusters and sorts behind every cluster), one pass for up to 255 clusters, which is the
// reference's regime.  A pass is
//   k_seg_hist     every workgroup counts the digits of ONE contiguous chunk of the current order in LDS -> table[digit][block]
//   exclusive scan over the table (pack.hip): entry [d][b] becomes the first slot of digit d in block b's chunk
//   k_seg_scatter  every workgroup walks its chunk again, 256 entries at a time, in order: a lane's rank among the lanes of its
//                  wave with the same digit comes from eight ballots and a population count of the lanes below it, the waves
//                  in front add their counts through LDS, the tiles in front are in the running base -- ranks in lane
//                  order, so equal keys keep their order
// The only atomics are the LDS counters of k_seg_hist (sums of integers: the same whatever the order; one add per group of
// lanes with the same digit).  The offsets come out of
// the sorted keys (k_seg_offsets: the first position of every key), the records from a gather of whole words.
//
// pcc_region_growing_segmentation: region_growing_segmentation (src/segmentation.cpp:218-327): VoxelGrid -> NormalEstimation ->
// RegionGrowing -> one cloud per cluster, the filtered cloud, its index, its rows, its normals and its labels on the device
// from the raw cloud to the cluster clouds.
//
// pcc_euclidean_cluster_segmentation: euclidean_cluster_segmentation (src/segmentation.cpp:64-156): VoxelGrid -> the plane-removal
// loop -> EuclideanClusterExtraction -> one cloud per cluster, the same way.
#include "entry.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace pcc {

struct SegmentScratch : Scratch {
    static constexpr ScratchSlot slot = SCRATCH_SEGMENT;
    WorkHandle work;                 // the handle the filtered cloud is indexed on (the caller's stream and options, scratch of its own)
    DevBuf cloud, normals, labels;   // the filtered cloud's records, float4[nv], int32[nv]: nothing voxel_grid, the k-NN rows, the
                                     // plane fit, the plane loop, grid_region_growing or grid_clusters reserves
    DevBuf remain;                   // pcc_euclidean_cluster_segmentation: the records that remain after the planes (a caller in host memory)
    DevBuf lab_in;                   // pcc_extract_clusters: the caller's labels, staged (host memory)
    DevBuf order_a, order_b;         // uint32[n]: the order going into a pass and coming out of it
    DevBuf table, scan_tmp;          // uint32[256][blocks]; the scan's block totals
    DevBuf offsets;                  // uint32[n_clusters + 1]
    DevBuf out_rec;                  // the cluster records of a caller in host memory
};

namespace {

// the sort key of a label: a kept label is its own key; -1 and every label outside [-1, n_clusters) carry n_clusters (left out:
// no table is ever indexed by the label itself); *bad is set for the latter
__device__ __forceinline__ unsigned int seg_key(int32_t label, int32_t n_clusters, bool* bad) {
    if (label < -1 || label >= n_clusters) { *bad = true; return (unsigned int)n_clusters; }
    return label < 0 ? (unsigned int)n_clusters : (unsigned int)label;
}

// the lanes of this wave that are valid and carry the same digit as the calling lane: one ballot per bit of the digit
__device__ __forceinline__ unsigned long long digit_peers(bool valid, unsigned int digit) {
    unsigned long long peers = __ballot(valid);
    for (int b = 0; b < 8; ++b) {
        const bool bit = (digit >> b) & 1u;
        const unsigned long long with = __ballot(valid && bit);
        peers &= bit ? with : ~with;
    }
    return peers;
}

// workgroup b counts the digits of entries [b * chunk, min(n, (b + 1) * chunk)) of the current order (order_in == nullptr: the
// identity) -> table[digit * gridDim.x + b].  With a handful of clusters nearly every lane of a wave carries the same digit: the
// first lane of every peer group adds the group's size, one LDS atomic per group instead of one per entry.
__global__ void __launch_bounds__(256)
k_seg_hist(const int32_t* __restrict__ labels, const unsigned int* __restrict__ order_in, unsigned int n, unsigned int chunk, int shift,
           int32_t n_clusters, unsigned int* __restrict__ table, unsigned int* __restrict__ bad_word) {
    __shared__ unsigned int hist[256];
    const unsigned int lane = threadIdx.x & 63u;
    hist[threadIdx.x] = 0u;
    __syncthreads();
    const size_t begin = (size_t)blockIdx.x * chunk;
    const size_t end = begin + chunk < (size_t)n ? begin + chunk : (size_t)n;
    bool bad = false;
    for (size_t tile = begin; tile < end; tile += 256) {  // (uniform over the wave: every lane takes part in the ballots)
        const size_t i = tile + threadIdx.x;
        const bool valid = i < end;
        unsigned int digit = 0u;
        if (valid) {
            const unsigned int p = order_in ? order_in[i] : (unsigned int)i;
            digit = (seg_key(labels[p], n_clusters, &bad) >> shift) & 255u;
        }
        const unsigned long long peers = digit_peers(valid, digit);
        if (valid && (peers & ((1ull << lane) - 1ull)) == 0ull) atomicAdd(&hist[digit], (unsigned int)__popcll(peers));
    }
    __syncthreads();
    table[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = hist[threadIdx.x];
    if (__syncthreads_or(bad ? 1 : 0) && threadIdx.x == 0) atomicOr(bad_word, 1u);
}

// the same chunks again: entry i goes to (the scanned table's slot of its digit in this workgroup) + (entries of the chunk in
// front of it with the same digit).  Every slot has one writer and the ranks follow the entries' order: a stable pass.
__global__ void __launch_bounds__(256)
k_seg_scatter(const int32_t* __restrict__ labels, const unsigned int* __restrict__ order_in, unsigned int n, unsigned int chunk, int shift,
              int32_t n_clusters, const unsigned int* __restrict__ table, unsigned int* __restrict__ order_out) {
    __shared__ unsigned int base[256];
    __shared__ unsigned int wave_count[4][256];
    const unsigned int lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    base[threadIdx.x] = table[(size_t)threadIdx.x * gridDim.x + blockIdx.x];
    for (int w = 0; w < 4; ++w) wave_count[w][threadIdx.x] = 0u;
    __syncthreads();
    const size_t begin = (size_t)blockIdx.x * chunk;
    const size_t end = begin + chunk < (size_t)n ? begin + chunk : (size_t)n;
    for (size_t tile = begin; tile < end; tile += 256) {  // (uniform over the workgroup: the barriers below are met by all)
        const size_t i = tile + threadIdx.x;
        const bool valid = i < end;
        unsigned int p = 0u, digit = 0u;
        if (valid) {
            bool bad = false;
            p = order_in ? order_in[i] : (unsigned int)i;
            digit = (seg_key(labels[p], n_clusters, &bad) >> shift) & 255u;
        }
        const unsigned long long peers = digit_peers(valid, digit);
        const unsigned int rank = (unsigned int)__popcll(peers & ((1ull << lane) - 1ull));
        if (valid && rank == 0u) wave_count[wave][digit] = (unsigned int)__popcll(peers);
        __syncthreads();
        if (valid) {
            unsigned int slot = base[digit] + rank;
            for (unsigned int w = 0; w < wave; ++w) slot += wave_count[w][digit];
            order_out[slot] = p;  // (slot < n: the table was counted from the same keys)
        }
        __syncthreads();
        base[threadIdx.x] += wave_count[0][threadIdx.x] + wave_count[1][threadIdx.x] + wave_count[2][threadIdx.x] + wave_count[3][threadIdx.x];
        for (int w = 0; w < 4; ++w) wave_count[w][threadIdx.x] = 0u;
        __syncthreads();
    }
}

// offsets[c] = the first position of a key >= c in the sorted order, c = 0 .. n_clusters: the entry at position j that starts a
// new key writes every offset between its predecessor's key and its own (clusters without a point), the last entry those behind it
__global__ void __launch_bounds__(256)
k_seg_offsets(const int32_t* __restrict__ labels, const unsigned int* __restrict__ order, unsigned int n, int32_t n_clusters,
              unsigned int* __restrict__ offsets) {
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (size_t)gridDim.x * blockDim.x) {
        bool bad = false;
        const unsigned int key = seg_key(labels[order[j]], n_clusters, &bad);
        const unsigned int before = j ? seg_key(labels[order[j - 1]], n_clusters, &bad) + 1u : 0u;
        for (unsigned int c = before; c <= key; ++c) offsets[c] = (unsigned int)j;
        if (j + 1 == n)
            for (unsigned int c = key + 1u; c <= (unsigned int)n_clusters; ++c) offsets[c] = n;
    }
}

// out record j = the first `words` pieces of input record order[j]; W = uint4: 16 bytes at a time (both bases, both strides and
// the record length are multiples of 16)
template <class W>
__global__ void __launch_bounds__(256)
k_seg_records(const char* __restrict__ in, size_t stride, const unsigned int* __restrict__ order, size_t m, unsigned int words,
              char* __restrict__ out, size_t out_stride) {
    const size_t total = m * words;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t j = t / words;
        const size_t w = t - j * words;
        *reinterpret_cast<W*>(out + j * out_stride + w * sizeof(W)) =
            *reinterpret_cast<const W*>(in + (size_t)order[j] * stride + w * sizeof(W));
    }
}

inline int g1(size_t n) {
    size_t b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace

// ---- what the other segmentation calls build on (pcc_internal.hpp: ground.hip) ------------------------------------------------

// labels[n] on the device, n > 0, n_clusters > 0 -> *order (uint32[n]: the kept points cluster by cluster, ascending inside a
// cluster, then the points left out) and *offsets (uint32[n_clusters + 1]), both in SegmentScratch; the bad-label flag is left in
// DevWords::op[0].  Everything enqueued, nothing waited for.
int extract_order(pcc_index* ix, const int32_t* labels, size_t n, int32_t n_clusters, const unsigned int** order_out,
                  const unsigned int** offsets_out) {
    hipStream_t s = ix->stream;
    SegmentScratch* sg = scratch<SegmentScratch>(ix);
    // contiguous chunks of whole tiles, at most 4096 workgroups
    size_t blocks = std::min<size_t>((n + 2047) / 2048, 4096);
    const size_t chunk = ((n + blocks - 1) / blocks + 255) / 256 * 256;
    blocks = (n + chunk - 1) / chunk;
    int passes = 1;
    while (passes < 4 && ((unsigned int)n_clusters >> (8 * passes)) != 0u) ++passes;  // the largest key is n_clusters itself
    const size_t table_n = 256 * blocks;
    PCC_TRY(sg->order_a.reserve(n * sizeof(unsigned int)));
    if (passes > 1) PCC_TRY(sg->order_b.reserve(n * sizeof(unsigned int)));
    PCC_TRY(sg->table.reserve(table_n * sizeof(unsigned int)));
    if (offsets_out) PCC_TRY(sg->offsets.reserve(((size_t)n_clusters + 1) * sizeof(unsigned int)));
    unsigned int* bad_word = ix->words()->op;
    PCC_HIP(hipMemsetAsync(bad_word, 0, sizeof(unsigned int), s));
    unsigned int* table = sg->table.as<unsigned int>();
    // the last pass writes order_a
    unsigned int* bufs[2] = {sg->order_a.as<unsigned int>(), sg->order_b.as<unsigned int>()};
    const unsigned int* in = nullptr;
    for (int p = 0; p < passes; ++p) {
        unsigned int* out = bufs[(passes - 1 - p) & 1];
        hipLaunchKernelGGL(k_seg_hist, dim3((unsigned int)blocks), dim3(256), 0, s, labels, in, (unsigned int)n, (unsigned int)chunk, 8 * p,
                           n_clusters, table, bad_word);
        PCC_HIP(hipGetLastError());
        PCC_TRY(launch_exclusive_scan(ix, s, table, table_n, sg->scan_tmp));
        hipLaunchKernelGGL(k_seg_scatter, dim3((unsigned int)blocks), dim3(256), 0, s, labels, in, (unsigned int)n, (unsigned int)chunk, 8 * p,
                           n_clusters, table, out);
        PCC_HIP(hipGetLastError());
        in = out;
    }
    *order_out = in;
    if (!offsets_out) return PCC_OK;  // (ground.hip: a lattice's cells are mostly empty, and it looks their starts up itself)
    hipLaunchKernelGGL(k_seg_offsets, dim3(g1(n)), dim3(256), 0, s, labels, in, (unsigned int)n, n_clusters, sg->offsets.as<unsigned int>());
    PCC_HIP(hipGetLastError());
    *offsets_out = sg->offsets.as<unsigned int>();
    return PCC_OK;
}

// the offsets and the bad-label flag on their way to the host (pinned): the caller waits, then reads them with offsets_arrived()
int offsets_to_host(pcc_index* ix, const unsigned int* d_offsets, int32_t n_clusters) {
    PCC_TRY(ix->host_a.reserve(((size_t)n_clusters + 1) * sizeof(unsigned int)));
    PCC_HIP(hipMemcpyAsync(ix->host_a.p, d_offsets, ((size_t)n_clusters + 1) * sizeof(unsigned int), hipMemcpyDeviceToHost, ix->stream));
    PCC_HIP(hipMemcpyAsync(ix->pinned()->readback, ix->words()->op, sizeof(unsigned int), hipMemcpyDeviceToHost, ix->stream));
    return PCC_OK;
}
int offsets_arrived(pcc_index* ix, int32_t n_clusters, size_t* out_offsets) {
    if (ix->pinned()->readback[0]) { set_error("a label outside [-1, %d)", n_clusters); return PCC_ERR_INVALID; }
    const unsigned int* h = ix->host_a.as<unsigned int>();
    for (size_t c = 0; c <= (size_t)n_clusters; ++c) out_offsets[c] = h[c];
    return PCC_OK;
}

int launch_records(hipStream_t s, const void* in, size_t stride, const unsigned int* order, size_t m, size_t record_bytes, void* out,
                   size_t out_stride) {
    if (m == 0) return PCC_OK;
    const bool vec = record_bytes % 16 == 0 && stride % 16 == 0 && out_stride % 16 == 0 && reinterpret_cast<uintptr_t>(in) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const unsigned int words = (unsigned int)(record_bytes / (vec ? 16 : 4));
    auto kernel = vec ? k_seg_records<uint4> : k_seg_records<unsigned int>;
    hipLaunchKernelGGL(kernel, dim3(g1(m * words)), dim3(256), 0, s, static_cast<const char*>(in), stride, order, m, words,
                       static_cast<char*>(out), out_stride);
    PCC_HIP(hipGetLastError());
    return PCC_OK;
}

// a result in a buffer of the library's into the caller's array in either space (host: through deliver; the caller waits)
int give(pcc_index* ix, int mem, void* user, const void* dev, size_t bytes) {
    if (!user || bytes == 0) return PCC_OK;
    if (mem == PCC_MEM_HOST) return deliver(ix, dev, user, bytes);
    PCC_HIP(hipMemcpyAsync(user, dev, bytes, hipMemcpyDeviceToDevice, ix->stream));
    return PCC_OK;
}

}  // namespace pcc

using namespace pcc;
extern "C" {
int pcc_extract_clusters(pcc_index* ix, const void* records, size_t n, size_t stride, size_t record_bytes, const int32_t* labels,
                         int32_t n_clusters, int mem, void* out_records, size_t out_stride, int32_t* out_index, size_t* out_offsets) {
    PCC_TRY(check_mem(mem));
    if (n >= (1ull << 31)) { set_error("more than 2^31 points"); return PCC_ERR_UNSUPPORTED; }
    if (n_clusters < 0) { set_error("n_clusters %d is negative", n_clusters); return PCC_ERR_INVALID; }
    if (n && !labels) { set_error("null labels"); return PCC_ERR_INVALID; }
    if (!out_offsets) { set_error("null output"); return PCC_ERR_INVALID; }
    if (out_records) {
        PCC_TRY(check_points(records, n, stride, mem));
        if (record_bytes < 12 || record_bytes % 4 || record_bytes > stride || record_bytes > out_stride || out_stride % 4) {
            set_error("record_bytes %zu must be a multiple of 4, >= 12 and at most both strides (%zu, %zu, the output's a multiple of 4)",
                      record_bytes, stride, out_stride);
            return PCC_ERR_INVALID;
        }
    }
    PCC_ENTER(ix);
    for (size_t c = 0; c <= (size_t)n_clusters; ++c) out_offsets[c] = 0;
    if (n == 0 || n_clusters == 0) { PCC_NOTHING_ENQUEUED(ix); return PCC_OK; }
    hipStream_t s = ix->stream;
    ev_next(ix);
    ev_mark(ix, EV_CALL0);
    const int32_t* d_labels = nullptr;
    PCC_TRY(stage_in(ix, labels, n, mem, scratch<SegmentScratch>(ix)->lab_in, &d_labels));
    const unsigned int *order = nullptr, *d_offsets = nullptr;
    PCC_TRY(extract_order(ix, d_labels, n, n_clusters, &order, &d_offsets));
    ev_mark(ix, EV_CALL1);
    PCC_TRY(offsets_to_host(ix, d_offsets, n_clusters));
    if (mem == PCC_MEM_DEVICE) {
        PCC_HIP(hipStreamSynchronize(s));  // the call's one wait
        PCC_TRY(offsets_arrived(ix, n_clusters, out_offsets));
        const size_t m = out_offsets[n_clusters];
        PCC_TRY(give(ix, mem, out_index, order, m * sizeof(int32_t)));
        if (out_records) PCC_TRY(launch_records(s, records, stride, order, m, record_bytes, out_records, out_stride));
        return PCC_OK;
    }
    // host memory: the index list comes down whole (n entries: the points left out lie behind the clusters') beside the offsets,
    // one wait; the records are the caller's own, copied on the host in the order of the list
    std::vector<int32_t> own_index;
    int32_t* index = out_index;
    if (out_records && !out_index) {
        own_index.resize(n);
        index = own_index.data();
    }
    PCC_TRY(deliver(ix, order, index, n * sizeof(int32_t)));
    PCC_HIP(hipStreamSynchronize(s));
    PCC_TRY(offsets_arrived(ix, n_clusters, out_offsets));
    const size_t m = out_offsets[n_clusters];
    if (out_records)
        for (size_t j = 0; j < m; ++j)
            std::memcpy(static_cast<char*>(out_records) + j * out_stride, static_cast<const char*>(records) + (size_t)index[j] * stride,
                        record_bytes);
    return PCC_OK;
}

int pcc_region_growing_segmentation(pcc_index* ix, const void* pts, size_t n, size_t stride, int mem, float leaf, int has_rgb, int normal_k,
                                    int k, float smoothness, float curvature_threshold, uint32_t min_size, uint32_t max_size,
                                    void* out_points, size_t out_stride, size_t* n_filtered, float* out_normals, int32_t* out_labels,
                                    size_t max_clusters, int32_t* n_clusters, size_t* out_offsets, void* out_cluster_points,
                                    int32_t* out_cluster_index) {
    // what pcc_voxel_grid refuses, with its messages
    PCC_TRY(check_points(pts, n, stride, mem));
    if (!out_points || !n_filtered || !n_clusters || !out_offsets) { set_error("null output"); return PCC_ERR_INVALID; }
    if (out_stride < 12 || out_stride % 4) { set_error("bad output stride"); return PCC_ERR_INVALID; }
    if (has_rgb && (stride < 20 || out_stride < 20)) { set_error("rgb needs a stride of at least 20 bytes"); return PCC_ERR_INVALID; }
    if (!(leaf > 0.f)) { set_error("leaf size must be positive"); return PCC_ERR_INVALID; }
    if ((out_cluster_points || out_cluster_index) && max_clusters == 0) {
        set_error("cluster outputs given without room: max_clusters is 0");
        return PCC_ERR_INVALID;
    }
    if (!std::isfinite(smoothness) || !std::isfinite(curvature_threshold)) {
        set_error("smoothness and curvature thresholds must be finite");
        return PCC_ERR_INVALID;
    }
    if (normal_k < 1 || normal_k > PCC_KNN_MAX_K) { set_error("k=%d outside [1, %d]", normal_k, PCC_KNN_MAX_K); return PCC_ERR_UNSUPPORTED; }
    if (k < 1 || k > PCC_KNN_MAX_K) { set_error("k=%d outside [1, %d]", k, PCC_KNN_MAX_K); return PCC_ERR_UNSUPPORTED; }
    PCC_ENTER(ix);
    *n_filtered = 0;
    *n_clusters = 0;
    out_offsets[0] = 0;
    PCC_TRY(sync_info(ix));  // (a pending mirror of the handle's own grid would overwrite stats[2] later)
    ix->stats[0] = ix->stats[1] = ix->stats[2] = ix->stats[7] = 0;
    ix->stats_pending = false;
    if (n == 0) { PCC_NOTHING_ENQUEUED(ix); return PCC_OK; }
    hipStream_t s = ix->stream;
    ev_next(ix);
    ev_mark(ix, EV_CALL0);
    SegmentScratch* sg = scratch<SegmentScratch>(ix);

    // 1. the voxel grid, on `ix`: the raw cloud on the device (a host cloud in q_raw, which voxel_grid leaves alone for a device
    // cloud), the centroids into a zeroed buffer of this call's own
    const void* src = pts;
    if (mem == PCC_MEM_HOST) {
        PCC_TRY(ix->q_raw.reserve(n * stride));
        // (a strided host view may end with its last row: up to the last byte read, as voxel_grid copies it)
        PCC_HIP(hipMemcpyAsync(ix->q_raw.p, pts, (n - 1) * stride + (has_rgb ? 20 : 12), hipMemcpyHostToDevice, s));
        src = ix->q_raw.p;
    }
    PCC_TRY(sg->cloud.reserve(n * out_stride));
    PCC_HIP(hipMemsetAsync(sg->cloud.p, 0, n * out_stride, s));
    size_t nv = 0;
    PCC_TRY(voxel_grid(ix, src, n, stride, PCC_MEM_DEVICE, leaf, has_rgb, sg->cloud.p, out_stride, &nv));
    *n_filtered = nv;
    ix->stats[0] = nv;
    if (nv == 0) return PCC_OK;  // (no finite point; voxel_grid has waited: nothing is in flight)

    // 2. the filtered cloud indexed on the work handle; one search with max(normal_k, k) neighbours serves both stages
    WorkLease lease;
    PCC_TRY(lease.take(ix, sg->work, true));
    pcc_index* w = lease.w;
    w->opt.knn_cache_k = std::max(normal_k, k);
    PCC_TRY(set_input(w, sg->cloud.p, nv, out_stride, PCC_MEM_DEVICE));
    entered(w);
    PCC_TRY(ensure_grid(w));

    // 3. normals from the first normal_k entries of the rows, 4. the growing over the first k
    const float origin[3] = {0.f, 0.f, 0.f};
    const unsigned long long* keys = nullptr;
    PCC_TRY(sg->normals.reserve(nv * sizeof(float4)));
    PCC_TRY(sg->labels.reserve(nv * sizeof(int32_t)));
    PCC_TRY(self_knn_keys(w, normal_k, &keys));
    PCC_TRY(launch_normals(s, keys, w->refs.as<float4>(), w->cell_refs.as<float4>(), w->d_grid.as<GridDev>(), nv, normal_k, origin,
                           sg->normals.as<float4>()));
    PCC_TRY(self_knn_keys(w, k, &keys));
    int32_t ncl = 0;
    unsigned int sweeps = 0;
    PCC_TRY(grid_region_growing(w, keys, sg->normals.as<float4>(), k, smoothness, curvature_threshold, min_size, max_size,
                                sg->labels.as<int32_t>(), &ncl, &sweeps));
    *n_clusters = ncl;
    ix->stats[1] = (uint64_t)ncl;
    ix->stats[7] = sweeps;

    // 5. labels -> cluster clouds, on `ix` again
    const bool fits = (size_t)ncl <= max_clusters;
    const unsigned int *order = nullptr, *d_offsets = nullptr;
    size_t m = 0;
    if (fits && ncl > 0) {
        PCC_TRY(extract_order(ix, sg->labels.as<int32_t>(), nv, ncl, &order, &d_offsets));
        PCC_TRY(offsets_to_host(ix, d_offsets, ncl));
        PCC_HIP(hipStreamSynchronize(s));
        PCC_TRY(offsets_arrived(ix, ncl, out_offsets));
        m = out_offsets[ncl];
        ix->stats[2] = m;
    }
    ev_mark(ix, EV_CALL1);
    // the caller's arrays: each once (host memory: through deliver, then the call's last wait)
    PCC_TRY(give(ix, mem, out_points, sg->cloud.p, nv * out_stride));
    PCC_TRY(give(ix, mem, out_normals, sg->normals.p, nv * sizeof(float4)));
    PCC_TRY(give(ix, mem, out_labels, sg->labels.p, nv * sizeof(int32_t)));
    if (m) {
        PCC_TRY(give(ix, mem, out_cluster_index, order, m * sizeof(int32_t)));
        if (out_cluster_points) {
            void* dst = out_cluster_points;
            if (mem == PCC_MEM_HOST) {
                PCC_TRY(sg->out_rec.reserve(m * out_stride));
                dst = sg->out_rec.p;
            }
            PCC_TRY(launch_records(s, sg->cloud.p, out_stride, order, m, out_stride, dst, out_stride));
            if (mem == PCC_MEM_HOST) PCC_TRY(give(ix, mem, out_cluster_points, dst, m * out_stride));
        }
    }
    if (mem == PCC_MEM_HOST) PCC_HIP(hipStreamSynchronize(s));
    if (!fits) {
        set_error("%d clusters, more than max_clusters = %zu", ncl, max_clusters);
        return PCC_ERR_OVERFLOW;
    }
    return PCC_OK;
}
int pcc_euclidean_cluster_segmentation(pcc_index* ix, const void* pts, size_t n, size_t stride, int mem, float leaf, int has_rgb,
                                       double stop_fraction, int max_iterations, double distance_threshold, double probability,
                                       int optimize, size_t max_planes, float* out_coefficients, uint32_t* out_plane_sizes,
                                       int* out_iterations, size_t* n_planes, int* ended_without_model, double tolerance,
                                       uint32_t min_size, uint32_t max_size, void* out_points, size_t out_stride, size_t* n_filtered,
                                       size_t* n_remaining, int32_t* out_labels, size_t max_clusters, int32_t* n_clusters,
                                       size_t* out_offsets, void* out_cluster_points, int32_t* out_cluster_index) {
    // what pcc_voxel_grid refuses, with its messages
    PCC_TRY(check_points(pts, n, stride, mem));
    if (!out_points) { set_error("null output"); return PCC_ERR_INVALID; }
    if (out_stride < 12 || out_stride % 4) { set_error("bad output stride"); return PCC_ERR_INVALID; }
    if (has_rgb && (stride < 20 || out_stride < 20)) { set_error("rgb needs a stride of at least 20 bytes"); return PCC_ERR_INVALID; }
    if (!(leaf > 0.f)) { set_error("leaf size must be positive"); return PCC_ERR_INVALID; }
    // what pcc_plane_removal refuses about its own parameters and tables (its records are whole voxel-grid records; n_remaining
    // has its turn below: n_planes stands in for it here)
    PCC_TRY(check_plane_loop(stop_fraction, max_iterations, distance_threshold, probability, max_planes, out_coefficients, out_plane_sizes,
                             n_planes, n_planes));
    if (!(tolerance >= 0)) { set_error("bad tolerance"); return PCC_ERR_INVALID; }
    if (!n_filtered || !n_remaining || !n_clusters || !out_offsets) { set_error("null output"); return PCC_ERR_INVALID; }
    if ((out_cluster_points || out_cluster_index) && max_clusters == 0) {
        set_error("cluster outputs given without room: max_clusters is 0");
        return PCC_ERR_INVALID;
    }
    PCC_ENTER(ix);
    *n_filtered = 0;
    *n_remaining = 0;
    *n_planes = 0;
    *n_clusters = 0;
    if (ended_without_model) *ended_without_model = 0;
    out_offsets[0] = 0;
    PCC_TRY(sync_info(ix));  // (a pending mirror of the handle's own grid would overwrite stats[2] later)
    ix->stats[0] = ix->stats[1] = ix->stats[2] = ix->stats[3] = ix->stats[4] = 0;
    ix->stats_pending = false;
    if (n == 0) { PCC_NOTHING_ENQUEUED(ix); return PCC_OK; }
    hipStream_t s = ix->stream;
    ev_next(ix);
    ev_mark(ix, EV_CALL0);
    SegmentScratch* sg = scratch<SegmentScratch>(ix);

    // 1. the voxel grid, on `ix`, into a zeroed buffer of this call's own (as pcc_region_growing_segmentation)
    const void* src = pts;
    if (mem == PCC_MEM_HOST) {
        PCC_TRY(ix->q_raw.reserve(n * stride));
        PCC_HIP(hipMemcpyAsync(ix->q_raw.p, pts, (n - 1) * stride + (has_rgb ? 20 : 12), hipMemcpyHostToDevice, s));
        src = ix->q_raw.p;
    }
    PCC_TRY(sg->cloud.reserve(n * out_stride));
    PCC_HIP(hipMemsetAsync(sg->cloud.p, 0, n * out_stride, s));
    size_t nv = 0;
    PCC_TRY(voxel_grid(ix, src, n, stride, PCC_MEM_DEVICE, leaf, has_rgb, sg->cloud.p, out_stride, &nv));
    *n_filtered = nv;
    ix->stats[0] = nv;
    if (nv == 0) return PCC_OK;  // (no finite point; voxel_grid has waited: nothing is in flight)

    // 2. the plane loop over the filtered cloud where it lies.  voxel_grid has waited for its last kernel, so vox_a/b/c are
    // free; the loop packs sg->cloud into q_packed (q_raw, the raw cloud of a host caller, is not needed again) and reads single
    // points by gathering them on the device -- turn 0 included: the filtered cloud has no host copy
    PlaneLoop L;
    L.pts = sg->cloud.p; L.n = nv; L.stride = out_stride; L.mem = PCC_MEM_DEVICE;
    L.stop_fraction = stop_fraction; L.max_iterations = max_iterations; L.threshold = distance_threshold; L.probability = probability;
    L.optimize = optimize; L.max_planes = max_planes;
    L.out_coefficients = out_coefficients; L.out_plane_sizes = out_plane_sizes; L.out_iterations = out_iterations;
    L.ended_without_model = ended_without_model;
    const int plane_status = plane_loop(ix, L);
    if (plane_status != PCC_OK && plane_status != PCC_ERR_OVERFLOW) return plane_status;
    const size_t nr = L.remaining;
    *n_planes = L.planes;
    *n_remaining = nr;
    ix->stats[3] = L.planes;
    ix->stats[4] = L.host_copies;
    if (plane_status != PCC_OK) {
        PCC_HIP(hipStreamSynchronize(s));  // (the arrays in space `mem` are unspecified, but nothing is in flight at the return)
        return plane_status;
    }
    if (nr == 0) {  // nothing remains: no cluster, nothing to hand over
        ev_mark(ix, EV_CALL1);
        return PCC_OK;
    }
    // the records that remain: into the caller's array in device memory, else into a buffer of this call's
    void* rem = out_points;
    if (mem == PCC_MEM_HOST) {
        PCC_TRY(sg->remain.reserve(nr * out_stride));
        rem = sg->remain.p;
    }
    PCC_TRY(launch_plane_records(s, sg->cloud.p, out_stride, L.remaining_index, nr, out_stride, rem, out_stride));

    // 3. the remaining cloud indexed on the work handle, 4. clustered there, the labels in a buffer of this call's
    WorkLease lease;
    PCC_TRY(lease.take(ix, sg->work, true));
    pcc_index* w = lease.w;
    PCC_TRY(set_input(w, rem, nr, out_stride, PCC_MEM_DEVICE));
    entered(w);
    PCC_TRY(ensure_grid(w));
    PCC_TRY(sg->labels.reserve(nr * sizeof(int32_t)));
    const float tol_f = (float)tolerance;  // (pcc_euclidean_clusters: r2 = float(double(float(tol))^2))
    int32_t ncl = 0;
    PCC_TRY(grid_clusters(w, tol_f, radius2((double)tol_f), min_size, max_size, sg->labels.as<int32_t>(), &ncl, nullptr, 0, true));
    *n_clusters = ncl;
    ix->stats[1] = (uint64_t)ncl;

    // 5. labels -> cluster clouds, on `ix` again
    const bool fits = (size_t)ncl <= max_clusters;
    const unsigned int *order = nullptr, *d_offsets = nullptr;
    size_t m = 0;
    if (fits && ncl > 0) {
        PCC_TRY(extract_order(ix, sg->labels.as<int32_t>(), nr, ncl, &order, &d_offsets));
        PCC_TRY(offsets_to_host(ix, d_offsets, ncl));
        PCC_HIP(hipStreamSynchronize(s));
        PCC_TRY(offsets_arrived(ix, ncl, out_offsets));
        m = out_offsets[ncl];
        ix->stats[2] = m;
    }
    ev_mark(ix, EV_CALL1);
    // the caller's arrays: each once (host memory: through deliver, then the call's last wait)
    if (mem == PCC_MEM_HOST) PCC_TRY(give(ix, mem, out_points, rem, nr * out_stride));
    PCC_TRY(give(ix, mem, out_labels, sg->labels.p, nr * sizeof(int32_t)));
    if (m) {
        PCC_TRY(give(ix, mem, out_cluster_index, order, m * sizeof(int32_t)));
        if (out_cluster_points) {
            void* dst = out_cluster_points;
            if (mem == PCC_MEM_HOST) {
                PCC_TRY(sg->out_rec.reserve(m * out_stride));
                dst = sg->out_rec.p;
            }
            PCC_TRY(launch_records(s, rem, out_stride, order, m, out_stride, dst, out_stride));
            if (mem == PCC_MEM_HOST) PCC_TRY(give(ix, mem, out_cluster_points, dst, m * out_stride));
        }
    }
    if (mem == PCC_MEM_HOST) PCC_HIP(hipStreamSynchronize(s));
    if (!fits) {
        set_error("%d clusters, more than max_clusters = %zu", ncl, max_clusters);
        return PCC_ERR_OVERFLOW;
    }
    return PCC_OK;
}
}  // extern "C"
