// region_rgb.hip -- pcl::RegionGrowingRGB::extract as color_growing_segmentation configures it (reference
// src/segmentation.cpp:161-216; called twice per accepted match, src/comparator.cpp:1456-1495) on the GPU: pcc_region_growing_rgb.
//
// PCL grows the colour segments one after another: the unlabelled point of lowest INDEX seeds a segment, which spreads
// breadth first along the first `nr_neighbours` entries of the k-neighbour rows -- u claims a still unlabelled neighbour v
// when the squared colour distance of the two is within the point colour threshold -- and every claimed point spreads.
// As for the sister algorithm (region.hip) the outcome has an order-free description, with rank = point index:
//
//     segment(v) = the lowest-indexed point that reaches v along valid edges.
//
// (The lowest-indexed point m that reaches v can not have been claimed by an earlier seed s -- s would reach v through m and
// have a lower index -- so m is a seed when the index-order scan arrives at it; a point already labelled on a path m -> v
// would put v into that earlier segment too, so m's segment takes v.)  tests/test_rgb_device_cpu.py holds that statement
// against the oracle's queue on six scenes.
//
// The rows (self k-NN, K = min(nr_region_neighbours, n_valid), ascending (d2, index)) never leave the device:
//   prepare  : parent[i] = i, label[i] = i, the key that ends the growing prefix of every row (u is in the prefix of row(v)
//              iff its key is <= that, distances being bitwise symmetric), the colours unpacked into one word per point
//   link     : one wave per point, one lane per row entry: valid edges present in BOTH prefixes (the colour test is
//              symmetric) are merged with the lock-free union-find -- both ends reach each other
//   flatten  : parent[i] = root; a root is its component's lowest member (uf_device.hpp), i.e. its label to start with
//   sweep    : one-directional valid edges between different components push the lower label across; repeated until a
//              sweep changes nothing (points without such an edge are listed by the first sweep, later ones visit those)
//   ids      : seeds (label == own index) flagged, exclusive scan: dense segment ids in index order
//   stats    : points and the three channel sums per segment, integer atomics (exact, order-free, wrapping as PCL's
//              unsigned int), combined inside the wave first
//   pairs    : min over (s, t != s) of the row distance from a point of s to a point of t over ALL K entries: duplicates
//              dropped inside the wave, the rest combined in an open-addressing table keyed by (s << 32 | t) -- slots
//              claimed by 64-bit atomicCAS, distances by atomicMin on their bits (d2 >= 0: they order as unsigned) -- sized
//              from a counting pass; the occupied slots compacted into a list
//   host     : the per-segment records (16 bytes) and the pair list (12 bytes) -- never the rows -- go through
//              rgb_merge.hpp (the nearest segments per segment, PCL's merging, folding and size filter); the cluster of
//              every segment comes back
//   label    : labels[i] = cluster of i's segment, written on the device for either memory space
// No result bit depends on execution order: min and integer sums commute, and the host sorts the pair list before use.
#include <algorithm>
#include <cmath>
#include <vector>

#include "entry.hpp"
#include "grid_device.hpp"
#include "rgb_merge.hpp"
#include "rgb_stages.hpp"
#include "uf_device.hpp"

namespace pcc {

namespace {

constexpr unsigned long long PAIR_EMPTY = ~0ull;  // no key: a segment id is below 2^32 - 1
static_assert(sizeof(RgbSegment) == 16 && sizeof(RgbSegmentPair) == 12, "records as the device writes them");

// RegionGrowingRGB::validatePoint without normals: the squared colour distance (unsigned, exact) as a float against the
// squared point colour threshold; colours are (r << 16 | g << 8 | b)
__device__ __forceinline__ bool colour_edge(unsigned int a, unsigned int b, float p2p2) {
    const int dr = (int)((a >> 16) & 255u) - (int)((b >> 16) & 255u);
    const int dg = (int)((a >> 8) & 255u) - (int)((b >> 8) & 255u);
    const int db = (int)(a & 255u) - (int)(b & 255u);
    return !((float)(unsigned int)(dr * dr + dg * dg + db * db) > p2p2);
}

__device__ __forceinline__ unsigned int wave_sum(unsigned int x) {
    for (int m = 32; m >= 1; m >>= 1) x += (unsigned int)__shfl_xor((int)x, m, 64);
    return x;
}

// Which points the wave-per-point kernels take, and in which order (a template parameter of theirs).  ByCell: the first
// gd->n_valid entries of cell_refs name them -- one indexed cloud, in CELL order, so that a wave's gathers stay spatially compact.
// ByIndex: every index 0 .. n itself -- a concatenation of clouds (region_rgb_batch.hip), which has no grid; the row of a
// non-finite point is empty there, so its wave finds nothing to do.
struct ByCell {
    const float4* __restrict__ cell_refs;
    const GridDev* __restrict__ gd;
    __device__ __forceinline__ unsigned int count() const { return gd->n_valid; }
    __device__ __forceinline__ unsigned int point(unsigned int w) const { return (unsigned int)__float_as_int(cell_refs[w].w); }
};
struct ByIndex {
    unsigned int n;
    __device__ __forceinline__ unsigned int count() const { return n; }
    __device__ __forceinline__ unsigned int point(unsigned int w) const { return w; }
};

// P = min(nr_neighbours, K): the length of the growing prefix of a row
__global__ void __launch_bounds__(256)
k_rgb_prepare(const unsigned long long* __restrict__ keys, const unsigned char* __restrict__ rgb, size_t rgb_stride, unsigned int n,
              int K, int P, unsigned int* __restrict__ parent, unsigned int* __restrict__ label,
              unsigned long long* __restrict__ kth, unsigned int* __restrict__ col) {
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        parent[i] = i;
        label[i] = i;
        kth[i] = keys[(size_t)i * K + (P - 1)];
        col[i] = *reinterpret_cast<const uint32_t*>(rgb + (size_t)i * rgb_stride) & 0x00ffffffu;
    }
}

// wave w owns the w-th point of the order (ByCell: the w-th valid point in CELL order): its row is read coalesced, its
// neighbours' colours and prefix keys are gathers into a spatially compact set
template <class Order>
__global__ void __launch_bounds__(256)
k_rgb_link(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ col,
           const unsigned long long* __restrict__ kth, const Order order, int K, int P, float p2p2, unsigned int* __restrict__ parent) {
    const unsigned int w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const unsigned int lane = threadIdx.x & 63;
    if (w >= order.count()) return;
    const unsigned int u = order.point(w);
    const unsigned int cu = col[u];
    const unsigned long long* row = keys + (size_t)u * K;
    for (int base = 0; base < P; base += 64) {
        const int j = base + (int)lane;
        const unsigned long long key = j < P ? row[j] : ~0ull;
        if (key_none(key)) continue;
        const unsigned int v = (unsigned int)key;
        if (v >= u) continue;  // every mutual pair is seen from both ends: the higher one links
        if (!colour_edge(cu, col[v], p2p2)) continue;
        const unsigned long long mine = (key & 0xffffffff00000000ull) | u;  // u's key in v's ordering
        if (mine <= kth[v]) uf_union(parent, u, v);
    }
}

__global__ void __launch_bounds__(256)
k_rgb_flatten(unsigned int n, unsigned int* __restrict__ parent) {
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const unsigned int r = uf_find(parent, i);
        atomicMin(&parent[i], r);
    }
}

// parent[] is flat here.  FIRST: every point is visited, and the points with an edge into another component are LISTED;
// the later sweeps are launched over that list alone.
template <bool FIRST, class Order>
__global__ void __launch_bounds__(256)
k_rgb_sweep(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ col, const Order order, int K, int P, float p2p2,
            const unsigned int* __restrict__ parent, unsigned int* __restrict__ label, unsigned int* __restrict__ changed,
            unsigned int* __restrict__ cross_list, unsigned int* __restrict__ cross_count, unsigned int list_n) {
    unsigned int w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const unsigned int lane = threadIdx.x & 63;
    if (FIRST) {
        if (w >= order.count()) return;
    } else {
        if (w >= list_n) return;
        w = cross_list[w];
    }
    const unsigned int u = order.point(w);
    const unsigned int cu = col[u];
    const unsigned int ru = parent[u];
    const unsigned int lu = __hip_atomic_load(&label[ru], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long* row = keys + (size_t)u * K;
    bool cross = false, moved = false;
    for (int base = 0; base < P; base += 64) {
        const int j = base + (int)lane;
        const unsigned long long key = j < P ? row[j] : ~0ull;
        if (key_none(key)) continue;
        const unsigned int v = (unsigned int)key;
        const unsigned int rv = parent[v];
        if (rv == ru) continue;
        if (!colour_edge(cu, col[v], p2p2)) continue;
        cross = true;
        if (atomicMin(&label[rv], lu) > lu) moved = true;
    }
    if (FIRST) {
        const bool any_cross = __ballot(cross) != 0ull;
        if (lane == 0 && any_cross) cross_list[atomicAdd(cross_count, 1u)] = w;
    }
    if (__ballot(moved) != 0ull && lane == 0) atomicOr(changed, 1u);
}

// flags[i] = 1 for the seeds: the finite points that are their own label (flags[n] = 0 was set in front)
__global__ void __launch_bounds__(256)
k_rgb_seed_flags(const float4* __restrict__ refs, const unsigned int* __restrict__ parent, const unsigned int* __restrict__ label,
                 unsigned int n, unsigned int* __restrict__ flags) {
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        flags[i] = (__float_as_int(refs[i].w) >= 0 && label[parent[i]] == i) ? 1u : 0u;
}

// pos: the exclusive scan of the flags = the dense id of every seed; seg[i] = id of i's seed, -1 for non-finite points
__global__ void __launch_bounds__(256)
k_rgb_segment_ids(const float4* __restrict__ refs, const unsigned int* __restrict__ parent, const unsigned int* __restrict__ label,
                  const unsigned int* __restrict__ pos, unsigned int n, int* __restrict__ seg) {
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        seg[i] = __float_as_int(refs[i].w) >= 0 ? (int)pos[label[parent[i]]] : -1;
}

// one lane per point of the order (neighbouring lanes mostly share a segment): the lanes of a wave that share a
// segment add up first, one lane of them issues the four atomics
template <class Order>
__global__ void __launch_bounds__(256)
k_rgb_stats(const Order order, const int* __restrict__ seg, const unsigned int* __restrict__ col, unsigned int ns,
            RgbSegment* __restrict__ stats) {
    const unsigned int n_valid = order.count();
    const unsigned int lane = threadIdx.x & 63;
    // (the trip count is the wave's: every lane takes part in the exchanges)
    for (unsigned int t0 = (blockIdx.x * blockDim.x + threadIdx.x) & ~63u; t0 < n_valid; t0 += gridDim.x * blockDim.x) {
        const unsigned int t = t0 + lane;
        bool pending = t < n_valid;
        int s = -1;
        unsigned int c = 0;
        if (pending) {
            const unsigned int i = order.point(t);
            s = seg[i];
            c = col[i];
        }
        for (;;) {
            const unsigned long long open = __ballot(pending);
            if (open == 0ull) break;
            const int leader = __ffsll((long long)open) - 1;
            const int s0 = __shfl(s, leader, 64);
            const bool mine = pending && s == s0;
            const unsigned int cnt = wave_sum(mine ? 1u : 0u);
            const unsigned int sr = wave_sum(mine ? (c >> 16) & 255u : 0u);
            const unsigned int sg = wave_sum(mine ? (c >> 8) & 255u : 0u);
            const unsigned int sb = wave_sum(mine ? c & 255u : 0u);
            if ((int)lane == leader && (unsigned int)s0 < ns) {
                RgbSegment* o = stats + s0;
                atomicAdd(&o->size, cnt);
                atomicAdd(&o->sum_r, sr);
                atomicAdd(&o->sum_g, sg);
                atomicAdd(&o->sum_b, sb);
            }
            pending = pending && !mine;
        }
    }
}

__device__ __forceinline__ size_t pair_slot(unsigned long long key, int log2_size) {
    return (size_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - log2_size));
}

// One wave per point of the order, one lane per row entry, all K of them.  An entry is FOREIGN when its point lies in
// another segment than the row's.  Of the foreign entries of a 64-entry chunk that name the same segment only the first
// counts -- rows ascend, it holds their minimum.  INSERT = false: those are counted (an upper bound of the distinct pairs);
// INSERT = true: they go into the table.
template <bool INSERT, class Order>
__global__ void __launch_bounds__(256)
k_rgb_pairs(const unsigned long long* __restrict__ keys, const int* __restrict__ seg, const Order order, int K,
            unsigned int* __restrict__ count, unsigned long long* __restrict__ tkeys, unsigned int* __restrict__ tdist, int log2_size,
            unsigned int* __restrict__ overflow) {
    const unsigned int w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const unsigned int lane = threadIdx.x & 63;
    if (w >= order.count()) return;
    const unsigned int u = order.point(w);
    const int su = seg[u];
    const unsigned long long* row = keys + (size_t)u * K;
    unsigned int firsts = 0;
    for (int base = 0; base < K; base += 64) {  // (K is the wave's: every lane takes part in the exchanges)
        const int j = base + (int)lane;
        const unsigned long long key = j < K ? row[j] : ~0ull;
        int t = su;
        if (!key_none(key)) t = seg[(unsigned int)key];
        bool pending = t != su;
        for (;;) {
            const unsigned long long open = __ballot(pending);
            if (open == 0ull) break;
            const int leader = __ffsll((long long)open) - 1;  // the lowest lane: the earliest entry of the row
            const int t0 = __shfl(t, leader, 64);
            if ((int)lane == leader) {
                if (INSERT) {
                    const unsigned long long pk = ((unsigned long long)(unsigned int)su << 32) | (unsigned int)t;
                    const unsigned int dbits = (unsigned int)(key >> 32);
                    const size_t mask = ((size_t)1 << log2_size) - 1;
                    size_t h = pair_slot(pk, log2_size);
                    bool placed = false;
                    for (size_t probe = 0; probe <= mask; ++probe) {
                        const unsigned long long cur = atomicCAS(&tkeys[h], PAIR_EMPTY, pk);
                        if (cur == PAIR_EMPTY || cur == pk) {
                            atomicMin(&tdist[h], dbits);
                            placed = true;
                            break;
                        }
                        h = (h + 1) & mask;
                    }
                    if (!placed) atomicOr(overflow, 1u);
                } else {
                    ++firsts;
                }
            }
            pending = pending && t != t0;
        }
    }
    if (!INSERT) {
        const unsigned int total = wave_sum(firsts);
        if (lane == 0 && total) atomicAdd(count, total);
    }
}

__global__ void __launch_bounds__(256)
k_rgb_compact_pairs(const unsigned long long* __restrict__ tkeys, const unsigned int* __restrict__ tdist, size_t size,
                    RgbSegmentPair* __restrict__ list, unsigned int* __restrict__ count, unsigned int cap) {
    for (size_t h = (size_t)blockIdx.x * blockDim.x + threadIdx.x; h < size; h += (size_t)gridDim.x * blockDim.x) {
        const unsigned long long pk = tkeys[h];
        if (pk == PAIR_EMPTY) continue;
        const unsigned int at = atomicAdd(count, 1u);
        if (at < cap) list[at] = RgbSegmentPair{(uint32_t)(pk >> 32), (uint32_t)pk, __uint_as_float(tdist[h])};
    }
}

__global__ void __launch_bounds__(256)
k_rgb_label(const int* __restrict__ seg, const int32_t* __restrict__ cluster_of_segment, unsigned int n, unsigned int ns,
            int32_t* __restrict__ labels) {
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int s = seg[i];
        labels[i] = (unsigned int)s < ns ? cluster_of_segment[s] : -1;
    }
}

// ids[c] = pos[bases[c]] for c <= n_clouds: the first segment id of every cloud of a concatenation (pos: the exclusive scan of
// the seed flags; bases[n_clouds] = n, so ids[n_clouds] = the number of segments)
__global__ void __launch_bounds__(256)
k_rgb_cloud_ids(const unsigned int* __restrict__ pos, const unsigned int* __restrict__ bases, unsigned int n_clouds,
                unsigned int* __restrict__ ids) {
    for (unsigned int c = blockIdx.x * blockDim.x + threadIdx.x; c <= n_clouds; c += gridDim.x * blockDim.x) ids[c] = pos[bases[c]];
}

inline int g1(size_t n) {
    size_t b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

// pairs that come down with their count, before the count is known (12 bytes each): a list beyond it costs one more wait
constexpr unsigned int RGB_PAIRS_FIRST_COPY = 1u << 18;

template <class Order>
int rgb_stages_in(pcc_index* ix, const RgbRun& run, const Order& order, const RgbHostHalf& host_half) {
    hipStream_t s = ix->stream;
    const unsigned int n = run.n;
    const unsigned long long* keys = run.keys;
    const int K = run.K;
    const int P = (int)std::min<unsigned int>(run.nr_neighbours, (unsigned int)K);
    const float p2p2 = run.point_color_threshold * run.point_color_threshold;
    PCC_TRY(ix->scratch_a.reserve((size_t)n * 4));        // label
    PCC_TRY(ix->scratch_c.reserve((size_t)n * 4));        // parent
    PCC_TRY(ix->scratch_d.reserve((size_t)n * 4));        // colours
    PCC_TRY(ix->scratch_e.reserve(((size_t)n + 1) * 4));  // seed flags -> their exclusive scan
    PCC_TRY(ix->scratch_f.reserve((size_t)n * 8));        // kth
    PCC_TRY(ix->scratch_g.reserve((size_t)n * 4));        // segment of every point
    PCC_TRY(ix->knn_fb.reserve(((size_t)n + 1) * sizeof(unsigned int)));  // (free here: the rows were searched before)
    auto* label = ix->scratch_a.as<unsigned int>();
    auto* parent = ix->scratch_c.as<unsigned int>();
    auto* col = ix->scratch_d.as<unsigned int>();
    auto* flags = ix->scratch_e.as<unsigned int>();
    auto* kth = ix->scratch_f.as<unsigned long long>();
    auto* seg = ix->scratch_g.as<int>();
    unsigned int* cross_list = ix->knn_fb.as<unsigned int>();
    unsigned int* d_words = ix->words()->op;  // growing: [0] changed, [1] -, [2] points with a cross edge; pairs: [0] foreign firsts, [1] pairs listed, [2] table overflow
    ev_mark(ix, EV_MAIN0);
    PCC_HIP(hipMemsetAsync(d_words, 0, sizeof(DevWords::op), s));
    hipLaunchKernelGGL(k_rgb_prepare, dim3(g1(n)), dim3(256), 0, s, keys, run.rgb, run.rgb_stride, n, K, P, parent, label, kth, col);
    const unsigned int wave_blocks = (n + 3) / 4;
    hipLaunchKernelGGL(k_rgb_link<Order>, dim3(wave_blocks), dim3(256), 0, s, keys, col, kth, order, K, P, p2p2, parent);
    hipLaunchKernelGGL(k_rgb_flatten, dim3(g1(n)), dim3(256), 0, s, n, parent);
    PCC_HIP(hipGetLastError());
    unsigned int n_cross = 0, sweeps = 0;
    for (unsigned int sweep = 0;; ++sweep) {
        // every sweep that goes on lowers a label, and a label is a point index: n sweeps settle any cloud
        if (sweep > n + 1) { set_error("colour region growing did not settle"); return PCC_ERR_DEVICE; }
        PCC_HIP(hipMemsetAsync(d_words, 0, 4, s));
        if (sweep == 0)
            hipLaunchKernelGGL((k_rgb_sweep<true, Order>), dim3(wave_blocks), dim3(256), 0, s, keys, col, order, K, P, p2p2, parent, label,
                               d_words, cross_list, d_words + 2, 0u);
        else
            hipLaunchKernelGGL((k_rgb_sweep<false, Order>), dim3((n_cross + 3) / 4), dim3(256), 0, s, keys, col, order, K, P, p2p2, parent,
                               label, d_words, cross_list, d_words + 2, n_cross);
        PCC_HIP(hipGetLastError());
        unsigned int w[3];  // changed, -, cross count
        PCC_TRY(read_back<3>(ix, d_words, w));
        ++sweeps;
        if (sweep == 0) n_cross = w[2];
        if (n_cross > n) { set_error("colour region growing: %u points with a cross edge among %u", n_cross, n); return PCC_ERR_DEVICE; }
        if (w[0] == 0 || n_cross == 0) break;
    }
    // dense segment ids in index order
    PCC_HIP(hipMemsetAsync(flags + n, 0, 4, s));
    hipLaunchKernelGGL(k_rgb_seed_flags, dim3(g1(n)), dim3(256), 0, s, run.refs, parent, label, n, flags);
    PCC_HIP(hipGetLastError());
    PCC_TRY(launch_exclusive_scan(ix, s, flags, (size_t)n + 1, ix->vox_c));
    hipLaunchKernelGGL(k_rgb_segment_ids, dim3(g1(n)), dim3(256), 0, s, run.refs, parent, label, flags, n, seg);
    PCC_HIP(hipGetLastError());
    unsigned int ns = 0;
    if (run.d_bases) {
        // a concatenation: ids are dense over all of it in index order, so cloud c owns the ids from pos[bases[c]] on
        hipLaunchKernelGGL(k_rgb_cloud_ids, dim3(g1((size_t)run.n_clouds + 1)), dim3(256), 0, s, flags, run.d_bases, run.n_clouds, run.d_id_bases);
        PCC_HIP(hipGetLastError());
        PCC_HIP(hipMemcpyAsync(run.h_id_bases, run.d_id_bases, ((size_t)run.n_clouds + 1) * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
        PCC_HIP(hipStreamSynchronize(s));
        ns = run.h_id_bases[run.n_clouds];
    } else {
        PCC_TRY(read_back(ix, flags + n, &ns));
        if (ns == 0) { set_error("colour region growing: no segment over %u points", n); return PCC_ERR_DEVICE; }
    }
    if (ns > n) { set_error("colour region growing: %u segments over %u points", ns, n); return PCC_ERR_DEVICE; }
    // per-segment records, and the count of what the pair table has to hold
    unsigned int np = 0;
    RgbSegment* h_stats = nullptr;
    RgbSegmentPair* h_pairs = nullptr;
    if (ns) {  // (a concatenation without a finite point has no segment: every label is -1)
        PCC_TRY(ix->scratch_b.reserve((size_t)ns * sizeof(RgbSegment)));
        RgbSegment* d_stats = ix->scratch_b.as<RgbSegment>();
        PCC_HIP(hipMemsetAsync(d_stats, 0, (size_t)ns * sizeof(RgbSegment), s));
        PCC_HIP(hipMemsetAsync(d_words, 0, sizeof(DevWords::op), s));
        hipLaunchKernelGGL(k_rgb_stats<Order>, dim3(g1(n)), dim3(256), 0, s, order, seg, col, ns, d_stats);
        hipLaunchKernelGGL((k_rgb_pairs<false, Order>), dim3(wave_blocks), dim3(256), 0, s, keys, seg, order, K, d_words,
                           (unsigned long long*)nullptr, (unsigned int*)nullptr, 0, d_words + 2);
        PCC_HIP(hipGetLastError());
        unsigned int n_first = 0;
        PCC_TRY(read_back(ix, d_words, &n_first));
        PCC_TRY(ix->host_a.reserve((size_t)ns * sizeof(RgbSegment)));
        h_stats = ix->host_a.as<RgbSegment>();
        PCC_HIP(hipMemcpyAsync(h_stats, d_stats, (size_t)ns * sizeof(RgbSegment), hipMemcpyDeviceToHost, s));
        if (n_first) {
            int log2_size = 10;
            while (((size_t)1 << log2_size) < (size_t)n_first * 2) ++log2_size;
            const size_t tsize = (size_t)1 << log2_size;
            PCC_TRY(ix->vox_a.reserve(tsize * sizeof(unsigned long long)));
            PCC_TRY(ix->vox_b.reserve(tsize * sizeof(unsigned int)));
            PCC_TRY(ix->rows_idx.reserve((size_t)n_first * sizeof(RgbSegmentPair)));
            auto* tkeys = ix->vox_a.as<unsigned long long>();
            auto* tdist = ix->vox_b.as<unsigned int>();
            auto* d_pairs = ix->rows_idx.as<RgbSegmentPair>();
            PCC_HIP(hipMemsetAsync(tkeys, 0xff, tsize * sizeof(unsigned long long), s));
            PCC_HIP(hipMemsetAsync(tdist, 0xff, tsize * sizeof(unsigned int), s));
            hipLaunchKernelGGL((k_rgb_pairs<true, Order>), dim3(wave_blocks), dim3(256), 0, s, keys, seg, order, K, d_words, tkeys, tdist,
                               log2_size, d_words + 2);
            hipLaunchKernelGGL(k_rgb_compact_pairs, dim3(g1(tsize)), dim3(256), 0, s, tkeys, tdist, tsize, d_pairs, d_words + 1, n_first);
            PCC_HIP(hipGetLastError());
            // the count and the list in one wait: the list's head comes down beside the count, the rest only when there is more
            const unsigned int head = std::min(n_first, RGB_PAIRS_FIRST_COPY);
            PCC_TRY(ix->host_b.reserve((size_t)head * sizeof(RgbSegmentPair)));
            PCC_HIP(hipMemcpyAsync(ix->pinned()->readback, d_words, 3 * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
            PCC_HIP(hipMemcpyAsync(ix->host_b.p, d_pairs, (size_t)head * sizeof(RgbSegmentPair), hipMemcpyDeviceToHost, s));
            PCC_HIP(hipStreamSynchronize(s));
            unsigned int w[3];  // -, pairs listed, table overflow
            memcpy(w, ix->pinned()->readback, sizeof(w));
            np = w[1];
            if (w[2] || np > n_first) { set_error("segment pair table overflow (%u pairs, room for %u)", np, n_first); return PCC_ERR_OVERFLOW; }
            if (np > head) {
                PCC_TRY(ix->host_b.reserve((size_t)np * sizeof(RgbSegmentPair)));  // (may move: everything comes down again)
                PCC_HIP(hipMemcpyAsync(ix->host_b.p, d_pairs, (size_t)np * sizeof(RgbSegmentPair), hipMemcpyDeviceToHost, s));
                PCC_HIP(hipStreamSynchronize(s));
            }
            h_pairs = ix->host_b.as<RgbSegmentPair>();
        } else {
            PCC_HIP(hipStreamSynchronize(s));
        }
    }
    // the host half: the nearest segments of every segment, PCL's merging, folding and size filter
    std::vector<int32_t> cluster_of_segment;
    PCC_TRY(host_half(h_stats, ns, h_pairs, np, cluster_of_segment));
    if (cluster_of_segment.size() != ns) { set_error("colour region growing: %zu cluster ids for %u segments", cluster_of_segment.size(), ns); return PCC_ERR_DEVICE; }
    if (run.labels_dev) {
        int32_t* d_ids = nullptr;
        if (ns) {
            int32_t* h_ids = ix->host_a.as<int32_t>();  // (the records are used up; ns x 16 bytes hold ns ids)
            std::copy(cluster_of_segment.begin(), cluster_of_segment.end(), h_ids);
            PCC_TRY(ix->rows_d2.reserve((size_t)ns * sizeof(int32_t)));
            d_ids = ix->rows_d2.as<int32_t>();
            PCC_HIP(hipMemcpyAsync(d_ids, h_ids, (size_t)ns * sizeof(int32_t), hipMemcpyHostToDevice, s));
        }
        hipLaunchKernelGGL(k_rgb_label, dim3(g1(n)), dim3(256), 0, s, seg, d_ids, n, ns, run.labels_dev);
        PCC_HIP(hipGetLastError());
        if (run.labels_host) PCC_HIP(hipMemcpyAsync(run.labels_host, run.labels_dev, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        ev_mark(ix, EV_MAIN1);
        PCC_HIP(hipStreamSynchronize(s));  // h_ids may be rewritten by the next call
    } else {
        ev_mark(ix, EV_MAIN1);  // (counts only: nothing has been enqueued since the wait for the pair list)
    }
    ix->stats[0] = ns;
    ix->stats[1] = np;
    ix->stats[7] = sweeps;
    ix->stats_pending = false;
    ix->open_pending = false;
    return PCC_OK;
}

}  // namespace

// the stages behind the rows (rgb_stages.hpp), over one indexed cloud in cell order or over a concatenation in index order
int rgb_stages(pcc_index* ix, const RgbRun& run, const RgbHostHalf& host_half) {
    if (run.cell_refs) return rgb_stages_in(ix, run, ByCell{run.cell_refs, run.gd}, host_half);
    return rgb_stages_in(ix, run, ByIndex{run.n}, host_half);
}

// keys: the self k-NN rows of the index (n x K); rgb: the colour words on the device (stride bytes apart); labels_dev[n]
int grid_region_growing_rgb(pcc_index* ix, const unsigned long long* keys, int K, const unsigned char* rgb, size_t rgb_stride,
                            float distance_threshold, float point_color_threshold, float region_color_threshold, uint32_t min_size,
                            uint32_t max_size, unsigned int nr_neighbours, unsigned int nr_region_neighbours, int32_t* labels_dev,
                            int32_t* n_clusters) {
    RgbRun run;
    run.refs = ix->refs.as<float4>();
    run.n = (unsigned int)ix->n_orig;
    run.keys = keys;
    run.K = K;
    run.rgb = rgb;
    run.rgb_stride = rgb_stride;
    run.cell_refs = ix->cell_refs.as<float4>();
    run.gd = ix->d_grid.as<GridDev>();
    run.point_color_threshold = point_color_threshold;
    run.nr_neighbours = nr_neighbours;
    run.labels_dev = labels_dev;
    const float dist2 = distance_threshold * distance_threshold, r2r2 = region_color_threshold * region_color_threshold;
    const int min_pts = (int)std::min<uint32_t>(min_size, 0x7fffffffu), max_pts = (int)std::min<uint32_t>(max_size, 0x7fffffffu);
    return rgb_stages(ix, run, [&](const RgbSegment* segs, unsigned int ns, RgbSegmentPair* pairs, unsigned int np, std::vector<int32_t>& cluster_of_segment) {
        *n_clusters = (int32_t)rgb_merge_regions(segs, ns, pairs, np, dist2, r2r2, nr_region_neighbours, min_pts, max_pts, cluster_of_segment);
        return PCC_OK;
    });
}

int check_rgb_params(float distance_threshold, float point_color_threshold, float region_color_threshold, unsigned int nr_neighbours,
                     unsigned int nr_region_neighbours) {
    for (float t : {distance_threshold, point_color_threshold, region_color_threshold})
        if (!(t >= 0.f) || !std::isfinite(t)) { set_error("bad threshold"); return PCC_ERR_INVALID; }
    if (nr_neighbours == 0 || nr_region_neighbours == 0 || nr_region_neighbours > PCC_KNN_MAX_K) {
        set_error("colour region growing with %u / %u neighbours: both must be at least 1, the region neighbours at most %d", nr_neighbours,
                  nr_region_neighbours, PCC_KNN_MAX_K);
        return PCC_ERR_UNSUPPORTED;
    }
    return PCC_OK;
}

}  // namespace pcc

using namespace pcc;
extern "C" {
int pcc_region_growing_rgb(pcc_index* ix, const void* rgb, size_t rgb_stride, int mem, float distance_threshold,
                           float point_color_threshold, float region_color_threshold, uint32_t min_size, uint32_t max_size,
                           unsigned int nr_neighbours, unsigned int nr_region_neighbours, int32_t* labels, int32_t* n_clusters) {
    // the arguments first: host arithmetic, refused before any device is looked at
    PCC_TRY(check_mem(mem));
    if (!rgb || !labels || !n_clusters) { set_error("null argument"); return PCC_ERR_INVALID; }
    if (rgb_stride < 4 || rgb_stride % 4 || reinterpret_cast<uintptr_t>(rgb) % 4) {
        set_error("colour words must be 4-byte aligned, stride %zu a multiple of 4 and >= 4", rgb_stride);
        return PCC_ERR_INVALID;
    }
    PCC_TRY(check_rgb_params(distance_threshold, point_color_threshold, region_color_threshold, nr_neighbours, nr_region_neighbours));
    PCC_ENTER(ix);
    PCC_TRY(ensure_grid(ix));
    PCC_TRY(sync_info(ix));
    if (ix->n_valid == 0) { set_error("index holds no finite point"); return PCC_ERR_EMPTY; }
    ev_next(ix);
    ev_mark(ix, EV_CALL0);
    const size_t n = ix->n_orig;
    // findPointNeighbours: one batched self k-NN over the packed references, K = min(nr_region_neighbours, points)
    const int K = (int)std::min<size_t>(nr_region_neighbours, ix->n_valid);
    if (n * (size_t)K >= ((size_t)1 << 32)) { set_error("%zu x %d row entries: 2^32 and more are not built", n, K); return PCC_ERR_UNSUPPORTED; }
    const unsigned long long* keys = nullptr;
    PCC_TRY(self_knn_keys(ix, K, &keys));
    const unsigned char* drgb = nullptr;
    PCC_TRY(stage_in(ix, reinterpret_cast<const unsigned char*>(rgb), (n - 1) * rgb_stride + 4, mem, ix->out_d2, &drgb));
    Out<int32_t> rl;
    PCC_TRY(rl.stage(labels, n, mem, ix->q_raw));
    PCC_TRY(grid_region_growing_rgb(ix, keys, K, drgb, rgb_stride, distance_threshold, point_color_threshold, region_color_threshold,
                                    min_size, max_size, nr_neighbours, nr_region_neighbours, rl.dev, n_clusters));
    ev_mark(ix, EV_CALL1);
    return finish(ix, mem, rl);
}
}  // extern "C"
