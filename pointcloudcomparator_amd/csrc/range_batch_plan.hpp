// range_batch_plan.hpp -- the host scaffold of the batch calls whose clusters are RANGES OF ONE ARRAY of records
// (pcc_fpfh_descriptors_batch, pcc_vfh_descriptors_batch): the one check of cluster offsets in the library, the
// split into the batch route and the work-handle route, the host pack and the layout of the one buffer a call goes up in.
// Plain C++ (no HIP): tests/cpp/test_range_batch_plan.cpp compiles it on its own.
#pragma once
#include <initializer_list>

#include "cloud_batch.hpp"

namespace pcc {

// ---- the offsets: cluster c is records offsets[c] .. offsets[c + 1] ------------------------------------------------------------
// refused for, in this order: any decrease (*bad, nullable: the first such cluster), then the size (2^31 clusters or records)
enum : int { RANGE_OFFSETS_OK = 0, RANGE_OFFSETS_DECREASE = 1, RANGE_OFFSETS_TOO_MANY = 2 };
inline int check_range_offsets(const size_t* offsets, size_t n_clusters, size_t* bad = nullptr) {
    for (size_t c = 0; c < n_clusters; ++c)
        if (offsets[c + 1] < offsets[c]) { if (bad) *bad = c; return RANGE_OFFSETS_DECREASE; }
    if (n_clusters >= (1ull << 31) || (n_clusters && offsets[n_clusters] - offsets[0] >= (1ull << 31))) return RANGE_OFFSETS_TOO_MANY;
    return RANGE_OFFSETS_OK;
}
// one or two scenes: every scene's decrease comes before any scene's size.  *side: the refused scene, counted from 1
struct ClusterOffsets {
    const size_t* offsets;
    size_t n_clusters;
};
inline int check_scene_offsets(std::initializer_list<ClusterOffsets> scenes, int* side, size_t* bad) {
    for (const int refusal : {(int)RANGE_OFFSETS_DECREASE, (int)RANGE_OFFSETS_TOO_MANY}) {
        *side = 0;
        for (const ClusterOffsets& s : scenes) {
            ++*side;
            if (check_range_offsets(s.offsets, s.n_clusters, bad) == refusal) return refusal;
        }
    }
    return RANGE_OFFSETS_OK;
}

// ---- the clusters of a call and their routes ----------------------------------------------------------------------------------
// records of `stride` bytes (x, y, z first) in host or device memory (mem); pts is not read while no cluster holds a point
struct ClusterRanges {
    const unsigned char* pts;
    size_t stride;
    const size_t* offsets;
    size_t n_clusters;
    int mem;
    const unsigned char* cluster(size_t c) const { return pts + offsets[c] * stride; }
};

// The clusters of min_points .. limit points form the concatenation the batch kernels run over (bases and work items as
// rift_batch_plan builds them: a cluster off that route has size 0 there and shares its base with the cluster behind it); the
// larger ones take the single call on the work handle, one by one; a cluster below min_points is on neither and is never read.
struct RangeBatchPlan {
    std::vector<size_t> n;          // points of cluster c
    std::vector<size_t> small_n;    // n[c] on the batch route, else 0
    std::vector<uint32_t> src;      // n_clusters + 1: offsets[c] - offsets[0], where cluster c starts among the caller's records
    std::vector<uint32_t> bases;    // n_clusters + 1: where it starts in the concatenation (the last entry: its points)
    std::vector<RiftBatchItem> items;  // the row builder's work items
    size_t n_brute = 0, n_large = 0;   // points on either route
    size_t min_points = 0;
    bool on_work_handle(size_t c) const { return n[c] >= min_points && n[c] != small_n[c]; }
    size_t total() const { return bases.back(); }
};
inline RangeBatchPlan range_batch_plan(const size_t* offsets, size_t n_clusters, size_t min_points, size_t limit) {
    RangeBatchPlan p;
    p.min_points = min_points;
    p.n.assign(n_clusters, 0);
    p.small_n.assign(n_clusters, 0);
    p.src.assign(n_clusters + 1, 0u);
    for (size_t c = 0; c <= n_clusters; ++c) p.src[c] = n_clusters ? (uint32_t)(offsets[c] - offsets[0]) : 0u;
    for (size_t c = 0; c < n_clusters; ++c) {
        const size_t n = p.n[c] = offsets[c + 1] - offsets[c];
        if (n < min_points) continue;
        if (n <= limit) p.small_n[c] = n;
        (n > limit ? p.n_large : p.n_brute) += n;
    }
    rift_batch_plan(p.small_n.data(), n_clusters, &p.bases, &p.items);
    return p;
}

// The batch route's points of a caller in host memory: p4[at] = x, y, z, w = bits(at) for point at = bases[c] + i.  With
// refuse_non_finite the first non-finite point -- clusters in ascending order -- ends the pack: false, *bad its cluster.
inline bool pack_ranges(const ClusterRanges& r, const RangeBatchPlan& p, bool refuse_non_finite, float* p4, size_t* bad) {
    for (size_t c = 0; c < r.n_clusters; ++c) {
        const size_t n = p.small_n[c];
        const unsigned char* src = n ? r.cluster(c) : nullptr;  // (hoisted: the loop below runs once a point)
        for (size_t i = 0; i < n; ++i) {
            const uint32_t at = p.bases[c] + (uint32_t)i;
            float v[3];
            memcpy(v, src + i * r.stride, 12);
            if (refuse_non_finite && !finite3(v[0], v[1], v[2])) { *bad = c; return false; }
            memcpy(p4 + (size_t)at * 4, v, 12);
            memcpy(p4 + (size_t)at * 4 + 3, &at, 4);
        }
    }
    return true;
}

// ---- the upload.  carve: a typed part of a buffer at an offset of a layout -- the pinned buffer and its device copy alike ------
template <class T> T* carve(char* b, size_t at) { return reinterpret_cast<T*>(b + at); }
template <class T> const T* carve(const char* b, size_t at) { return reinterpret_cast<const T*>(b + at); }

// One pinned buffer, one copy: GridDev | src[n_clusters + 1] | extra_bytes of the call's own | ConcatLayout(bases, items, from
// host memory 16 bytes a point; no colour is read: the layout's last part is not used).
constexpr size_t RANGE_GRID_BYTES = 112;      // sizeof(GridDev), 16-byte aligned: asserted in range_batch.hip
constexpr size_t RANGE_GRID_N_VALID_AT = 52;  // offsetof(GridDev, n_valid): the one word of it the consumers read
struct RangeUpload {
    size_t extra_at;  // where the call's own part starts: 4-byte aligned
    ConcatLayout concat;
    static size_t extra_start(size_t n_clusters) { return RANGE_GRID_BYTES + (n_clusters + 1) * sizeof(uint32_t); }
    RangeUpload(const RangeBatchPlan& p, size_t extra_bytes)
        : extra_at(extra_start(p.n.size())), concat(extra_at + extra_bytes, 128, p.n.size(), p.items.size(), p.total()) {}
    size_t bytes(bool host_points) const { return host_points ? concat.rgb_at : concat.pts_at; }  // what goes up
    size_t device_bytes() const { return concat.rgb_at; }
    template <class C> auto src(C* b) const { return carve<uint32_t>(b, RANGE_GRID_BYTES); }
    template <class C> auto extra(C* b) const { return carve<char>(b, extra_at); }
    template <class C> auto bases(C* b) const { return carve<uint32_t>(b, concat.bases_at); }
    template <class C> auto items(C* b) const { return carve<RiftBatchItem>(b, concat.items_at); }
    template <class C> auto pts(C* b) const { return carve<float>(b, concat.pts_at); }
    // all in front of the items zeroed (the extra part is the caller's to fill), n_valid = total, the tables, a host caller's pack
    bool fill(char* u, const ClusterRanges& r, const RangeBatchPlan& p, bool host_points, bool refuse_non_finite, size_t* bad) const {
        memset(u, 0, concat.items_at);
        const uint32_t n_valid = (uint32_t)p.total();
        memcpy(u + RANGE_GRID_N_VALID_AT, &n_valid, 4);
        memcpy(src(u), p.src.data(), p.src.size() * sizeof(uint32_t));
        memcpy(bases(u), p.bases.data(), p.bases.size() * sizeof(uint32_t));
        if (!p.items.empty()) memcpy(items(u), p.items.data(), p.items.size() * sizeof(RiftBatchItem));
        return !host_points || pack_ranges(r, p, refuse_non_finite, pts(u), bad);
    }
};

}  // namespace pcc
