// cloud_batch.hpp -- the host scaffold the "every cloud at once" calls share (rift_batch.hip, sift_batch.hip,
// region_rgb_batch.hip): the caller's clouds as one argument, the split into the batch route and the work-handle route, the
// pack of the concatenation and the layout of the one buffer it goes up in.  The calls whose clusters are ranges of ONE array
// (fpfh_batch.hip, vfh_batch.hip) build on finite3, align_up and ConcatLayout in range_batch_plan.hpp.
// Plain C++ (no HIP): tests/cpp/test_cloud_batch.cpp compiles it on its own.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "rift_batch_plan.hpp"

#if defined(__HIPCC__)
#define PCC_HOST_DEVICE __host__ __device__
#else
#define PCC_HOST_DEVICE
#endif

namespace pcc {

// the host clouds of one call: n[c] records of `stride` bytes at pts[c] (x, y, z first), their colour words rgb_stride apart
// at rgb[c]; the pointers of an empty cloud are not read
struct CloudBatch {
    size_t n_clouds;
    const void* const* pts;
    const size_t* n;
    size_t stride;
    const void* const* rgb;
    size_t rgb_stride;
};

// the library's finiteness test, host and device: v - v is 0 for a finite v, NaN for NaN and both infinities
PCC_HOST_DEVICE inline bool finite3(float x, float y, float z) { return (x - x) == 0.0f && (y - y) == 0.0f && (z - z) == 0.0f; }

inline bool cloud_any_finite(const void* pts, size_t n, size_t stride) {
    const char* p = static_cast<const char*>(pts);
    for (size_t i = 0; i < n; ++i) {
        float v[3];
        memcpy(v, p + i * stride, 12);
        if (finite3(v[0], v[1], v[2])) return true;
    }
    return false;
}

// Clouds above `limit` points leave the batch route for the work handle.  small_n[c]: n[c] on the batch route, 0 for a cloud
// that left it (an empty cloud of the batch: its slice comes from the work handle); the points on either route.
struct BatchRoutes {
    std::vector<size_t> small_n;
    size_t n_brute = 0, n_large = 0;
};
inline BatchRoutes batch_routes(const size_t* n, size_t n_clouds, size_t limit) {
    BatchRoutes r;
    r.small_n.assign(n, n + n_clouds);
    for (size_t c = 0; c < n_clouds; ++c) {
        (n[c] > limit ? r.n_large : r.n_brute) += n[c];
        if (n[c] > limit) r.small_n[c] = 0;
    }
    return r;
}

// The concatenation of a batch (bases[c] + i is point i of cloud c): p4[at] = x, y, z, w = bits(at) -- ~0, a negative w, for a
// non-finite point when mark_non_finite -- and words[at] = the point's colour word.
inline void pack_clouds(const CloudBatch& b, const uint32_t* bases, bool mark_non_finite, float* p4, uint32_t* words) {
    for (size_t c = 0; c < b.n_clouds; ++c) {
        const char* src = static_cast<const char*>(b.pts[c]);
        const char* col = static_cast<const char*>(b.rgb[c]);
        for (size_t i = 0; i < b.n[c]; ++i) {
            const size_t at = bases[c] + i;
            float v[3];
            memcpy(v, src + i * b.stride, 12);
            const uint32_t w = mark_non_finite && !finite3(v[0], v[1], v[2]) ? 0xffffffffu : (uint32_t)at;
            memcpy(p4 + at * 4, v, 12);
            memcpy(p4 + at * 4 + 3, &w, 4);
            memcpy(words + at, col + i * b.rgb_stride, 4);
        }
    }
}

inline size_t align_up(size_t b, size_t a) { return (b + a - 1) / a * a; }

// One buffer, several aligned parts -- the upload of a packed concatenation (bases and items: rift_batch_plan.hpp), laid out
// for one copy: header_bytes of the caller's | bases[n_clouds + 1] at header_align | items | float4 points | colour words.
struct ConcatLayout {
    size_t bases_at, items_at, pts_at, rgb_at, bytes;
    ConcatLayout(size_t header_bytes, size_t header_align, size_t n_clouds, size_t n_items, size_t total) {
        bases_at = align_up(header_bytes, header_align);
        items_at = align_up(bases_at + (n_clouds + 1) * sizeof(uint32_t), 16);
        pts_at = items_at + n_items * sizeof(RiftBatchItem);
        rgb_at = pts_at + total * 4 * sizeof(float);
        bytes = rgb_at + total * sizeof(uint32_t);
    }
    // everything in front of the items zeroed (the header is the caller's to fill), then the tables and the pack
    void fill(char* u, const CloudBatch& b, const std::vector<uint32_t>& bases, const std::vector<RiftBatchItem>& items, bool mark_non_finite) const {
        memset(u, 0, items_at);
        memcpy(u + bases_at, bases.data(), bases.size() * sizeof(uint32_t));
        if (!items.empty()) memcpy(u + items_at, items.data(), items.size() * sizeof(RiftBatchItem));
        pack_clouds(b, bases.data(), mark_non_finite, reinterpret_cast<float*>(u + pts_at), reinterpret_cast<uint32_t*>(u + rgb_at));
    }
};

}  // namespace pcc
