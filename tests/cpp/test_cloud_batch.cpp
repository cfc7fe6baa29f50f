// csrc/cloud_batch.hpp on the CPU (no library, no GPU): the route split, the pack of a concatenation against a naive per-point
// reference, the finiteness test against std::isfinite, and the layouts of the three batch uploads against offsets recorded from
// the arithmetic each call carried of its own before the header existed.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "cloud_batch.hpp"
#include "sift_batch_plan.hpp"

using namespace pcc;

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            ++failures;                                   \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
        }                                                 \
    } while (0)

static float from_bits(uint32_t b) {
    float f;
    memcpy(&f, &b, 4);
    return f;
}

static void test_routes() {
    const size_t n[] = {0, 1, 26, 65, 300, 2049};
    const size_t nc = sizeof(n) / sizeof(n[0]);
    struct Case { size_t limit, n_brute, n_large; } cases[] = {
        {299, 92, 2349},   // below a cloud's size
        {300, 392, 2049},  // at it
        {301, 392, 2049},  // above it
        {2049, 2441, 0},   // every cloud on the batch route
        {0, 0, 2441},      // every cloud with a point on the work handle
    };
    for (const Case& k : cases) {
        const BatchRoutes r = batch_routes(n, nc, k.limit);
        CHECK(r.n_brute == k.n_brute && r.n_large == k.n_large, "limit %zu: %zu + %zu points, expected %zu + %zu", k.limit, r.n_brute, r.n_large,
              k.n_brute, k.n_large);
        CHECK(r.small_n.size() == nc, "limit %zu: %zu sizes", k.limit, r.small_n.size());
        for (size_t c = 0; c < nc; ++c)
            CHECK(r.small_n[c] == (n[c] > k.limit ? 0 : n[c]), "limit %zu: cloud %zu keeps %zu of %zu points", k.limit, c, r.small_n[c], n[c]);
    }
    const BatchRoutes none = batch_routes(nullptr, 0, 8192);
    CHECK(none.small_n.empty() && none.n_brute == 0 && none.n_large == 0, "no cloud at all");
}

// clouds of 0, 1, 2 and 65 points at the given strides, NaN / +inf / -inf coordinates among them
static void test_pack(size_t stride, size_t rgb_stride) {
    const size_t n[] = {0, 1, 2, 65, 0, 2};
    const size_t nc = sizeof(n) / sizeof(n[0]);
    const float specials[] = {from_bits(0x7fc12345u), INFINITY, -INFINITY, from_bits(0xffa00001u)};
    std::vector<std::vector<unsigned char>> raw(nc), col(nc);
    std::vector<const void*> pts(nc, nullptr), rgb(nc, nullptr);
    std::vector<uint32_t> bases(nc + 1, 0);
    uint32_t seed = 12345u;
    auto next = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed; };
    for (size_t c = 0; c < nc; ++c) {
        bases[c + 1] = bases[c] + (uint32_t)n[c];
        raw[c].assign(n[c] * stride + 1, 0xAB);  // (filler between the records must not be read as coordinates)
        col[c].assign(n[c] * rgb_stride + 1, 0xCD);
        for (size_t i = 0; i < n[c]; ++i) {
            float v[3];
            for (int a = 0; a < 3; ++a) v[a] = (float)(next() % 2000) * 0.001f - 1.0f;
            if (next() % 4 == 0) v[next() % 3] = specials[next() % 4];
            if (c == 2 && i == 1) v[0] = v[1] = v[2] = specials[0];
            const uint32_t word = next();
            memcpy(raw[c].data() + i * stride, v, 12);
            memcpy(col[c].data() + i * rgb_stride, &word, 4);
        }
        if (n[c]) { pts[c] = raw[c].data(); rgb[c] = col[c].data(); }
    }
    const CloudBatch b{nc, pts.data(), n, stride, rgb.data(), rgb_stride};
    const size_t total = bases[nc];
    size_t marked = 0;
    for (int mark = 0; mark < 2; ++mark) {
        std::vector<float> p4(total * 4 + 4, -7.0f);
        std::vector<uint32_t> words(total + 1, 0x5a5a5a5au);
        pack_clouds(b, bases.data(), mark != 0, p4.data(), words.data());
        for (size_t c = 0; c < nc; ++c)
            for (size_t i = 0; i < n[c]; ++i) {
                const size_t at = bases[c] + i;
                float v[3];
                uint32_t word, w;
                memcpy(v, raw[c].data() + i * stride, 12);
                memcpy(&word, col[c].data() + i * rgb_stride, 4);
                memcpy(&w, &p4[at * 4 + 3], 4);
                const bool fin = std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]);
                const uint32_t want = (mark && !fin) ? 0xffffffffu : (uint32_t)at;
                if (mark && !fin) ++marked;
                CHECK(memcmp(&p4[at * 4], v, 12) == 0, "strides %zu / %zu, mark %d: cloud %zu point %zu: coordinates changed", stride, rgb_stride, mark, c, i);
                CHECK(w == want, "strides %zu / %zu, mark %d: cloud %zu point %zu: w %08x, expected %08x", stride, rgb_stride, mark, c, i, w, want);
                CHECK(words[at] == word, "strides %zu / %zu, mark %d: cloud %zu point %zu: colour word", stride, rgb_stride, mark, c, i);
            }
        CHECK(p4[total * 4] == -7.0f && words[total] == 0x5a5a5a5au, "strides %zu / %zu: the pack wrote past the concatenation", stride, rgb_stride);
    }
    CHECK(marked > 0, "strides %zu / %zu: no non-finite point among the clouds", stride, rgb_stride);
}

static void test_any_finite() {
    const float nan = from_bits(0x7fc00000u);
    float all_nan[5][4], last[5][4];
    for (int i = 0; i < 5; ++i)
        for (int a = 0; a < 4; ++a) { all_nan[i][a] = nan; last[i][a] = a == 1 ? INFINITY : nan; }
    last[4][0] = 0.f; last[4][1] = -1.f; last[4][2] = FLT_MAX;
    CHECK(!cloud_any_finite(all_nan, 5, 16), "an all-NaN cloud has a finite point");
    CHECK(cloud_any_finite(last, 5, 16), "the finite last point was missed");
    CHECK(!cloud_any_finite(last, 4, 16), "a point with one infinite coordinate counts as finite");
    CHECK(!cloud_any_finite(nullptr, 0, 16), "an empty cloud has a finite point");
}

static void test_finite3() {
    const float edge[] = {0.0f, -0.0f, FLT_MIN, -FLT_MIN, from_bits(1u), from_bits(0x80000001u), from_bits(0x007fffffu), FLT_MAX, -FLT_MAX, 1.0f,
                          INFINITY, -INFINITY, from_bits(0x7fc00000u), from_bits(0xffc00000u), from_bits(0x7f800001u), from_bits(0x7fc12345u),
                          from_bits(0xffa00001u)};
    const size_t ne = sizeof(edge) / sizeof(edge[0]);
    for (size_t i = 0; i < ne; ++i)
        for (size_t j = 0; j < ne; ++j)
            for (size_t k = 0; k < ne; ++k) {
                const bool want = std::isfinite(edge[i]) && std::isfinite(edge[j]) && std::isfinite(edge[k]);
                CHECK(finite3(edge[i], edge[j], edge[k]) == want, "finite3(%a, %a, %a) is not %d", edge[i], edge[j], edge[k], (int)want);
            }
}

// The expected offsets: the arithmetic the three calls used before they shared a header (align_up by hand around
// sizeof(GridDev) = 112, 16-byte work items, 16 + 4 bytes a point), run once and written down.
static void test_layouts() {
    static_assert(sizeof(RiftBatchItem) == 16, "work item size");
    struct Concat { size_t n_clouds, n_items, total, rift[5], rgb[4]; } concat[] = {
        // rift: bases, items, points, colour words, bytes; rgb: items, points, colour words, bytes (bases at 0)
        {1, 0, 7, {128, 144, 144, 256, 284}, {16, 16, 128, 156}},
        {1, 3, 7, {128, 144, 192, 304, 332}, {16, 64, 176, 204}},
        {5, 0, 1234, {128, 160, 160, 19904, 24840}, {32, 32, 19776, 24712}},
        {5, 3, 1234, {128, 160, 208, 19952, 24888}, {32, 80, 19824, 24760}},
    };
    for (const Concat& k : concat) {
        const ConcatLayout rift(112, 128, k.n_clouds, k.n_items, k.total);  // pcc_rift_descriptors_batch: a GridDev in front
        CHECK(rift.bases_at == k.rift[0] && rift.items_at == k.rift[1] && rift.pts_at == k.rift[2] && rift.rgb_at == k.rift[3] && rift.bytes == k.rift[4],
              "rift upload, %zu clouds, %zu items: %zu %zu %zu %zu %zu", k.n_clouds, k.n_items, rift.bases_at, rift.items_at, rift.pts_at, rift.rgb_at,
              rift.bytes);
        const ConcatLayout rgb(0, 1, k.n_clouds, k.n_items, k.total);  // pcc_region_growing_rgb_batch: no header
        CHECK(rgb.bases_at == 0 && rgb.items_at == k.rgb[0] && rgb.pts_at == k.rgb[1] && rgb.rgb_at == k.rgb[2] && rgb.bytes == k.rgb[3],
              "rgb upload, %zu clouds, %zu items: %zu %zu %zu %zu %zu", k.n_clouds, k.n_items, rgb.bases_at, rgb.items_at, rgb.pts_at, rgb.rgb_at,
              rgb.bytes);
    }
    // pcc_sift_keypoints_batch's round table behind at0 bytes: int64 bases, uint32 bases, items, the whole rounded up to 16
    struct Table { size_t n_clouds, n_items, at0, want[4]; } tables[] = {
        {1, 0, 0, {0, 16, 32, 32}},    {1, 0, 1000, {1008, 1024, 1040, 1040}}, {1, 3, 0, {0, 16, 32, 80}},    {1, 3, 1000, {1008, 1024, 1040, 1088}},
        {5, 0, 0, {0, 48, 80, 80}},    {5, 0, 1000, {1008, 1056, 1088, 1088}}, {5, 3, 0, {0, 48, 80, 128}},   {5, 3, 1000, {1008, 1056, 1088, 1136}},
    };
    for (const Table& k : tables) {
        const TableLayout t(k.n_clouds, k.n_items, k.at0);
        CHECK(t.bases64_at == k.want[0] && t.bases_at == k.want[1] && t.items_at == k.want[2] && t.bytes == k.want[3],
              "sift table, %zu clouds, %zu items behind %zu bytes: %zu %zu %zu %zu", k.n_clouds, k.n_items, k.at0, t.bases64_at, t.bases_at, t.items_at, t.bytes);
    }
    // fill(): the header and the padding zeroed, the tables and the pack where the layout says
    const size_t n[] = {2, 0, 1};
    const float xyz[3][3] = {{1, 2, 3}, {4, NAN, 6}, {7, 8, 9}};
    const uint32_t colours[3] = {0x11u, 0x22u, 0x33u};
    const void* pts[] = {xyz[0], nullptr, xyz[2]};
    const void* rgb[] = {&colours[0], nullptr, &colours[2]};
    const CloudBatch b{3, pts, n, 12, rgb, 4};
    std::vector<uint32_t> bases;
    std::vector<RiftBatchItem> items;
    rift_batch_plan(n, 3, &bases, &items);
    const ConcatLayout up(112, 128, 3, items.size(), bases[3]);
    std::vector<char> u(up.bytes + 1, (char)0x77);
    up.fill(u.data(), b, bases, items, true);
    for (size_t i = 0; i < up.bases_at; ++i) CHECK(u[i] == 0, "header byte %zu not zeroed", i);
    CHECK(memcmp(u.data() + up.bases_at, bases.data(), 16) == 0 && memcmp(u.data() + up.items_at, items.data(), items.size() * 16) == 0, "tables");
    uint32_t w[3];
    for (int i = 0; i < 3; ++i) memcpy(&w[i], u.data() + up.pts_at + i * 16 + 12, 4);
    CHECK(w[0] == 0 && w[1] == 0xffffffffu && w[2] == 2, "w words %08x %08x %08x", w[0], w[1], w[2]);
    CHECK(memcmp(u.data() + up.rgb_at, colours, 12) == 0 && u[up.bytes] == (char)0x77, "colour words, or a write past the upload");
}

int main() {
    test_routes();
    for (size_t stride : {12, 16, 32})
        for (size_t rgb_stride : {4, 32}) test_pack(stride, rgb_stride);
    test_any_finite();
    test_finite3();
    test_layouts();
    if (failures) {
        std::printf("cloud batch: %d failures\n", failures);
        return 1;
    }
    std::printf("cloud batch ok: routes, pack at 3 x 2 strides in both marking modes, finiteness, 3 upload layouts\n");
    return 0;
}
