// test_range_batch_plan.cpp -- csrc/range_batch_plan.hpp on the CPU (no library, no GPU): the routes of range_batch_plan and
// the two uploads (RangeUpload alone for pcc_fpfh_descriptors_batch, with VfhUploadExtra for pcc_vfh_descriptors_batch) against
// values recorded from the arithmetic each call carried of its own before the header existed; the host pack with and without
// its refusal of non-finite points; the offsets' refusals, for one scene and for two.
// usage: test_range_batch_plan   (no arguments; exit status 0 and one line "range batch plan ok: ..." when every case holds)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fpfh_batch_plan.hpp"
#include "vfh_batch_plan.hpp"

using namespace pcc;

static int failures = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            ++failures;                                      \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                        \
            std::printf("\n");                               \
        }                                                    \
    } while (0)

static std::vector<size_t> offsets_of(const std::vector<size_t>& sizes, size_t first) {
    std::vector<size_t> off(sizes.size() + 1, first);
    for (size_t c = 0; c < sizes.size(); ++c) off[c + 1] = off[c] + sizes[c];
    return off;
}
template <class A, class B>
static bool same(const std::vector<A>& a, const std::vector<B>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if ((size_t)a[i] != (size_t)b[i]) return false;
    return true;
}

// ---- the plan: min_points 0 was fpfh_batch_plan, min_points 2 vfh_batch_plan; their outputs, written down ---------------------
static size_t test_plan() {
    const std::vector<size_t> sizes[2] = {{0, 0, 5, 0, 0, 64, 65, 0}, {0, 1, 2, 3, 499, 500, 501}};
    const std::vector<size_t> src[2] = {{0, 0, 0, 5, 5, 5, 69, 134, 134}, {0, 0, 1, 3, 6, 505, 1005, 1506}};
    struct Case {
        int set;
        size_t limit, min_points;
        std::vector<size_t> small_n, bases;
        size_t n_brute, n_large, n_items;
    };
    const Case cases[] = {
        {0, 0, 0, {0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0, 0}, 0, 134, 0},
        {0, 0, 2, {0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0, 0}, 0, 134, 0},
        {0, 64, 0, {0, 0, 5, 0, 0, 64, 0, 0}, {0, 0, 0, 5, 5, 5, 69, 69, 69}, 69, 65, 18},
        {0, 64, 2, {0, 0, 5, 0, 0, 64, 0, 0}, {0, 0, 0, 5, 5, 5, 69, 69, 69}, 69, 65, 18},
        {0, 500, 0, {0, 0, 5, 0, 0, 64, 65, 0}, {0, 0, 0, 5, 5, 5, 69, 134, 134}, 134, 0, 35},
        {0, 500, 2, {0, 0, 5, 0, 0, 64, 65, 0}, {0, 0, 0, 5, 5, 5, 69, 134, 134}, 134, 0, 35},
        {1, 0, 0, {0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}, 0, 1506, 0},
        {1, 0, 2, {0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}, 0, 1505, 0},
        {1, 64, 0, {0, 1, 2, 3, 0, 0, 0}, {0, 0, 1, 3, 6, 6, 6, 6}, 6, 1500, 3},
        {1, 64, 2, {0, 0, 2, 3, 0, 0, 0}, {0, 0, 0, 2, 5, 5, 5, 5}, 5, 1500, 2},
        {1, 500, 0, {0, 1, 2, 3, 499, 500, 0}, {0, 0, 1, 3, 6, 505, 1005, 1005}, 1005, 501, 253},
        {1, 500, 2, {0, 0, 2, 3, 499, 500, 0}, {0, 0, 0, 2, 5, 504, 1004, 1004}, 1004, 501, 252},
    };
    size_t n = 0;
    for (const Case& k : cases) {
        const std::vector<size_t>& sz = sizes[k.set];
        const std::vector<size_t> off = offsets_of(sz, 7);
        const RangeBatchPlan p = range_batch_plan(off.data(), sz.size(), k.min_points, k.limit);
        const char* what = "set %d, limit %zu, min_points %zu: %s";
        CHECK(same(p.n, sz), what, k.set, k.limit, k.min_points, "n");
        CHECK(same(p.small_n, k.small_n), what, k.set, k.limit, k.min_points, "small_n");
        CHECK(same(p.src, src[k.set]), what, k.set, k.limit, k.min_points, "src");
        CHECK(same(p.bases, k.bases), what, k.set, k.limit, k.min_points, "bases");
        CHECK(p.n_brute == k.n_brute && p.n_large == k.n_large && p.items.size() == k.n_items && p.total() == k.n_brute, what, k.set, k.limit,
              k.min_points, "the points per route, or the items");
        for (size_t c = 0; c < sz.size(); ++c) {
            // below min_points: neither route; above the limit: the work handle; else the batch route (an empty cluster too)
            const bool large = sz[c] >= k.min_points && sz[c] > k.limit;
            CHECK(p.on_work_handle(c) == large, "set %d, limit %zu, min_points %zu: cluster %zu is on the wrong route", k.set, k.limit, k.min_points, c);
        }
        if (k.min_points == VFH_MIN_POINTS) {  // the plan VFH builds on it is the same plan
            const VfhBatchPlan v = vfh_batch_plan(off.data(), sz.size(), k.limit);
            CHECK(same(v.small_n, k.small_n) && same(v.bases, k.bases) && v.n_brute == k.n_brute && v.n_large == k.n_large, what, k.set, k.limit,
                  k.min_points, "vfh_batch_plan differs");
        }
        ++n;
    }
    const size_t none[] = {3};
    const RangeBatchPlan e = range_batch_plan(none, 0, 0, 8192);
    CHECK(e.n.empty() && e.src.size() == 1 && e.src[0] == 0 && e.bases.size() == 1 && e.total() == 0, "no cluster at all");
    return n + 1;
}

// ---- the uploads: 3 clusters of 2, 65 and 0 points, the first record at 7 ------------------------------------------------------
// (recorded: align_up by hand around sizeof(GridDev) = 112 with n_valid at byte 52, 16-byte work and vote items, 16 bytes a point)
static const uint32_t FPFH_TABLES[108] = {
    0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 67u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 2u, 67u, 67u, 0u, 2u, 67u, 67u,
    0u, 2u, 0u, 2u, 2u, 65u, 0u, 4u, 2u, 65u, 4u, 4u, 2u, 65u, 8u, 4u, 2u, 65u, 12u, 4u, 2u, 65u, 16u, 4u, 2u, 65u, 20u, 4u, 2u, 65u, 24u, 4u, 2u, 65u,
    28u, 4u, 2u, 65u, 32u, 4u, 2u, 65u, 36u, 4u, 2u, 65u, 40u, 4u, 2u, 65u, 44u, 4u, 2u, 65u, 48u, 4u, 2u, 65u, 52u, 4u, 2u, 65u, 56u, 4u, 2u, 65u,
    60u, 4u, 2u, 65u, 64u, 1u};
static const uint32_t VFH_TABLES[140] = {
    0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 67u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 2u, 67u, 67u, 0u, 1u, 2u, 0u,
    1u, 0u, 0u, 0u, 0u, 0u, 2u, 0u, 1u, 2u, 65u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 2u, 67u, 67u, 0u, 2u, 0u, 2u,
    2u, 65u, 0u, 4u, 2u, 65u, 4u, 4u, 2u, 65u, 8u, 4u, 2u, 65u, 12u, 4u, 2u, 65u, 16u, 4u, 2u, 65u, 20u, 4u, 2u, 65u, 24u, 4u, 2u, 65u, 28u, 4u, 2u, 65u,
    32u, 4u, 2u, 65u, 36u, 4u, 2u, 65u, 40u, 4u, 2u, 65u, 44u, 4u, 2u, 65u, 48u, 4u, 2u, 65u, 52u, 4u, 2u, 65u, 56u, 4u, 2u, 65u, 60u, 4u, 2u, 65u,
    64u, 1u};

struct Records {  // 67 records of 32 bytes behind 7 others, x = the record's number
    std::vector<float> raw;
    std::vector<size_t> off;
    ClusterRanges ranges;
    explicit Records(const std::vector<size_t>& sizes) : raw((7 + 67) * 8, -3.0f), off(offsets_of(sizes, 7)) {
        for (size_t i = 0; i < 7 + 67; ++i) raw[i * 8] = (float)i;
        ranges = ClusterRanges{reinterpret_cast<const unsigned char*>(raw.data()), 32, off.data(), sizes.size(), 0};
    }
};

static void check_upload(const char* call, const RangeUpload& up, const Records& rec, const RangeBatchPlan& plan, bool refuse, const uint32_t* tables,
                         size_t pts_at, const std::vector<char>* extra_fill) {
    const size_t total = 67;
    CHECK(up.concat.pts_at == pts_at && up.bytes(false) == pts_at && up.bytes(true) == pts_at + total * 16 && up.device_bytes() == pts_at + total * 16,
          "%s upload: points at %zu, %zu bytes from device memory, %zu from host memory, %zu on the device", call, up.concat.pts_at, up.bytes(false),
          up.bytes(true), up.device_bytes());
    for (const bool host : {false, true}) {
        std::vector<char> u(up.bytes(true) + 16, (char)0x77);
        size_t bad = 99;
        CHECK(up.fill(u.data(), rec.ranges, plan, host, refuse, &bad) && bad == 99, "%s upload: finite points are refused", call);
        if (extra_fill) memcpy(up.extra(u.data()), extra_fill->data(), extra_fill->size());
        CHECK(memcmp(u.data(), tables, pts_at) == 0, "%s upload (host %d): the tables differ from the recorded bytes", call, (int)host);
        const size_t end = up.bytes(host);
        for (size_t i = end; i < u.size(); ++i)
            if (u[i] != (char)0x77) { CHECK(false, "%s upload (host %d): byte %zu behind the upload was written", call, (int)host, i); break; }
        if (!host) continue;
        const float* p4 = up.pts(static_cast<const char*>(u.data()));
        for (size_t at = 0; at < total; ++at) {
            uint32_t w;
            memcpy(&w, p4 + at * 4 + 3, 4);
            CHECK(p4[at * 4] == (float)(7 + at) && p4[at * 4 + 1] == -3.0f && p4[at * 4 + 2] == -3.0f && w == at, "%s upload: point %zu of the pack", call, at);
        }
    }
}

static void test_uploads() {
    const Records rec({2, 65, 0});
    {
        const RangeBatchPlan plan = range_batch_plan(rec.off.data(), 3, 0, 8192);
        const RangeUpload up(plan, 0);
        CHECK(RangeUpload::extra_start(3) == 128 && up.extra_at == 128 && up.concat.bases_at == 128 && up.concat.items_at == 144,
              "fpfh upload: %zu %zu %zu", up.extra_at, up.concat.bases_at, up.concat.items_at);
        check_upload("fpfh", up, rec, plan, false, FPFH_TABLES, 432, nullptr);
    }
    {
        const VfhBatchPlan plan = vfh_batch_plan(rec.off.data(), 3, 8192);
        const VfhUploadExtra extra(plan, RangeUpload::extra_start(3));
        const RangeUpload up(plan, extra.bytes);
        // row at 128, route at 140, vote items at 160 (the next 16-byte boundary), the header ends at 192
        CHECK(up.extra_at == 128 && extra.route_at == 12 && extra.votes_at == 32 && extra.bytes == 64 && up.concat.bases_at == 256 &&
                  up.concat.items_at == 272,
              "vfh upload: %zu %zu %zu %zu %zu %zu", up.extra_at, extra.route_at, extra.votes_at, extra.bytes, up.concat.bases_at, up.concat.items_at);
        std::vector<char> e(extra.bytes, 0);
        extra.fill(e.data(), plan);
        check_upload("vfh", up, rec, plan, true, VFH_TABLES, 560, &e);
        // the same offsets carve the device copy
        const char* d = reinterpret_cast<const char*>(VFH_TABLES);
        CHECK(up.src(d)[1] == 2 && up.bases(d)[3] == 67 && up.items(d)[17].q0 == 64 && extra.row(up.extra(d))[2] == 2 && extra.route(up.extra(d))[1] == 1 &&
                  extra.votes(up.extra(d))[1].count == 65,
              "the accessors over a base pointer");
    }
}

// ---- the host pack ----------------------------------------------------------------------------------------------------------------
static void test_pack() {
    // clusters of 3, 1, 4, 70 and 5 points; limit 64 and min_points 2: cluster 1 is on neither route, cluster 3 on the work handle
    Records rec({3, 1, 4, 70, 5});
    rec.raw.resize((7 + 83) * 8, -3.0f);
    rec.ranges.pts = reinterpret_cast<const unsigned char*>(rec.raw.data());
    const RangeBatchPlan plan = range_batch_plan(rec.off.data(), 5, 2, 64);
    const size_t total = plan.total();
    CHECK(total == 12, "the batch route holds %zu points", total);
    auto record = [&](size_t c, size_t i) { return &rec.raw[(rec.off[c] + i) * 8]; };
    auto run = [&](bool refuse, size_t* bad, std::vector<float>* p4) {
        p4->assign(total * 4 + 4, -7.0f);
        const bool ok = pack_ranges(rec.ranges, plan, refuse, p4->data(), bad);
        CHECK((*p4)[total * 4] == -7.0f, "the pack wrote past the concatenation");
        return ok;
    };
    std::vector<float> p4;
    size_t bad = 99;
    // off the route: a non-finite point in the cluster of 1 point and in the cluster above the limit is not seen
    record(1, 0)[0] = NAN;
    record(3, 69)[2] = INFINITY;
    CHECK(run(true, &bad, &p4) && bad == 99, "a non-finite point off the batch route refuses the pack (cluster %zu)", bad);
    // on the route: the clusters are taken in ascending order, so the lowest offender is named; with the switch off the raw
    // coordinates are staged
    record(4, 0)[1] = -INFINITY;
    record(2, 3)[0] = NAN;
    CHECK(!run(true, &bad, &p4) && bad == 2, "the first offender is cluster %zu, not the lowest on the route", bad);
    bad = 99;
    CHECK(run(false, &bad, &p4) && bad == 99, "the pack refuses with its switch off");
    uint32_t w;
    memcpy(&w, &p4[6 * 4 + 3], 4);
    CHECK(std::isnan(p4[6 * 4]) && w == 6 && p4[7 * 4 + 1] == -INFINITY, "raw coordinates are not staged as they are");
    record(2, 3)[0] = 1.0f;
    CHECK(!run(true, &bad, &p4) && bad == 4, "the offender is cluster %zu, not 4", bad);
}

// ---- the offsets --------------------------------------------------------------------------------------------------------------------
static void test_offsets() {
    const size_t big = (size_t)1 << 31;
    const size_t good[] = {3, 3, 8}, dec[] = {0, 5, 4, 9}, over[] = {10, 10 + big}, at_limit[] = {10, 10 + big - 1}, both[] = {0, big, big - 1};
    size_t bad = 99;
    CHECK(check_range_offsets(good, 2) == RANGE_OFFSETS_OK && check_range_offsets(at_limit, 1) == RANGE_OFFSETS_OK, "good offsets are refused");
    CHECK(check_range_offsets(dec, 3, &bad) == RANGE_OFFSETS_DECREASE && bad == 1, "a decrease is not refused at its cluster (%zu)", bad);
    CHECK(check_range_offsets(over, 1) == RANGE_OFFSETS_TOO_MANY, "2^31 points are not refused");
    CHECK(check_range_offsets(both, 2) == RANGE_OFFSETS_DECREASE, "a decrease does not come before the size");
    CHECK(check_range_offsets(dec, 0) == RANGE_OFFSETS_OK, "no cluster: nothing to refuse");
    // two scenes: a decrease in scene 2 wins over a size fault in scene 1
    int side = 0;
    bad = 99;
    CHECK(check_scene_offsets({{over, 1}, {dec, 3}}, &side, &bad) == RANGE_OFFSETS_DECREASE && side == 2 && bad == 1, "scene %d, cluster %zu", side, bad);
    CHECK(check_scene_offsets({{good, 2}, {over, 1}}, &side, &bad) == RANGE_OFFSETS_TOO_MANY && side == 2, "the size fault of scene 2 (scene %d)", side);
    CHECK(check_scene_offsets({{over, 1}, {good, 2}}, &side, &bad) == RANGE_OFFSETS_TOO_MANY && side == 1, "the size fault of scene 1 (scene %d)", side);
    CHECK(check_scene_offsets({{dec, 3}, {dec, 3}}, &side, &bad) == RANGE_OFFSETS_DECREASE && side == 1, "the first scene's decrease (scene %d)", side);
    CHECK(check_scene_offsets({{good, 2}, {dec, 0}}, &side, &bad) == RANGE_OFFSETS_OK, "two good scenes are refused");
    CHECK(check_scene_offsets({{good, 2}}, &side, &bad) == RANGE_OFFSETS_OK, "one good scene is refused");
}

int main() {
    const size_t plans = test_plan();
    test_uploads();
    test_pack();
    test_offsets();
    if (failures) {
        std::printf("range batch plan: %d failures\n", failures);
        return 1;
    }
    std::printf("range batch plan ok: %zu plans, 2 upload layouts from host and device memory, the host pack, the offsets of 1 and 2 scenes\n", plans);
    return 0;
}
