// test_match_fpfh_plan.cpp -- csrc/match_fpfh_plan.hpp on the CPU (no library, no GPU): the 36-float record of
// pcc_match_fpfh_batch, invalid records, the bytes read of a record, the table the pack from device memory is driven by.
//   1. packing: floats 0 .. 32 copied bit for bit, three +0 behind them; (+inf, 0, ...) for a record with a non-finite float among
//      its 33, bin 32 alone included; floats 33 and beyond of a wide record are never read (they hold NaN here)
//   2. of every record 132 bytes are read: the arrays here are heap blocks that END at the last record's 132 bytes, so that under
//      AddressSanitizer (make asan) one byte more is an error
//   3. the plan: the slice of a 36-float record, shared reference clouds laid out once, and the sources of the device pack -- no
//      empty one, first records ascending from 0, every packed record in exactly one
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "match_fpfh_plan.hpp"

static int failures = 0;
#define REQUIRE(c)                                                                  \
    do {                                                                            \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

static uint32_t bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

constexpr int DIM = pcc::MF_DIM, DP = pcc::MF_DP;

// n records of `stride` bytes in a block that ends after the last record's 132 bytes; record i, float k = value(i, k)
static char* tight_array(size_t n, size_t stride, float (*value)(size_t, int)) {
    const size_t bytes = n ? (n - 1) * stride + 4 * (size_t)DIM : 0;
    char* block = static_cast<char*>(std::malloc(bytes ? bytes : 1));
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (size_t i = 0; i < n; ++i)
        for (size_t k = 0; k < stride / 4; ++k) {
            if (i * stride + 4 * k + 4 > bytes) break;
            const float v = k < (size_t)DIM ? value(i, (int)k) : nan;  // (the unread tail of a record holds NaN)
            std::memcpy(block + i * stride + 4 * k, &v, 4);
        }
    return block;
}

static float plain_value(size_t i, int k) { return (float)(i * 37 + k) * 0.25f - 3.0f; }
static float first_bin_value(size_t i, int k) {
    if (i == 1 && k == 0) return std::numeric_limits<float>::quiet_NaN();
    if (i == 3) return k == 0 ? std::numeric_limits<float>::infinity() : 1.0f;
    return plain_value(i, k);
}
static float last_bin_value(size_t i, int k) {  // bin 32 is the only non-finite float of records 2, 5 and 6 (the last)
    if (i == 2 && k == DIM - 1) return -std::numeric_limits<float>::infinity();
    if (i == 5 && k == DIM - 1) return std::numeric_limits<float>::quiet_NaN();
    if (i == 6 && k == DIM - 1) return std::numeric_limits<float>::infinity();
    return plain_value(i, k);
}

static void test_pack() {
    const float inf = std::numeric_limits<float>::infinity();
    REQUIRE(DIM == 33 && DP == 36 && (DP * sizeof(float)) % 16 == 0);
    for (size_t stride : {(size_t)132, (size_t)136, (size_t)144, (size_t)256}) {
        const size_t n = 7;
        // every record valid: copied bit for bit, +0 in the padding; NaN behind float 32 is never seen
        char* a = tight_array(n, stride, plain_value);
        std::vector<float> out(n * DP, -1.f);
        REQUIRE(pcc::match_fpfh_pack(a, n, stride, out.data()) == n);
        for (size_t i = 0; i < n; ++i)
            for (int k = 0; k < DP; ++k) REQUIRE(bits(out[i * DP + k]) == bits(k < DIM ? plain_value(i, k) : 0.0f));
        std::free(a);
        // non-finite floats in bin 0, and in bin 32 alone
        for (int which = 0; which < 2; ++which) {
            float (*value)(size_t, int) = which ? last_bin_value : first_bin_value;
            a = tight_array(n, stride, value);
            std::fill(out.begin(), out.end(), -1.f);
            const size_t valid = pcc::match_fpfh_pack(a, n, stride, out.data());
            size_t want_valid = 0;
            for (size_t i = 0; i < n; ++i) {
                bool ok = true;
                for (int k = 0; k < DIM; ++k) ok = ok && std::isfinite(value(i, k));
                want_valid += ok;
                for (int k = 0; k < DP; ++k) {
                    const float want = !ok ? (k == 0 ? inf : 0.0f) : (k < DIM ? value(i, k) : 0.0f);
                    REQUIRE(bits(out[i * DP + k]) == bits(want));
                }
            }
            REQUIRE(valid == want_valid && valid == n - (which ? 3 : 2));
            std::free(a);
        }
    }
    // a single record in a block of exactly 132 bytes
    char* one = tight_array(1, 132, plain_value);
    float out1[DP];
    REQUIRE(pcc::match_fpfh_pack(one, 1, 132, out1) == 1 && bits(out1[32]) == bits(plain_value(0, 32)) && bits(out1[33]) == 0 && bits(out1[35]) == 0);
    std::free(one);
    REQUIRE(pcc::match_fpfh_pack(nullptr, 0, 132, nullptr) == 0);
}

static void test_plan_and_sources() {
    REQUIRE(pcc::match_dims_slice_max(DP) == 512);
    static char arena[64];
    // pairs 0 and 2 share a reference cloud (pointer AND length); pair 1 has no reference, pair 3 no query
    const void* des1[4] = {arena, arena + 8, arena, arena + 16};
    const void* des2[4] = {arena + 24, arena + 32, arena + 40, arena + 48};
    const size_t n1[4] = {700, 0, 700, 5}, n2[4] = {130, 9, 1, 0};
    pcc::MatchFpfhPlan pl;
    REQUIRE(pcc::match_fpfh_plan(4, des1, n1, n2, &pl));
    REQUIRE(pl.clouds.size() == 3 && pl.n_rec == 700 + 0 + 5 + 130 + 9 + 1 && pl.n_slots == 140);
    REQUIRE(pl.slice >= pcc::MATCH_SLICE_MIN && pl.slice <= 512);
    REQUIRE(pl.cloud_of[0] == pl.cloud_of[2] && pl.q_rec0[0] == 705 && pl.q_rec0[1] == 835 && pl.q_rec0[2] == 844);
    // items: pairs 0 (3 query blocks) and 2 (1) over ceil(700 / slice) slices each
    const size_t slices = (700 + pl.slice - 1) / pl.slice;
    REQUIRE(pl.items.size() == 4 * slices);
    for (const pcc::MatchItem& it : pl.items) {
        REQUIRE(it.r0 + it.nr <= 700 && it.nq >= 1 && it.nq <= 64 && it.q0 >= 705 && it.q0 + it.nq <= pl.n_rec);
        REQUIRE(it.qslot0 + it.nq <= pl.n_slots && it.ridx0 == it.r0);
    }
    std::vector<pcc::MatchFpfhSource> src;
    pcc::match_fpfh_sources(pl, 4, des2, n2, &src);
    REQUIRE(src.size() == 5);  // clouds of 700 and 5, queries of 130, 9 and 1: nothing empty
    size_t next = 0;
    for (const pcc::MatchFpfhSource& s : src) {
        REQUIRE(s.n > 0 && s.rec0 == next);
        next += s.n;
    }
    REQUIRE(next == pl.n_rec);
    REQUIRE(src[0].p == arena && src[1].p == arena + 16 && src[2].p == arena + 24 && src[3].p == arena + 32 && src[4].p == arena + 40);
    REQUIRE(sizeof(pcc::MatchFpfhSource) == 16);
    // nothing to search at all: no item, no source beyond the clouds that hold records
    const size_t z[4] = {0, 0, 0, 0};
    REQUIRE(pcc::match_fpfh_plan(4, des1, z, z, &pl) && pl.items.empty() && pl.n_rec == 0);
    pcc::match_fpfh_sources(pl, 4, des2, z, &src);
    REQUIRE(src.empty());
    // 2^31 records and more are refused
    const size_t big1[2] = {(size_t)1 << 30, (size_t)1 << 30}, small2[2] = {1, 1};
    REQUIRE(!pcc::match_fpfh_plan(2, des1, big1, small2, &pl));
}

int main() {
    test_pack();
    test_plan_and_sources();
    if (failures) { std::printf("test_match_fpfh_plan: %d FAILED\n", failures); return 1; }
    std::printf("test_match_fpfh_plan: ok\n");
    return 0;
}
