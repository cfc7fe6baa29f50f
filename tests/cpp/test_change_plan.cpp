// test_change_plan.cpp -- csrc/change_plan.hpp on the CPU (no library, no GPU): the voxel lattice of pcc_change_detection
//   1. the anchor arithmetic against numbers written out by hand, and where it stops being finite
//   2. floor on exact voxel faces and one float step below them, negative coordinates, dyadic values against integers
//   3. the 2^31 range verdict on both sides of its edge, Inf-producing inputs included
//   4. the 2^21 span verdict and the key packing at the corners of its range
//   5. the table size (0 and 2^31 points included) and the spread of the hash over lattice-aligned keys
// Built plain and with -fsanitize=address,undefined,float-cast-overflow: no conversion here may be one an integer cannot hold.
#include "change_plan.hpp"

#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <set>
#include <tuple>

using namespace pcc;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static const double EPS = (double)FLT_EPSILON;  // 2^-23

static void test_anchor() {
    // p = 0, res = 1: mn = -0.5, mx = 0.5, side = 2 - eps, over = 0.5 - eps/2, a = -1 + eps/2
    CHECK(change_anchor(0.f, 1.0) == -1.0 + EPS / 2);
    // p = 1.5, res = 0.25: mn = 1.375, mx = 1.625, side = 0.5 - eps, over = 0.125 - eps/2, a = 1.25 + eps/2
    CHECK(change_anchor(1.5f, 0.25) == 1.25 + EPS / 2);
    CHECK(change_anchor(-1.5f, 0.25) == -1.75 + EPS / 2);
    // a large resolution: mn = 0, mx = 32, side = 64 - eps, over = 16 - eps/2 (still exact: 16 - 2^-24 has 28 bits)
    CHECK(change_anchor(16.f, 32.0) == -16.0 + EPS / 2);
    // the point itself lies in voxel 0, just below the face to voxel 1: the first box is centred on it
    for (double res : {0.03, 0.1, 0.125, 0.25, 0.5, 32.0}) {
        for (float p : {0.f, 1.f, -1.f, 0.37f, -123.456f, 49.99f}) {
            int64_t k = 99;
            CHECK(change_coord(p, change_anchor(p, res), res, &k) && k == 0);
        }
    }
    // the operations in their order, not an algebraic short cut: a rounding of mx - mn shows in the result
    {
        const float p = 0.1f;
        const double res = 0.03, mn = (double)p - res / 2, mx = (double)p + res / 2, side = 2 * res - EPS;
        CHECK(change_anchor(p, res) == mn - (side - (mx - mn)) / 2);
    }
    // 2 * res overflows: the anchor is -Inf and no coordinate passes
    const double a = change_anchor(1.f, 1.7e308);
    int64_t k = 7;
    CHECK(std::isinf(a) && a < 0 && !change_coord(1.f, a, 1.7e308, &k) && k == 7);
    // the smallest subnormal resolution: res / 2 is 0, the side is negative, the point's own quotient is -Inf
    const double tiny = std::numeric_limits<double>::denorm_min();
    CHECK(change_anchor(2.f, tiny) == 2.0 + EPS / 2 && !change_coord(2.f, change_anchor(2.f, tiny), tiny, &k) && k == 7);
}

static void test_faces() {
    int64_t k = 0;
    // a = 0, res = 0.25: 0.75 is the face between voxels 2 and 3
    CHECK(change_coord(0.75f, 0.0, 0.25, &k) && k == 3);
    CHECK(change_coord(std::nextafterf(0.75f, 0.f), 0.0, 0.25, &k) && k == 2);
    CHECK(change_coord(0.f, 0.0, 0.25, &k) && k == 0);
    CHECK(change_coord(-0.f, 0.0, 0.25, &k) && k == 0);
    CHECK(change_coord(-std::numeric_limits<float>::denorm_min(), 0.0, 0.25, &k) && k == -1);
    CHECK(change_coord(-0.5f, 0.0, 0.25, &k) && k == -2);
    CHECK(change_coord(std::nextafterf(-0.5f, -1.f), 0.0, 0.25, &k) && k == -3);
    CHECK(change_coord(-0.3f, 0.0, 0.25, &k) && k == -2);
    // PCL's own anchor: p = 0, res = 1 puts the faces at integers + 2^-24, which floats hold around 0
    const double a = change_anchor(0.f, 1.0);
    const float face0 = -1.f + (float)(EPS / 2), face1 = (float)(EPS / 2);
    CHECK((double)face0 == a && (double)face1 == a + 1.0);
    CHECK(change_coord(face0, a, 1.0, &k) && k == 0);
    CHECK(change_coord(std::nextafterf(face0, -2.f), a, 1.0, &k) && k == -1);  // (-1 exactly)
    CHECK(change_coord(face1, a, 1.0, &k) && k == 1);
    CHECK(change_coord(std::nextafterf(face1, -1.f), a, 1.0, &k) && k == 0);
    CHECK(change_coord(0.f, a, 1.0, &k) && k == 0);
    // dyadic values: x = m / 8, a = j / 8, res = 1 / 8 -> k = m - j, whatever the signs
    std::mt19937 rng(11);
    std::uniform_int_distribution<int> d(-1000000, 1000000);
    for (int it = 0; it < 200000; ++it) {
        const int m = d(rng), j = d(rng);
        CHECK(change_coord((float)m / 8.f, (double)j / 8.0, 0.125, &k) && k == (int64_t)m - j);
    }
}

static void test_range() {
    const float below31 = 2147483520.f /* 2^31 - 128 */, two31 = 2147483648.f;
    int64_t k = 7;
    CHECK(change_coord(below31, 0.0, 1.0, &k) && k == 2147483520ll);
    CHECK(change_coord(-below31, 0.0, 1.0, &k) && k == -2147483520ll);
    k = 7;
    CHECK(!change_coord(two31, 0.0, 1.0, &k) && !change_coord(-two31, 0.0, 1.0, &k) && k == 7);  // "below 2^31 in magnitude"
    CHECK(!change_coord(3e9f, 0.0, 1.0, &k) && !change_coord(-3e38f, 0.0, 1.0, &k) && k == 7);
    // just inside through the anchor: the quotient, not the coordinate, is what is tested
    CHECK(change_coord(below31, -127.5, 1.0, &k) && k == 2147483647ll);
    CHECK(!change_coord(below31, -128.0, 1.0, &k));
    CHECK(change_coord(-below31, 127.5, 1.0, &k) && k == -2147483648ll);  // floor(-(2^31 - 0.5))
    CHECK(!change_coord(-below31, 128.0, 1.0, &k));
    // the issue's refusal: coordinates 10^9 apart at a resolution of 0.01
    CHECK(!change_coord(1e9f, 0.0, 0.01, &k) && change_coord(1e7f, 0.0, 0.01, &k) && k == 1000000000ll);
    // quotients that are Inf: the division overflows, the anchor is infinite
    k = 7;
    CHECK(!change_coord(3e38f, 0.0, 1e-300, &k) && !change_coord(-3e38f, 0.0, 1e-300, &k));
    CHECK(!change_coord(1.f, 0.0, std::numeric_limits<double>::denorm_min(), &k));
    CHECK(!change_coord(1.f, -INFINITY, 1.0, &k) && !change_coord(1.f, INFINITY, 1.0, &k) && k == 7);
    CHECK(!change_coord(1.f, std::nan(""), 1.0, &k) && k == 7);
    // ... and one that is 0 / tiny = 0
    CHECK(change_coord(0.f, 0.0, std::numeric_limits<double>::denorm_min(), &k) && k == 0);
}

static void test_span_and_keys() {
    const int64_t full = (int64_t)CHANGE_MAX_SPAN;  // 2^21
    CHECK(change_span(0, 0) == 1 && change_span_ok(0, 0));
    CHECK(change_span(0, full - 1) == CHANGE_MAX_SPAN && change_span_ok(0, full - 1));
    CHECK(change_span(0, full) == CHANGE_MAX_SPAN + 1 && !change_span_ok(0, full));
    CHECK(change_span_ok(-5, full - 6) && !change_span_ok(-5, full - 5));
    CHECK(change_span_ok(-full / 2, full / 2 - 1) && !change_span_ok(-full / 2, full / 2));
    // the whole range change_coord lets through: 2^32 voxels, counted without overflow
    CHECK(change_span(-2147483648ll, 2147483647ll) == 4294967296ull && !change_span_ok(-2147483648ll, 2147483647ll));
    CHECK(change_span_ok(2147483647ll - (full - 1), 2147483647ll) && change_span_ok(-2147483648ll, -2147483648ll + full - 1));
    // keys: x in bits 0-20, y in 21-41, z in 42-62, relative to the minimum; never the empty key
    const int64_t mn[3] = {-7, 2147483647ll - (full - 1), -2147483648ll};
    const int64_t lo[3] = {mn[0], mn[1], mn[2]}, hi[3] = {mn[0] + full - 1, mn[1] + full - 1, mn[2] + full - 1};
    CHECK(change_key(lo, mn) == 0ull);
    CHECK(change_key(hi, mn) == 0x7fffffffffffffffull && change_key(hi, mn) != CHANGE_EMPTY_KEY);
    const int64_t kx[3] = {mn[0] + 5, mn[1], mn[2]}, ky[3] = {mn[0], mn[1] + 5, mn[2]}, kz[3] = {mn[0], mn[1], mn[2] + 5};
    CHECK(change_key(kx, mn) == 5ull && change_key(ky, mn) == 5ull << 21 && change_key(kz, mn) == 5ull << 42);
    const int64_t kxm[3] = {hi[0], mn[1], mn[2]}, kym[3] = {mn[0], hi[1], mn[2]};
    CHECK(change_key(kxm, mn) == (1ull << 21) - 1 && change_key(kym, mn) == ((1ull << 21) - 1) << 21);
    // distinct coordinates, distinct keys
    std::mt19937_64 rng(5);
    std::set<uint64_t> seen;
    std::set<std::tuple<int64_t, int64_t, int64_t>> coords;
    for (int it = 0; it < 100000; ++it) {
        const int64_t k[3] = {mn[0] + (int64_t)(rng() % full), mn[1] + (int64_t)(rng() % 4), mn[2] + (int64_t)(rng() % full)};
        coords.insert({k[0], k[1], k[2]});
        seen.insert(change_key(k, mn));
    }
    CHECK(seen.size() == coords.size());
}

static void test_table() {
    CHECK(change_table_slots(0) == CHANGE_MIN_SLOTS && change_table_slots(1) == CHANGE_MIN_SLOTS && change_table_slots(32) == 64);
    CHECK(change_table_slots(33) == 128 && change_table_slots(64) == 128 && change_table_slots(65) == 256);
    CHECK(change_table_slots(3500) == 8192 && change_table_slots(4096) == 8192 && change_table_slots(4097) == 16384);
    CHECK(change_table_slots(1ull << 31) == 1ull << 32);
    CHECK(change_table_slots((1ull << 31) + 1) == 1ull << 33);
    CHECK(change_table_slots((1ull << 32) - 2) == 1ull << 33);  // two clouds of 2^31 - 1 points
    for (uint64_t n : {0ull, 1ull, 7ull, 100ull, 65535ull, 65536ull, 20000000ull, (1ull << 31) - 1}) {
        const uint64_t s = change_table_slots(n);
        CHECK((s & (s - 1)) == 0 && s >= 2 * n && s >= CHANGE_MIN_SLOTS && (s == CHANGE_MIN_SLOTS || s / 2 < 2 * n));
    }
    // the hash stays inside the table and spreads keys that differ in high bits only: 20 000 multiples of 1024 along x, the same
    // along z, into 65536 slots -- a hash of the low bits would put each set into 64 slots (x) or one (z)
    const uint64_t slots = 65536;
    for (int set = 0; set < 3; ++set) {  // along x; along z; along y and z
        std::set<uint64_t> used;
        for (uint64_t i = 0; i < 20000; ++i) {
            const uint64_t key = set == 0 ? i << 10 : (set == 1 ? i << 42 : ((i % 2048) << 31 | (i / 2048) << 52));
            const uint64_t h = change_hash(key, slots);
            CHECK(h < slots);
            used.insert(h);
        }
        // 20 000 random throws into 65536 slots fill about 17 200 of them
        CHECK(used.size() > 16000);
    }
    CHECK(change_hash(0, 64) < 64 && change_hash(0x7fffffffffffffffull, 64) < 64 && change_hash(12345, 1ull << 33) < (1ull << 33));
}

int main() {
    test_anchor();
    test_faces();
    test_range();
    test_span_and_keys();
    test_table();
    if (failures) { std::printf("test_change_plan: %d FAILED\n", failures); return 1; }
    std::printf("test_change_plan: ok\n");
    return 0;
}
