// test_voxel_plan.cpp -- csrc/voxel_plan.hpp on the CPU (no library, no GPU): the leaf lattice of a bounding box
//   1. ordinary boxes, both signs, against numbers written out by hand
//   2. the 2^26 rule on both sides of its edge
//   3. bounds at 2^24 and at 2^31 -/+ one float step: the last lattice an int holds, the first it does not
//   4. products that are Inf or NaN, an infinite inverse from a subnormal leaf, an infinite leaf (one voxel)
//   5. random boxes against 64-bit integer arithmetic
// Built plain and with -fsanitize=address,undefined,float-cast-overflow: no conversion here may be one an int cannot hold.
#include "voxel_plan.hpp"

#include <cmath>
#include <cstdio>
#include <limits>
#include <random>

using namespace pcc;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static VoxelPlan plan(float l0, float l1, float l2, float h0, float h1, float h2, float inv) {
    const float lo[3] = {l0, l1, l2}, hi[3] = {h0, h1, h2};
    return voxel_plan(lo, hi, inv);
}
// one axis under test, the other two a single voxel at the origin
static VoxelPlan axis(float lo, float hi, float inv) { return plan(lo, 0.f, 0.f, hi, 0.f, 0.f, inv); }

static void test_ordinary() {
    VoxelPlan p = plan(0.f, 0.f, 0.f, 1.f, 2.f, 3.f, 10.f);
    CHECK(p.verdict == VOXEL_PLAN_OK && p.cells == 7161.0);
    CHECK(p.org[0] == 0.f && p.org[1] == 0.f && p.org[2] == 0.f && p.dim[0] == 11 && p.dim[1] == 21 && p.dim[2] == 31);
    // both signs: -1.05 * 4 = -4.2 -> -5, 1.05 * 4 = 4.2 -> 4; -0.5 * 4 = -2 (on a face) -> -2; an all-negative axis
    p = plan(-1.05f, -0.5f, -3.f, 1.05f, 0.5f, -2.f, 4.f);
    CHECK(p.verdict == VOXEL_PLAN_OK && p.cells == 250.0);
    CHECK(p.org[0] == -5.f && p.org[1] == -2.f && p.org[2] == -12.f && p.dim[0] == 10 && p.dim[1] == 5 && p.dim[2] == 5);
    // a single point; -0.0 is voxel 0
    p = plan(0.3f, -7.25f, -0.f, 0.3f, -7.25f, -0.f, 40.f);
    CHECK(p.verdict == VOXEL_PLAN_OK && p.cells == 1.0 && p.org[0] == 12.f && p.org[1] == -290.f && p.org[2] == 0.f);
    CHECK(p.dim[0] == 1 && p.dim[1] == 1 && p.dim[2] == 1);
    // a geo-referenced box: 1e5 * 4 = 400000
    p = plan(1000.f, 1e5f, -1e5f, 1003.984375f, 100003.984375f, -99996.015625f, 4.f);
    CHECK(p.verdict == VOXEL_PLAN_OK && p.org[0] == 4000.f && p.org[1] == 400000.f && p.org[2] == -400000.f);
    CHECK(p.dim[0] == 16 && p.dim[1] == 16 && p.dim[2] == 16 && p.cells == 4096.0);
}

static void test_cell_limit() {
    VoxelPlan p = plan(0.f, 0.f, 0.f, 1023.f, 1023.f, 63.f, 1.f);
    CHECK(p.verdict == VOXEL_PLAN_OK && p.cells == 67108864.0 && p.dim[0] == 1024 && p.dim[1] == 1024 && p.dim[2] == 64);
    p = plan(0.f, 0.f, 0.f, 1023.f, 1023.f, 64.f, 1.f);
    CHECK(p.verdict == VOXEL_PLAN_CELLS && p.cells == 1024.0 * 1024.0 * 65.0);
    p = axis(-3.f, 67108860.f, 1.f);  // (floats are 4 apart below 2^26)
    CHECK(p.verdict == VOXEL_PLAN_OK && p.org[0] == -3.f && p.dim[0] == 67108864 && p.cells == 67108864.0);
    p = axis(-4.f, 67108860.f, 1.f);
    CHECK(p.verdict == VOXEL_PLAN_CELLS && p.cells == 67108865.0);
}

static void test_int_edges() {
    const float two24 = 16777216.f, below31 = 2147483520.f /* 2^31 - 128 */, two31 = 2147483648.f, above31 = 2147483904.f /* 2^31 + 256 */;
    CHECK(std::nextafterf(two31, 0.f) == below31 && std::nextafterf(two31, INFINITY) == above31);
    VoxelPlan p = axis(two24, two24, 1.f);
    CHECK(p.verdict == VOXEL_PLAN_OK && p.org[0] == two24 && p.dim[0] == 1);
    p = axis(two24, two24 + 2.f, 1.f);  // (the float after 2^24)
    CHECK(p.verdict == VOXEL_PLAN_OK && p.org[0] == two24 && p.dim[0] == 3);
    p = axis(-two24 - 2.f, -two24, 1.f);
    CHECK(p.verdict == VOXEL_PLAN_OK && p.org[0] == -16777218.f && p.dim[0] == 3);
    p = axis(below31, below31, 1.f);
    CHECK(p.verdict == VOXEL_PLAN_OK && p.org[0] == below31 && p.dim[0] == 1 && p.cells == 1.0);
    p = axis(-below31, -below31, 1.f);
    CHECK(p.verdict == VOXEL_PLAN_OK && p.org[0] == -below31 && p.dim[0] == 1);
    p = axis(std::nextafterf(below31, 0.f), below31, 1.f);
    CHECK(p.verdict == VOXEL_PLAN_OK && p.dim[0] == 129);
    for (float edge : {two31, above31, 3e9f, 3e38f}) {
        CHECK(axis(edge, edge, 1.f).verdict == VOXEL_PLAN_RANGE);
        CHECK(axis(-edge, -edge, 1.f).verdict == VOXEL_PLAN_RANGE);
        CHECK(axis(0.f, edge, 1.f).verdict == VOXEL_PLAN_RANGE);      // only the upper bound
        CHECK(axis(-edge, 0.f, 1.f).verdict == VOXEL_PLAN_RANGE);     // only the lower bound
        CHECK(plan(0.f, 0.f, -edge, 0.f, 0.f, 0.f, 1.f).verdict == VOXEL_PLAN_RANGE);  // the last axis
    }
    // the whole range of an int along one axis: every bound converts, the count does not fit an int and is not converted
    p = axis(-below31, below31, 1.f);
    CHECK(p.verdict == VOXEL_PLAN_CELLS && p.cells == 4294967041.0);
    p = plan(-below31, -below31, -below31, below31, below31, below31, 1.f);
    CHECK(p.verdict == VOXEL_PLAN_CELLS && p.cells > 7.9e28);
    // reached through the product: x in [3000, 3000.001] at a leaf of 1e-6 is voxel 3e9; its mirror image
    const float inv6 = 1.0f / 1e-6f;
    CHECK(plan(3000.f, 0.f, 0.f, 3000.001f, 1e-4f, 1e-4f, inv6).verdict == VOXEL_PLAN_RANGE);
    CHECK(plan(-3000.001f, 0.f, 0.f, -3000.f, 1e-4f, 1e-4f, inv6).verdict == VOXEL_PLAN_RANGE);
    p = plan(2000.f, 0.f, 0.f, 2000.00001f, 1e-4f, 1e-4f, inv6);  // 2e9 is below 2^31
    CHECK(p.verdict == VOXEL_PLAN_OK && p.org[0] == std::floor(2000.f * inv6) && p.dim[1] == 101 && p.dim[2] == 101);
}

static void test_not_finite() {
    const float inf = std::numeric_limits<float>::infinity();
    CHECK(axis(1e30f, 1e30f, 1e30f).verdict == VOXEL_PLAN_RANGE);   // the product overflows
    CHECK(axis(-1e30f, 1.f, 1e30f).verdict == VOXEL_PLAN_RANGE);
    CHECK(axis(0.f, 0.f, inf).verdict == VOXEL_PLAN_RANGE);         // 0 * inf = NaN
    CHECK(axis(1.f, 2.f, inf).verdict == VOXEL_PLAN_RANGE);
    const float leaf = 1e-39f;                                      // subnormal: positive, its inverse is not finite
    CHECK(leaf > 0.f && std::fpclassify(leaf) == FP_SUBNORMAL && 1.0f / leaf == inf);
    CHECK(plan(0.f, 0.f, 0.f, 1.f, 1.f, 1.f, 1.0f / leaf).verdict == VOXEL_PLAN_RANGE);
    CHECK(plan(-1.f, 1.f, 2.f, -0.5f, 1.f, 2.f, 1.0f / leaf).verdict == VOXEL_PLAN_RANGE);
    // an infinite leaf: the inverse is 0, every point is in voxel (0, 0, 0)
    const VoxelPlan p = plan(-3e38f, -1.f, 0.f, 3e38f, 5.f, 1e20f, 1.0f / inf);
    CHECK(p.verdict == VOXEL_PLAN_OK && p.cells == 1.0 && p.dim[0] == 1 && p.dim[1] == 1 && p.dim[2] == 1);
    CHECK(p.org[0] == 0.f && p.org[1] == 0.f && p.org[2] == 0.f);
}

static void test_random() {
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> mag(-12.f, 12.f), unit(-1.f, 1.f);
    int ok = 0, range = 0, cells = 0;
    for (int it = 0; it < 200000; ++it) {
        float lo[3], hi[3];
        for (int a = 0; a < 3; ++a) {
            const float c = unit(rng) * std::exp2(mag(rng)), e = std::fabs(unit(rng)) * std::exp2(mag(rng) - 4.f);
            lo[a] = c - e;
            hi[a] = c + e;
        }
        const float inv = 1.0f / std::exp2(mag(rng) * 2.f - 8.f);
        const VoxelPlan p = voxel_plan(lo, hi, inv);
        bool in_range = true;
        double want_cells = 1;
        long long mn[3], mx[3];
        for (int a = 0; a < 3; ++a) {
            const double fl = std::floor((double)(lo[a] * inv)), fh = std::floor((double)(hi[a] * inv));  // (float products)
            if (!(std::fabs(fl) < 2147483648.0) || !(std::fabs(fh) < 2147483648.0)) { in_range = false; break; }
            mn[a] = (long long)fl;
            mx[a] = (long long)fh;
            want_cells *= (double)(mx[a] - mn[a] + 1);
        }
        if (!in_range) { CHECK(p.verdict == VOXEL_PLAN_RANGE); ++range; continue; }
        CHECK(p.cells == want_cells);
        if (want_cells > 67108864.0) { CHECK(p.verdict == VOXEL_PLAN_CELLS); ++cells; continue; }
        CHECK(p.verdict == VOXEL_PLAN_OK);
        for (int a = 0; a < 3; ++a) CHECK(p.org[a] == (float)mn[a] && (long long)p.dim[a] == mx[a] - mn[a] + 1);
        ++ok;
    }
    CHECK(ok > 1000 && range > 1000 && cells > 1000);
    std::printf("random boxes: %d lattices, %d beyond int32, %d above 2^26 voxels\n", ok, range, cells);
}

int main() {
    test_ordinary();
    test_cell_limit();
    test_int_edges();
    test_not_finite();
    test_random();
    if (failures) { std::printf("test_voxel_plan: %d FAILED\n", failures); return 1; }
    std::printf("test_voxel_plan: ok\n");
    return 0;
}
