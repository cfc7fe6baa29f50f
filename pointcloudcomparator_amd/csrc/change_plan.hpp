// change_plan.hpp -- the voxel lattice of pcl::octree::OctreePointCloudChangeDetector as pcc_change_detection restates it: the
// anchor from the first point that takes part, the voxel coordinate of a value with its range verdict, the span verdict and key
// packing, and the size of the occupancy table.  One set of functions for the host and the device (change.hip).  Plain C++ (no
// HIP needed: tests/cpp/test_change_plan.cpp compiles it on its own).
//
// PCL (octree_pointcloud.hpp, adoptBoundingBoxToPoint): the first point p makes a box of side 2 * res - eps centred on p (eps =
// FLT_EPSILON); every later point outside the box doubles it in whole multiples of res, away from the violated side.  So the
// LATTICE is fixed by p alone: a voxel is floor((x - a) / res) with a = the first box's minimum, whatever the box became.
// The conversion of a coordinate to an integer is defined only below 2^31 in magnitude here (PCL's own keys are 32 bits per axis):
// that is decided in floating point, BEFORE any conversion, as in voxel_plan.hpp.  Everything is IEEE double: subtraction, then
// division -- no reciprocal, no contraction (the library and the tests are built with -ffp-contract=off).
#pragma once
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PCC_CHANGE_HD __host__ __device__
#else
#define PCC_CHANGE_HD
#endif

namespace pcc {

// PCL's octree keys take 2^32 voxels per axis; this library packs three coordinates into one 64-bit key and draws the line at 2^21
constexpr int CHANGE_AXIS_BITS = 21;
constexpr uint64_t CHANGE_MAX_SPAN = 1ull << CHANGE_AXIS_BITS;
constexpr uint64_t CHANGE_EMPTY_KEY = ~0ull;  // (a packed key has bit 63 clear)
constexpr size_t CHANGE_MIN_SLOTS = 64;

// the minimum corner, along one axis, of PCL's first box around p
PCC_CHANGE_HD inline double change_anchor(float p, double res) {
    const double eps = (double)FLT_EPSILON;
    const double mn = (double)p - res / 2;
    const double mx = (double)p + res / 2;
    const double side = 2 * res - eps;
    const double over = (side - (mx - mn)) / 2;
    return mn - over;
}

// the voxel coordinate of x along an axis anchored at a: *k = floor((x - a) / res).  false (and *k untouched) when the quotient
// is not below 2^31 in magnitude -- Inf and NaN included: nothing is converted then
PCC_CHANGE_HD inline bool change_coord(float x, double a, double res, int64_t* k) {
    const double q = ((double)x - a) / res;
    if (!(fabs(q) < 2147483648.0)) return false;
    *k = (int64_t)floor(q);  // in [-2^31, 2^31)
    return true;
}

// the number of voxels an axis spans, mn <= mx both from change_coord (at most 2^32), and whether a key has room for it
PCC_CHANGE_HD inline uint64_t change_span(int64_t mn, int64_t mx) { return (uint64_t)(mx - mn) + 1u; }
PCC_CHANGE_HD inline bool change_span_ok(int64_t mn, int64_t mx) { return change_span(mn, mx) <= CHANGE_MAX_SPAN; }

// three coordinates, each in [mn, mn + 2^21) along its axis, in one key: x in bits 0-20, y in 21-41, z in 42-62
PCC_CHANGE_HD inline uint64_t change_key(const int64_t k[3], const int64_t mn[3]) {
    return (uint64_t)(k[0] - mn[0]) | ((uint64_t)(k[1] - mn[1]) << CHANGE_AXIS_BITS) | ((uint64_t)(k[2] - mn[2]) << (2 * CHANGE_AXIS_BITS));
}

// the table slot a key starts probing at: a mixer of all 64 bits (splitmix64's finaliser) -- lattice-aligned clouds give keys
// that differ in a few high bits only.  slots is a power of two
PCC_CHANGE_HD inline uint64_t change_hash(uint64_t key, uint64_t slots) {
    key ^= key >> 30; key *= 0xbf58476d1ce4e5b9ull;
    key ^= key >> 27; key *= 0x94d049bb133111ebull;
    key ^= key >> 31;
    return key & (slots - 1);
}

// slots of the occupancy table for `points` points (both clouds together, up to 2^32 - 2): the power of two that is at least
// twice the points and at least CHANGE_MIN_SLOTS
PCC_CHANGE_HD inline uint64_t change_table_slots(uint64_t points) {
    uint64_t s = CHANGE_MIN_SLOTS;
    while (s < 2 * points) s <<= 1;
    return s;
}

}  // namespace pcc
