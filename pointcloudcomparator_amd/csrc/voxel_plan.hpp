// voxel_plan.hpp -- the leaf lattice of pcl::VoxelGrid from a cloud's finite bounding box: (lo, hi, inverse leaf) -> origin,
// dimensions, voxel count and a verdict.  One function for the host (voxel.hip, the check of pcc_sift_keypoints_batch) and the
// device (sift_batch.hip's k_sb_voxel_keys).  Plain C++ (no HIP needed: tests/cpp/test_voxel_plan.cpp compiles it on its own).
//
// PCL (pcl/filters/impl/voxel_grid.hpp): min_b = int(floor(min_p * inverse_leaf)), max_b likewise, div_b = max_b - min_b + 1;
// a point's voxel is int(floor(p * inverse_leaf) - float(min_b)), so org = float(min_b).  The conversion to int is defined only
// for a finite value below 2^31 in magnitude: that is decided here in floating point, BEFORE any conversion -- an (int) of a
// larger product, of Inf or of NaN (0 * inf: a subnormal leaf has an infinite inverse) is undefined, and where it yields INT_MIN
// for both bounds the axis would pass as one voxel.  Lattices that pass get the numbers the expressions above give.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define PCC_VOXEL_HD __host__ __device__
#else
#define PCC_VOXEL_HD
#endif

namespace pcc {

constexpr unsigned int VOXEL_MAX_CELLS = 1u << 26;  // PCL refuses where the voxel index overflows int32; this library at 2^26

enum {
    VOXEL_PLAN_OK = 0,
    VOXEL_PLAN_RANGE = 1,  // a bound's voxel coordinate is not finite or not below 2^31 in magnitude: nothing else is set
    VOXEL_PLAN_CELLS = 2   // more than VOXEL_MAX_CELLS voxels: `cells` says how many, org and dim are not to be used
};

struct VoxelPlan {
    float org[3];  // float(min_b)
    int dim[3];    // div_b
    double cells;  // dim[0] * dim[1] * dim[2]
    int verdict;
};

// lo <= hi per axis, all six finite (the caller has dealt with a cloud without finite points)
PCC_VOXEL_HD inline VoxelPlan voxel_plan(const float lo[3], const float hi[3], float inv) {
    VoxelPlan p;
    p.cells = 1;
    p.verdict = VOXEL_PLAN_OK;
    for (int a = 0; a < 3; ++a) { p.org[a] = 0.f; p.dim[a] = 0; }
    for (int a = 0; a < 3; ++a) {
        const float fl = floorf(lo[a] * inv), fh = floorf(hi[a] * inv);
        if (!(fabsf(fl) < 2147483648.0f) || !(fabsf(fh) < 2147483648.0f)) {  // (false for NaN)
            p.cells = 0;
            p.verdict = VOXEL_PLAN_RANGE;
            return p;
        }
        const int mn = (int)fl, mx = (int)fh;
        p.org[a] = (float)mn;
        const double d = (double)mx - (double)mn + 1.0;  // (up to 2^32: not an int yet)
        p.cells *= d;
        p.dim[a] = d <= (double)VOXEL_MAX_CELLS ? (int)d : 0;
    }
    if (p.cells > (double)VOXEL_MAX_CELLS) p.verdict = VOXEL_PLAN_CELLS;
    return p;
}

}  // namespace pcc
