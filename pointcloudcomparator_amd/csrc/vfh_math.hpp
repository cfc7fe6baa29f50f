// vfh_math.hpp -- the arithmetic of the VFH descriptor and of its distance (reference src/comparator.cpp:471-516: processVHF =
// pcl::NormalEstimation, pcl::VFHEstimation with setNormalizeBins(true), setNormalizeDistance(false); matchVHF = the Euclidean
// distance of two 308-bin histograms), shared by the device kernels (vfh.hip) and the host mirror of the tests
// (tests/cpp/vfh_host.cpp).  The pair features are fpfh_math.hpp's fpfh_pair as it stands; what is added here are the 45-bin and
// 128-bin forms of the bin expressions, the two increments, the viewpoint direction and the distance.  Unfused fp32
// (-ffp-contract=off), correctly rounded '/' and sqrtf on both sides, IEEE double where PCL's expressions promote: the device
// returns the host's bits.
// The PCL details are [recalled]: PCL 1.7 is not available to compare against, parity with it is unpinned.
#pragma once
#include "fpfh_math.hpp"

namespace pcc {

constexpr int VFH_F_BINS = 45;                              // nr_bins_f1_ = ... = nr_bins_f4_
constexpr int VFH_VP_BINS = 128;                            // nr_bins_vp_
constexpr int VFH_BINS = 4 * VFH_F_BINS + VFH_VP_BINS;      // pcl::VFHSignature308: f1, f2, f3, f4, then the viewpoint component
constexpr int VFH_COUNTERS = 3 * VFH_F_BINS + VFH_VP_BINS;  // the bins that receive votes: f1, f2, f3, viewpoint (f4's increment is 0)
constexpr int VFH_NO_VOTE = -1;

// PCL's clamp of a bin number computed in double, and the conversion x86 leaves behind it: anything that is not >= 0, a NaN
// included, is bin 0
__host__ __device__ inline int vfh_clamp_bin(double h, int bins) {
    if (!(h >= 0.0)) return 0;
    return h > (double)(bins - 1) ? bins - 1 : (int)h;
}
// fpfh_bin_f1 / fpfh_bin_f23 with 45 in place of 11
__host__ __device__ inline int vfh_bin_f1(float f1) {
    return vfh_clamp_bin(floor((double)VFH_F_BINS * (((double)f1 + FPFH_PI) * (double)FPFH_D_PI)), VFH_F_BINS);
}
__host__ __device__ inline int vfh_bin_f23(float f) {
    return vfh_clamp_bin(floor((double)VFH_F_BINS * (((double)f + 1.0) * 0.5)), VFH_F_BINS);
}
// the viewpoint component: alpha = (n . d_vp_p + 1) / 2 in double, bin floor(alpha * 128)
__host__ __device__ inline int vfh_bin_vp(float n_dot_d) {
    const double alpha = ((double)n_dot_d + 1.0) * 0.5;
    return vfh_clamp_bin(floor(alpha * (double)VFH_VP_BINS), VFH_VP_BINS);
}
// hist_incr of f1 .. f3 with setNormalizeBins(true): 100 / (n - 1), n the points of the cloud (n >= 2); and the viewpoint
// component's: 100.0 / n in double, rounded to float.  A bin with `count` votes holds its increment added count times
// (fpfh_spfh_value).
__host__ __device__ inline float vfh_incr(unsigned int n) { return 100.0f / (float)(n - 1u); }
__host__ __device__ inline float vfh_incr_vp(unsigned int n) { return (float)(100.0 / (double)n); }

// d_vp_p: the direction from the centroid to the viewpoint (0, 0, 0), normalised by a true division
__host__ __device__ inline void vfh_view_direction(const float centroid[3], float d[3]) {
    for (int k = 0; k < 3; ++k) d[k] = 0.0f - centroid[k];
    const float len = sqrtf(fpfh_dot(d, d));
    for (int k = 0; k < 3; ++k) d[k] = d[k] / len;
}

// The bins ONE point votes into: f1, f2, f3 of computePairFeatures(centroid, normal centroid, point, normal) at 45 bins -- all
// three VFH_NO_VOTE when there is no pair (the point at the centroid, or the line along the source's normal) -- and the bin of
// the viewpoint component, which every point has.  The normal is taken with whatever it holds: a NaN normal votes bin 0 of f1
// and f2, its real f3 bin (a comparison with NaN is false: the roles are never exchanged) and bin 0 of the viewpoint component.
struct VfhVote {
    int f1, f2, f3, vp;
};
__host__ __device__ inline VfhVote vfh_vote(const float centroid[3], const float normal_centroid[3], const float d_vp_p[3], const float p[3],
                                            const float n[3]) {
    VfhVote v = {VFH_NO_VOTE, VFH_NO_VOTE, VFH_NO_VOTE, vfh_bin_vp(fpfh_dot(n, d_vp_p))};
    const FpfhPair f = fpfh_pair(centroid, normal_centroid, p, n);
    if (f.ok) {
        v.f1 = vfh_bin_f1(f.f1);
        v.f2 = vfh_bin_f23(f.f2);
        v.f3 = vfh_bin_f23(f.f3);
    }
    return v;
}
// bin b of the descriptor from the votes' counters (f1[45], f2[45], f3[45], vp[128]); the f4 component is +0.0f in every bin
__host__ __device__ inline float vfh_bin_value(const unsigned int* counters, unsigned int n, int b) {
    if (b < 3 * VFH_F_BINS) return fpfh_spfh_value(counters[b], vfh_incr(n));
    if (b < 4 * VFH_F_BINS) return 0.0f;
    return fpfh_spfh_value(counters[b - VFH_F_BINS], vfh_incr_vp(n));
}

// matchVHF: sqrt(sum over the 308 bins, in order, of pow(h1[k] - h2[k], 2)) -- the difference in float, its square (exact in
// double) and the running sum in double, the root in double
__host__ __device__ inline double vfh_distance(const float* h1, const float* h2) {
    double dis = 0.0;
    for (int k = 0; k < VFH_BINS; ++k) {
        const float d = h1[k] - h2[k];
        const double dd = (double)d;
        dis += dd * dd;
    }
    return sqrt(dis);
}

}  // namespace pcc
