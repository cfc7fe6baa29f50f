// fpfh_math.hpp -- the arithmetic of the FPFH descriptor pipeline (reference src/comparator.cpp:824-875: processFPFH =
// pcl::NormalEstimation, removeNaNNormalsFromPointCloud, pcl::FPFHEstimation with 11 + 11 + 11 bins), shared by the device kernels
// (fpfh.hip) and the host mirror of the tests (tests/cpp/fpfh_host.cpp).  Unfused fp32 (-ffp-contract=off), correctly rounded '/'
// and sqrtf on both sides, lm_acosf and lm_atan2f (libm_f32.hpp) for the transcendentals, IEEE double where PCL's expressions
// promote: the device returns the host's bits.
// The PCL details are [recalled]: PCL 1.7 is not available to compare against, parity with it is unpinned.
#pragma once
#include "libm_f32.hpp"

namespace pcc {

constexpr int FPFH_F_BINS = 11;             // nr_bins_f1 = nr_bins_f2 = nr_bins_f3 (the only shape built)
constexpr int FPFH_BINS = 3 * FPFH_F_BINS;  // pcl::FPFHSignature33: the f1 bins, then f2, then f3
constexpr double FPFH_PI = 3.14159265358979323846;                     // M_PI
constexpr float FPFH_D_PI = 1.0f / (2.0f * 3.14159274101257324f);      // d_pi_ = 1.0f / (2.0f * static_cast<float>(M_PI))

__host__ __device__ inline bool fpfh_finite(float f) { return (lm_bits(f) & 0x7f800000u) != 0x7f800000u; }

// Eigen's Vector4f::dot with the fourth component zero, in storage order: ((x x' + y y') + z z') (+ 0, which changes nothing)
__host__ __device__ inline float fpfh_dot(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
// Eigen's cross3
__host__ __device__ inline void fpfh_cross(const float a[3], const float b[3], float c[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// pcl::computePairFeatures of the pair (p, q) with normals np, nq: f1 = the angle theta, f2 = alpha, f3 = phi, f4 = the
// distance; swapped: the roles of p and q were exchanged (the point whose normal makes the smaller angle with the connecting
// line is the source).  ok == 0: no pair (coincident points, or the line along the source's normal), every feature 0.
struct FpfhPair {
    float f1, f2, f3, f4;
    int ok, swapped;
};
__host__ __device__ inline FpfhPair fpfh_pair(const float p[3], const float np[3], const float q[3], const float nq[3]) {
    FpfhPair r = {0.f, 0.f, 0.f, 0.f, 0, 0};
    float dp[3] = {q[0] - p[0], q[1] - p[1], q[2] - p[2]};
    const float f4 = sqrtf(fpfh_dot(dp, dp));
    if (f4 == 0.f) return r;
    const float a1 = fpfh_dot(np, dp) / f4, a2 = fpfh_dot(nq, dp) / f4;
    float n1[3] = {np[0], np[1], np[2]}, n2[3] = {nq[0], nq[1], nq[2]};
    float f3 = a1;
    if (lm_acosf(fabsf(a1)) > lm_acosf(fabsf(a2))) {
        for (int k = 0; k < 3; ++k) { n1[k] = nq[k]; n2[k] = np[k]; dp[k] = dp[k] * -1.0f; }
        f3 = -a2;
        r.swapped = 1;
    }
    float v[3], w[3];
    fpfh_cross(dp, n1, v);
    const float vn = sqrtf(fpfh_dot(v, v));
    if (vn == 0.f) return r;
    v[0] = v[0] / vn; v[1] = v[1] / vn; v[2] = v[2] / vn;
    fpfh_cross(n1, v, w);
    r.f1 = lm_atan2f(fpfh_dot(w, n2), fpfh_dot(n1, n2));
    r.f2 = fpfh_dot(v, n2);
    r.f3 = f3;
    r.f4 = f4;
    r.ok = 1;
    return r;
}

// computePointSPFHSignature's bins: floor(nr_bins * ((f1 + M_PI) * d_pi_)) and floor(nr_bins * ((f + 1.0) * 0.5)), evaluated in
// double as the C++ expressions promote, clamped to 0 .. 10 (anything that is not >= 0, a NaN included, is bin 0)
__host__ __device__ inline int fpfh_clamp_bin(double h) {
    if (!(h >= 0.0)) return 0;
    return h > (double)(FPFH_F_BINS - 1) ? FPFH_F_BINS - 1 : (int)h;
}
__host__ __device__ inline int fpfh_bin_f1(float f1) {
    return fpfh_clamp_bin(floor((double)FPFH_F_BINS * (((double)f1 + FPFH_PI) * (double)FPFH_D_PI)));
}
__host__ __device__ inline int fpfh_bin_f23(float f) {
    return fpfh_clamp_bin(floor((double)FPFH_F_BINS * (((double)f + 1.0) * 0.5)));
}
// hist_incr of a row of row_len entries (the point itself included): 100 / (row_len - 1); +inf for a row of one, never added
__host__ __device__ inline float fpfh_incr(unsigned int row_len) { return 100.0f / (float)(row_len - 1u); }
// a bin that received `count` votes: hist_incr added count times, which is what PCL's loop leaves whatever the order of the entries
__host__ __device__ inline float fpfh_spfh_value(unsigned int count, float incr) {
    float s = 0.f;
    for (unsigned int k = 0; k < count; ++k) s += incr;
    return s;
}

// weightPointSPFHSignature: the weight of a row entry at squared distance d2 (entries with d2 == 0 are skipped by the caller), and
// the factor a feature's eleven bins are multiplied by, from the running sum of everything added to them: 100.0 / sum in double,
// rounded to float; a zero sum stays zero
__host__ __device__ inline float fpfh_weight(float d2) { return 1.0f / d2; }
__host__ __device__ inline float fpfh_norm_factor(float sum) {
    if (sum != 0.f) sum = (float)(100.0 / (double)sum);
    return sum;
}

}  // namespace pcc
