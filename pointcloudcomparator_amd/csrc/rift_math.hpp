// rift_math.hpp -- the arithmetic of the RIFT descriptor pipeline (reference src/comparator.cpp:590-684: processRIFT =
// pcl::PointCloudXYZRGBtoXYZI, pcl::IntensityGradientEstimation, pcl::RIFTEstimation), shared by the device kernels (rift.hip)
// and the host mirror of the tests (tests/cpp/rift_host.cpp).  Unfused fp32 throughout (-ffp-contract=off), correctly rounded
// '/' and sqrtf on both sides, and ONE acosf (lm_acosf, libm_f32.hpp): the device returns the host's bits.
// The PCL details are [recalled]: PCL 1.7 is not available to compare against, parity with it is unpinned.
#pragma once
#include "libm_f32.hpp"

namespace pcc {

#if defined(__HIPCC__)
#define RIFT_UNROLL _Pragma("unroll")
#else
#define RIFT_UNROLL
#endif

constexpr int RIFT_D_BINS = 4;   // nr_distance_bins (the only shape built)
constexpr int RIFT_G_BINS = 8;   // nr_gradient_bins
constexpr int RIFT_BINS = RIFT_D_BINS * RIFT_G_BINS;
constexpr float RIFT_EPS = 1.1920928955078125e-7f;  // std::numeric_limits<float>::epsilon()
constexpr float RIFT_PI = 3.14159274101257324f;     // static_cast<float>(M_PI)

__host__ __device__ inline bool rift_finite(float f) { return (lm_bits(f) & 0x7f800000u) != 0x7f800000u; }

// PointCloudXYZRGBtoXYZI: 0.299 r + 0.587 g + 0.114 b on the bytes of PCL's packed colour word (b, g, r, a from the low byte)
__host__ __device__ inline float rift_intensity(uint32_t bgra) {
    const float r = (float)((bgra >> 16) & 0xffu), g = (float)((bgra >> 8) & 0xffu), b = (float)(bgra & 0xffu);
    return 0.299f * r + 0.587f * g + 0.114f * b;
}

// A x = b for a symmetric 3 x 3 A (a[6] = A00 A01 A02 A11 A12 A22): Householder QR with column pivoting, the method of
// Eigen's colPivHouseholderQr().solve(): the column of largest remaining squared norm is reflected next; pivots not above
// epsilon * 3 * |largest pivot| count as zero and their unknowns are set to 0 (the rank-revealing solve of a minimum basis,
// not a least-norm solution).  Every index is static so that the device keeps the matrix in registers.
__host__ __device__ inline void rift_solve3(const float a[6], const float b[3], float x[3]) {
    // columns c0 c1 c2 (rows r), right-hand side y, p* = which unknown each column stands for
    float c0[3] = {a[0], a[1], a[2]}, c1[3] = {a[1], a[3], a[4]}, c2[3] = {a[2], a[4], a[5]}, y[3] = {b[0], b[1], b[2]};
    int p0 = 0, p1 = 1, p2 = 2;
#define RIFT_SWAP_COL(u, v, pu, pv)                                                                   \
    {                                                                                                 \
        RIFT_UNROLL for (int r_ = 0; r_ < 3; ++r_) { const float t_ = u[r_]; u[r_] = v[r_]; v[r_] = t_; } \
        const int t_ = pu; pu = pv; pv = t_;                                                          \
    }
    // step 0: pivot among three columns over rows 0..2
    {
        const float n0 = c0[0] * c0[0] + c0[1] * c0[1] + c0[2] * c0[2], n1 = c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2],
                    n2 = c2[0] * c2[0] + c2[1] * c2[1] + c2[2] * c2[2];
        if (n1 > n0 && n1 >= n2) RIFT_SWAP_COL(c0, c1, p0, p1)
        else if (n2 > n0 && n2 > n1) RIFT_SWAP_COL(c0, c2, p0, p2)
    }
    float r00 = 0.f, r11 = 0.f, r22 = 0.f;
    {
        const float tail = c0[1] * c0[1] + c0[2] * c0[2];
        const float nrm = sqrtf(c0[0] * c0[0] + tail);
        r00 = c0[0];
        if (tail != 0.f) {
            const float beta = c0[0] >= 0.f ? -nrm : nrm;  // the reflected column is (beta, 0, 0)
            const float v0 = c0[0] - beta, v1 = c0[1], v2 = c0[2];
            const float vv = v0 * v0 + tail;
            // H z = z - 2 v (v . z) / (v . v)
#define RIFT_REFLECT3(z)                                           \
    {                                                              \
        const float f_ = 2.0f * (v0 * z[0] + v1 * z[1] + v2 * z[2]) / vv; \
        z[0] -= f_ * v0; z[1] -= f_ * v1; z[2] -= f_ * v2;         \
    }
            RIFT_REFLECT3(c1) RIFT_REFLECT3(c2) RIFT_REFLECT3(y)
#undef RIFT_REFLECT3
            r00 = beta;
        }
    }
    // step 1: pivot among two columns over rows 1..2
    {
        const float n1 = c1[1] * c1[1] + c1[2] * c1[2], n2 = c2[1] * c2[1] + c2[2] * c2[2];
        if (n2 > n1) RIFT_SWAP_COL(c1, c2, p1, p2)
    }
#undef RIFT_SWAP_COL
    {
        const float tail = c1[2] * c1[2];
        const float nrm = sqrtf(c1[1] * c1[1] + tail);
        r11 = c1[1];
        if (tail != 0.f) {
            const float beta = c1[1] >= 0.f ? -nrm : nrm;
            const float v1 = c1[1] - beta, v2 = c1[2];
            const float vv = v1 * v1 + tail;
#define RIFT_REFLECT2(z)                                \
    {                                                   \
        const float f_ = 2.0f * (v1 * z[1] + v2 * z[2]) / vv; \
        z[1] -= f_ * v1; z[2] -= f_ * v2;               \
    }
            RIFT_REFLECT2(c2) RIFT_REFLECT2(y)
#undef RIFT_REFLECT2
            r11 = beta;
        }
    }
    r22 = c2[2];
    // rank: pivots above epsilon * 3 * |largest pivot| (the pivots do not grow, so the first is the largest)
    const float thr = fabsf(r00) * (RIFT_EPS * 3.0f);
    const int rank = fabsf(r00) > thr ? (fabsf(r11) > thr ? (fabsf(r22) > thr ? 3 : 2) : 1) : 0;
    // back substitution on the leading rank x rank triangle
    float z0 = 0.f, z1 = 0.f, z2 = 0.f;
    if (rank == 3) z2 = y[2] / r22;
    if (rank >= 2) z1 = (y[1] - c2[1] * z2) / r11;
    if (rank >= 1) z0 = ((y[0] - c1[0] * z1) - c2[0] * z2) / r00;
    x[0] = p0 == 0 ? z0 : (p1 == 0 ? z1 : z2);
    x[1] = p0 == 1 ? z0 : (p1 == 1 ? z1 : z2);
    x[2] = p0 == 2 ? z0 : (p1 == 2 ? z1 : z2);
}

// IntensityGradientEstimation's tail: the least-squares gradient x projected onto the tangent plane of normal n, (I - n n^T) x
__host__ __device__ inline void rift_project(const float n[3], const float x[3], float g[3]) {
    const float m00 = 1.0f - n[0] * n[0], m01 = 0.0f - n[0] * n[1], m02 = 0.0f - n[0] * n[2];
    const float m11 = 1.0f - n[1] * n[1], m12 = 0.0f - n[1] * n[2], m22 = 1.0f - n[2] * n[2];
    g[0] = (m00 * x[0] + m01 * x[1]) + m02 * x[2];
    g[1] = (m01 * x[0] + m11 * x[1]) + m12 * x[2];
    g[2] = (m02 * x[0] + m12 * x[1]) + m22 * x[2];
}

// what one row entry contributes: its place on the distance axis, on the angle axis, and the vote it casts
struct RiftVote {
    float d, g, mag;
};
// p0: the descriptor's point; p, gv: the entry's point and intensity gradient; d2: the entry's squared distance as the radius
// search returned it; radius: the float search radius
__host__ __device__ inline RiftVote rift_vote(const float p0[3], const float p[3], const float gv[3], float d2, float radius) {
    RiftVote v;
    v.mag = sqrtf((gv[0] * gv[0] + gv[1] * gv[1]) + gv[2] * gv[2]);
    const float ex = p[0] - p0[0], ey = p[1] - p0[1], ez = p[2] - p0[2];
    const float en = sqrtf((ex * ex + ey * ey) + ez * ez);
    const float ux = ex / en, uy = ey / en, uz = ez / en;
    float ang = lm_acosf(((gv[0] * ux + gv[1] * uy) + gv[2] * uz) / v.mag);
    if (!rift_finite(ang)) ang = 0.0f;  // (the point itself: 0 / 0)
    v.d = (float)RIFT_D_BINS * sqrtf(d2) / (radius + RIFT_EPS);
    v.g = (float)RIFT_G_BINS * ang / (RIFT_PI + RIFT_EPS);
    return v;
}
// the bins a vote reaches: d_idx in [d_lo, d_hi], g_idx in [g_lo, g_hi] (g_idx wraps modulo the angular bins)
__host__ __device__ inline void rift_vote_range(const RiftVote& v, int* d_lo, int* d_hi, int* g_lo, int* g_hi) {
    const int dl = (int)ceilf(v.d - 1.0f), dh = (int)floorf(v.d + 1.0f);
    *d_lo = dl > 0 ? dl : 0;
    *d_hi = dh < RIFT_D_BINS - 1 ? dh : RIFT_D_BINS - 1;
    *g_lo = (int)ceilf(v.g - 1.0f);
    *g_hi = (int)floorf(v.g + 1.0f);
}
// the share of the vote that bin (d_idx, g_idx) receives (bilinear in both axes)
__host__ __device__ inline float rift_vote_term(const RiftVote& v, int d_idx, int g_idx) {
    const float w = (1.0f - fabsf(v.d - (float)d_idx)) * (1.0f - fabsf(v.g - (float)g_idx));
    return w * v.mag;
}
// |h|_2 of the 32 bins in output order (histogram[g_bin * 4 + d_bin]); every bin is then divided by it
__host__ __device__ inline float rift_norm(const float* h, int stride = 1) {
    float s = 0.f;
    for (int k = 0; k < RIFT_BINS; ++k) s += h[k * stride] * h[k * stride];
    return sqrtf(s);
}

}  // namespace pcc
