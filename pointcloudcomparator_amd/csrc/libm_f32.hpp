// libm_f32.hpp -- glibc 2.35's sinf / cosf / atan2f (and acosf, for the RIFT histogram: see lm_acosf; expf, for the SIFT scale space: see lm_expf), restated so that the device evaluates what the host's libm does.
//
// pcl::eigen33 (NormalEstimation, the RANSAC refit; reference src/segmentation.cpp:232-241, 79-117) takes the roots of the
// characteristic cubic in closed form: theta = atan2f(sqrtf(-q), half_b) / 3, then cosf(theta), sinf(theta).  The smallest
// root is a difference of O(1) terms, so an ulp in those three calls is an ulp-sized slice of the curvature and the normal:
// with the device's own (correctly rounded) versions 2.3 % of all points differed from the host's in their last bits.  A libm
// is not specified to the bit, but an IMPLEMENTATION is: these are the algorithms of the glibc the oracle runs against
// (2.35, x86-64), operation for operation, compiled without contraction on both sides:
//   sinf / cosf : sysdeps/ieee754/flt-32/s_sinf.c, s_cosf.c, s_sincosf.h (Szabolcs Nagy / Wilco Dijkstra's double-precision
//                 polynomials: reduction by pi/2 through a scaled integer conversion, degree-7 / degree-8 minimax forms), in
//                 the form glibc runs on CPUs with FMA (__sinf_fma / __cosf_fma: every multiply-add contracted -- explicit
//                 fma() here, v_fma_f64 on the device).  On [0, 1.2] -- theta never leaves [0, pi/3] -- the contracted and the
//                 baseline build return the same float for every one of the 1 067 030 939 arguments; over [0, 120) they
//                 differ for ~1 argument in two million (cancellation next to the zeros).
//   atan2f      : sysdeps/ieee754/flt-32/e_atan2f.c + s_atanf.c (fdlibm: float arithmetic, four reduction intervals, an
//                 11-term odd / even polynomial; one build for all CPUs).  The constants are the ones the binary holds
//                 (aT[0] is 0x3eaaaaab; the source's comment says ...aa).
// tests/test_libm_cpu.py (tests/cpp/test_libm.cpp) compares them with the host's libm: sinf / cosf on every float of
// [2^-13, 1.2] and 80M arguments over (-120, 120), atanf on every 64th float of the whole line plus three whole binades,
// atan2f on 40M pairs and the special cases -- all bits equal (the full sweeps, 2^32 arguments of atanf and 4e8 pairs of
// atan2f, were run once when this file was written: no mismatch).  Beyond 120 in magnitude sinf / cosf fall back to the
// double-precision functions (never reached by the callers).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#else
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif
#include <cmath>
#include <cstdint>
#include <cstring>

namespace pcc {

__host__ __device__ inline uint32_t lm_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
#endif
}
__host__ __device__ inline float lm_float(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f;
    memcpy(&f, &u, 4);
    return f;
#endif
}

// ---- sinf / cosf ------------------------------------------------------------------------------------------------------
// a * b + c as glibc's build for FMA-capable CPUs evaluates it (__sinf_fma / __cosf_fma: every multiply-add of the
// polynomials and of the reduction contracted); LM_NO_FMA gives the baseline build's form (tests)
#ifdef LM_NO_FMA
#define LM_MADD(a, b, c) ((a) * (b) + (c))
#else
#define LM_MADD(a, b, c) fma((a), (b), (c))
#endif
struct LmSincos {
    double sign[4];
    double hpi_inv, hpi, c0, c1, c2, c3, c4, s1, s2, s3;
};
__host__ __device__ inline LmSincos lm_sincos_table(int k) {
    // __sincosf_table[0] and [1] (the second negates the cosine polynomial)
    const double sg = k ? -1.0 : 1.0;
    return LmSincos{{1.0, -1.0, -1.0, 1.0},
                    0x1.45F306DC9C883p+23,  // 2 / pi * 2^24
                    0x1.921FB54442D18p0,    // pi / 2
                    sg * 0x1p0, sg * -0x1.ffffffd0c621cp-2, sg * 0x1.55553e1068f19p-5, sg * -0x1.6c087e89a359dp-10, sg * 0x1.99343027bf8c3p-16,
                    -0x1.555545995a603p-3, 0x1.1107605230bc4p-7, -0x1.994eb3774cf24p-13};
}
__host__ __device__ inline uint32_t lm_abstop12(float x) { return (lm_bits(x) >> 20) & 0x7ffu; }
// sin (n even) or cos (n odd) polynomial of the reduced argument, evaluated in double and rounded once
__host__ __device__ inline float lm_sinf_poly(double x, double x2, const LmSincos& p, int n) {
    if ((n & 1) == 0) {
        const double x3 = x * x2;
        const double s1 = LM_MADD(x2, p.s3, p.s2);
        const double x7 = x3 * x2;
        const double s = LM_MADD(x3, p.s1, x);
        return (float)LM_MADD(x7, s1, s);
    }
    const double x4 = x2 * x2;
    const double c2 = LM_MADD(x2, p.c4, p.c3);
    const double c1 = LM_MADD(x2, p.c1, p.c0);
    const double x6 = x4 * x2;
    const double c = LM_MADD(x4, p.c2, c1);
    return (float)LM_MADD(x6, c2, c);
}
__host__ __device__ inline double lm_reduce_fast(double x, const LmSincos& p, int* np) {
    const double r = x * p.hpi_inv;
    const int n = ((int32_t)r + 0x800000) >> 24;
    *np = n;
    return LM_MADD(-(double)n, p.hpi, x);
}
// 2 / pi in 32-bit windows one byte apart (__inv_pio4); a switch, not an array: no table in memory on the device
__host__ __device__ inline uint32_t lm_inv_pio4(unsigned int i) {
    switch (i) {
#define LM_P(I, V) case I: return V
        LM_P(0, 0xa2u); LM_P(1, 0xa2f9u); LM_P(2, 0xa2f983u); LM_P(3, 0xa2f9836eu);
        LM_P(4, 0xf9836e4eu); LM_P(5, 0x836e4e44u); LM_P(6, 0x6e4e4415u); LM_P(7, 0x4e441529u);
        LM_P(8, 0x441529fcu); LM_P(9, 0x1529fc27u); LM_P(10, 0x29fc2757u); LM_P(11, 0xfc2757d1u);
        LM_P(12, 0x2757d1f5u); LM_P(13, 0x57d1f534u); LM_P(14, 0xd1f534ddu); LM_P(15, 0xf534ddc0u);
        LM_P(16, 0x34ddc0dbu); LM_P(17, 0xddc0db62u); LM_P(18, 0xc0db6295u); LM_P(19, 0xdb629599u);
        LM_P(20, 0x6295993cu); LM_P(21, 0x95993c43u); LM_P(22, 0x993c4390u);
#undef LM_P
        default: return 0x3c439041u;
    }
}
// reduce_large: |y| >= 120, finite.  The argument's 24 significant bits times 96 bits of 2 / pi in integers; the quadrant is
// the top two bits of the product, the rest (a signed 62-bit fraction of a quadrant) goes to double and is scaled by pi / 2.
__host__ __device__ inline double lm_reduce_large(uint32_t xi, int* np) {
    const unsigned int w = (xi >> 26) & 15u;
    const int shift = (int)((xi >> 23) & 7u);
    xi = (xi & 0xffffffu) | 0x800000u;
    xi <<= shift;
    uint64_t res0 = (uint64_t)(uint32_t)(xi * lm_inv_pio4(w));
    const uint64_t res1 = (uint64_t)xi * lm_inv_pio4(w + 4), res2 = (uint64_t)xi * lm_inv_pio4(w + 8);
    res0 = (res2 >> 32) | (res0 << 32);
    res0 += res1;
    const uint64_t n = (res0 + (1ull << 61)) >> 62;
    res0 -= n << 62;
    *np = (int)n;
    return (double)(int64_t)res0 * 0x1.921FB54442D18p-62;
}
// |y| >= 120: sinf (odd = 0) or cosf (odd = 1) through reduce_large; Inf and NaN give NaN
__host__ __device__ inline float lm_sincosf_large(float y, int odd) {
    if (lm_abstop12(y) >= 0x7f8u) return (y - y) / (y - y);
    const uint32_t xi = lm_bits(y);
    const int sign = (int)(xi >> 31);
    int n;
    const double x = lm_reduce_large(xi, &n);
    const LmSincos p0 = lm_sincos_table(0);
    const double s = p0.sign[(n + sign) & 3];
    return lm_sinf_poly(x * s, x * x, lm_sincos_table(((n + sign) & 2) ? 1 : 0), n ^ odd);
}
__host__ __device__ inline float lm_sinf(float y) {
    double x = (double)y;
    if (lm_abstop12(y) < lm_abstop12(0x1.921FB6p-1f)) {  // |y| < pi / 4
        if (lm_abstop12(y) < lm_abstop12(0x1p-12f)) return y;
        return lm_sinf_poly(x, x * x, lm_sincos_table(0), 0);
    }
    if (lm_abstop12(y) < lm_abstop12(120.0f)) {
        int n;
        const LmSincos p0 = lm_sincos_table(0);
        x = lm_reduce_fast(x, p0, &n);
        const double s = p0.sign[n & 3];
        return lm_sinf_poly(x * s, x * x, lm_sincos_table((n & 2) ? 1 : 0), n);
    }
    // (no caller gets here: the branch is glibc's so that the whole-line sweep against the host's libm holds, see above)
    return lm_sincosf_large(y, 0);
}
__host__ __device__ inline float lm_cosf(float y) {
    double x = (double)y;
    if (lm_abstop12(y) < lm_abstop12(0x1.921FB6p-1f)) {
        if (lm_abstop12(y) < lm_abstop12(0x1p-12f)) return 1.0f;
        return lm_sinf_poly(x, x * x, lm_sincos_table(0), 1);
    }
    if (lm_abstop12(y) < lm_abstop12(120.0f)) {
        int n;
        const LmSincos p0 = lm_sincos_table(0);
        x = lm_reduce_fast(x, p0, &n);
        const double s = p0.sign[n & 3];
        return lm_sinf_poly(x * s, x * x, lm_sincos_table((n & 2) ? 1 : 0), n ^ 1);
    }
    return lm_sincosf_large(y, 1);
}

// ---- atanf / atan2f (fdlibm, float arithmetic) ---------------------------------------------------------------------------
__host__ __device__ inline float lm_atanf(float x) {
    const float atanhi[4] = {lm_float(0x3eed6338u), lm_float(0x3f490fdau), lm_float(0x3f7b985eu), lm_float(0x3fc90fdau)};
    const float atanlo[4] = {lm_float(0x31ac3769u), lm_float(0x33222168u), lm_float(0x33140fb4u), lm_float(0x33a22168u)};
    const float aT0 = lm_float(0x3eaaaaabu), aT1 = lm_float(0xbe4ccccdu), aT2 = lm_float(0x3e124925u), aT3 = lm_float(0xbde38e38u),
                aT4 = lm_float(0x3dba2e6eu), aT5 = lm_float(0xbd9d8795u), aT6 = lm_float(0x3d886b35u), aT7 = lm_float(0xbd6ef16bu),
                aT8 = lm_float(0x3d4bda59u), aT9 = lm_float(0xbd15a221u), aT10 = lm_float(0x3c8569d7u);
    const int32_t hx = (int32_t)lm_bits(x), ix = hx & 0x7fffffff;
    int id;
    if (ix >= 0x4c000000) {  // |x| >= 2^25
        if (ix > 0x7f800000) return x + x;
        return hx > 0 ? atanhi[3] + atanlo[3] : -atanhi[3] - atanlo[3];
    }
    if (ix < 0x3ee00000) {  // |x| < 0.4375
        if (ix < 0x31000000) return x;  // |x| < 2^-29
        id = -1;
    } else {
        x = fabsf(x);
        if (ix < 0x3f980000) {      // |x| < 1.1875
            if (ix < 0x3f300000) { id = 0; x = (2.0f * x - 1.0f) / (2.0f + x); }
            else { id = 1; x = (x - 1.0f) / (x + 1.0f); }
        } else {
            if (ix < 0x401c0000) { id = 2; x = (x - 1.5f) / (1.0f + 1.5f * x); }
            else { id = 3; x = -1.0f / x; }
        }
    }
    const float z = x * x, w = z * z;
    const float s1 = z * (aT0 + w * (aT2 + w * (aT4 + w * (aT6 + w * (aT8 + w * aT10)))));
    const float s2 = w * (aT1 + w * (aT3 + w * (aT5 + w * (aT7 + w * aT9))));
    if (id < 0) return x - x * (s1 + s2);
    const float r = atanhi[id] - ((x * (s1 + s2) - atanlo[id]) - x);
    return hx < 0 ? -r : r;
}
__host__ __device__ inline float lm_atan2f(float y, float x) {
    const float tiny = 1.0e-30f, pi_o_4 = lm_float(0x3f490fdbu), pi_o_2 = lm_float(0x3fc90fdbu), pi = lm_float(0x40490fdbu),
                pi_lo = lm_float(0xb3bbbd2eu);
    const int32_t hx = (int32_t)lm_bits(x), ix = hx & 0x7fffffff, hy = (int32_t)lm_bits(y), iy = hy & 0x7fffffff;
    if (ix > 0x7f800000 || iy > 0x7f800000) return x + y;  // NaN
    if (hx == 0x3f800000) return lm_atanf(y);              // x = 1
    const int m = ((hy >> 31) & 1) | ((hx >> 30) & 2);     // 2 * sign(x) + sign(y)
    if (iy == 0) {
        if (m < 2) return y;
        return m == 2 ? pi + tiny : -pi - tiny;
    }
    if (ix == 0) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
    if (ix == 0x7f800000) {
        if (iy == 0x7f800000) {
            if (m == 0) return pi_o_4 + tiny;
            if (m == 1) return -pi_o_4 - tiny;
            return m == 2 ? 3.0f * pi_o_4 + tiny : -3.0f * pi_o_4 - tiny;
        }
        if (m == 0) return 0.0f;
        if (m == 1) return -0.0f;
        return m == 2 ? pi + tiny : -pi - tiny;
    }
    if (iy == 0x7f800000) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
    const int k = (iy - ix) >> 23;
    float z;
    if (k > 60) z = pi_o_2 + 0.5f * pi_lo;
    else if (hx < 0 && k < -60) z = 0.0f;
    else z = lm_atanf(fabsf(y / x));
    if (m == 0) return z;
    if (m == 1) return lm_float(lm_bits(z) ^ 0x80000000u);
    return m == 2 ? pi - (z - pi_lo) : (z - pi_lo) - pi;
}

// ---- acosf (fdlibm, float arithmetic) ---------------------------------------------------------------------------------
// sysdeps/ieee754/flt-32/e_acosf.c: three intervals (|x| < 0.5, x <= -0.5, x >= 0.5), one rational approximation
// R(z) = z P(z) / Q(z) of (asin(x) - x) / x^3, a correctly rounded sqrtf and float arithmetic in the source's order; one
// build for all CPUs.  The caller is the RIFT histogram (rift_math.hpp): the angle between a gradient and the direction to
// a neighbour, where one ulp moves a share of a vote from one angular bin to the next.
__host__ __device__ inline float lm_acosf(float x) {
    const float one = 1.0f, pi = lm_float(0x40490fdau), pio2_hi = lm_float(0x3fc90fdau), pio2_lo = lm_float(0x33a22168u),
                pS0 = lm_float(0x3e2aaaabu), pS1 = lm_float(0xbea6b090u), pS2 = lm_float(0x3e4e0aa8u), pS3 = lm_float(0xbd241146u),
                pS4 = lm_float(0x3a4f7f04u), pS5 = lm_float(0x3811ef08u), qS1 = lm_float(0xc019d139u), qS2 = lm_float(0x4001572du),
                qS3 = lm_float(0xbf303361u), qS4 = lm_float(0x3d9dc62eu);
    const int32_t hx = (int32_t)lm_bits(x), ix = hx & 0x7fffffff;
    if (ix == 0x3f800000) return hx > 0 ? 0.0f : pi + 2.0f * pio2_lo;  // |x| = 1
    if (ix > 0x3f800000) return (x - x) / (x - x);                      // |x| > 1 or NaN
    if (ix < 0x3f000000) {                                              // |x| < 0.5
        if (ix <= 0x32800000) return pio2_hi + pio2_lo;                // |x| <= 2^-26
        const float z = x * x;
        const float p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        const float q = one + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        const float r = p / q;
        return pio2_hi - (x - (pio2_lo - x * r));
    }
    if (hx < 0) {  // x <= -0.5
        const float z = (one + x) * 0.5f;
        const float p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        const float q = one + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        const float s = sqrtf(z);
        const float r = p / q;
        const float w = r * s - pio2_lo;
        return pi - 2.0f * (s + w);
    }
    const float z = (one - x) * 0.5f;  // x >= 0.5
    const float s = sqrtf(z);
    const float df = lm_float(lm_bits(s) & 0xfffff000u);
    const float c = (z - df * df) / (s + df);
    const float p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    const float q = one + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    const float r = p / q;
    const float w = r * s + c;
    return 2.0f * (df + w);
}

// ---- expf (double-precision table form) ---------------------------------------------------------------------------------
// sysdeps/ieee754/flt-32/e_expf.c + e_exp2f_data.c (Szabolcs Nagy): x * 32 / ln 2 = k + r with k an integer (the 0x1.8p52
// shift) and r in [-1/2, 1/2]; exp(x) = 2^(k / 32) * 2^(r / 32), the first factor from a 32-entry table whose entries have
// the exponent bits of k folded in by an integer add, the second a degree-3 polynomial; everything in double, rounded to
// float once.  As for sinf / cosf the host runs the build for CPUs with FMA (__expf_fma), which contracts every
// multiply-add -- the scaling product included: it feeds only the shift's addition and the subtraction that yields r, and
// both were fused.  The table is 2^(i / 32) correctly rounded (generated with 80-digit decimal arithmetic), stored as
// bits(2^(i / 32)) - (i << 47).  The caller is the SIFT detector's Gaussian weight (sift_math.hpp), arguments in [-4.5, 0];
// tests/cpp/test_expf.cpp compares every float of that interval, a stride sample of [-104, 89] and the special cases with
// the host's expf.
__host__ __device__ inline double lm_double(uint64_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __longlong_as_double((long long)u);
#else
    double d;
    memcpy(&d, &u, 8);
    return d;
#endif
}
__host__ __device__ inline uint64_t lm_bits64(double d) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint64_t)__double_as_longlong(d);
#else
    uint64_t u;
    memcpy(&u, &d, 8);
    return u;
#endif
}
__host__ __device__ inline uint64_t lm_exp2f_tab(unsigned int i) {
    switch (i & 31u) {
#define LM_T(I, V) case I: return V
        LM_T(0, 0x3ff0000000000000ull); LM_T(1, 0x3fefd9b0d3158574ull); LM_T(2, 0x3fefb5586cf9890full); LM_T(3, 0x3fef9301d0125b51ull);
        LM_T(4, 0x3fef72b83c7d517bull); LM_T(5, 0x3fef54873168b9aaull); LM_T(6, 0x3fef387a6e756238ull); LM_T(7, 0x3fef1e9df51fdee1ull);
        LM_T(8, 0x3fef06fe0a31b715ull); LM_T(9, 0x3feef1a7373aa9cbull); LM_T(10, 0x3feedea64c123422ull); LM_T(11, 0x3feece086061892dull);
        LM_T(12, 0x3feebfdad5362a27ull); LM_T(13, 0x3feeb42b569d4f82ull); LM_T(14, 0x3feeab07dd485429ull); LM_T(15, 0x3feea47eb03a5585ull);
        LM_T(16, 0x3feea09e667f3bcdull); LM_T(17, 0x3fee9f75e8ec5f74ull); LM_T(18, 0x3feea11473eb0187ull); LM_T(19, 0x3feea589994cce13ull);
        LM_T(20, 0x3feeace5422aa0dbull); LM_T(21, 0x3feeb737b0cdc5e5ull); LM_T(22, 0x3feec49182a3f090ull); LM_T(23, 0x3feed503b23e255dull);
        LM_T(24, 0x3feee89f995ad3adull); LM_T(25, 0x3feeff76f2fb5e47ull); LM_T(26, 0x3fef199bdd85529cull); LM_T(27, 0x3fef3720dcef9069ull);
        LM_T(28, 0x3fef5818dcfba487ull); LM_T(29, 0x3fef7c97337b9b5full); LM_T(30, 0x3fefa4afa2a490daull);
#undef LM_T
        default: return 0x3fefd0765b6e4540ull;
    }
}
__host__ __device__ inline float lm_expf(float x) {
    const double inv_ln2_n = 0x1.71547652b82fep+0 * 32.0, shift = 0x1.8p+52;
    const double c0 = 0x1.c6af84b912394p-5 / 32.0 / 32.0 / 32.0, c1 = 0x1.ebfce50fac4f3p-3 / 32.0 / 32.0, c2 = 0x1.62e42ff0c52d6p-1 / 32.0;
    const uint32_t abstop = (lm_bits(x) >> 20) & 0x7ffu;
    if (abstop >= ((lm_bits(88.0f) >> 20) & 0x7ffu)) {  // |x| >= 88 or NaN
        if (lm_bits(x) == 0xff800000u) return 0.0f;
        if (abstop >= 0x7f8u) return x + x;
        if (x > 0x1.62e42ep6f) return lm_float(0x7f800000u);  // overflow
        if (x < -0x1.9fe368p6f) return 0.0f;                  // underflow
    }
    const double xd = (double)x;
    double kd = LM_MADD(inv_ln2_n, xd, shift);
    const uint64_t ki = lm_bits64(kd);
    kd -= shift;
    const double r = LM_MADD(inv_ln2_n, xd, -kd);
    const uint64_t t = lm_exp2f_tab((unsigned int)ki) + (ki << 47);
    const double s = lm_double(t);
    const double z = LM_MADD(c0, r, c1);
    const double r2 = r * r;
    double y = LM_MADD(c2, r, 1.0);
    y = LM_MADD(z, r2, y);
    y = y * s;
    return (float)y;
}

}  // namespace pcc
