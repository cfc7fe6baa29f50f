// libm_f64.hpp -- acos and atan2 in double for the SHOT descriptor (shot_math.hpp), built from + - * / sqrt and bit operations
// alone, so that the gfx950 compile and the host compile return the same bits.  The device's own double functions (ocml) and
// the host's (glibc) each stay below an ulp, but not the same ulp: a SHOT bin receives float(value), and the two would part at
// every float rounding boundary a last double bit straddles.  These functions are pcc_shot_descriptors' own DEFINITION of acos
// and atan2; glibc's double routines (table-driven, correctly rounded in recent versions) cannot be restated.
//
// What is restated, [recalled] from fdlibm 5.3 (Sun Microsystems, freely distributable), operation for operation:
//   lm_acos  : e_acos.c   -- |x| < 0.5: pi/2 - (x + x R(x^2)); x < -0.5: pi - 2 (s + R(z) s) with z = (1 + x) / 2, s = sqrt(z);
//                            x > 0.5: 2 (df + (R(z) s + c)) with z = (1 - x) / 2, df = s with its low word cleared, c the
//                            correction (z - df^2) / (s + df); R = p / q, degree 6 over degree 4.
//   lm_atan  : s_atan.c   -- reduction at 7/16, 11/16, 19/16, 39/16 to atan(0.5), atan(1), atan(1.5), atan(inf) (hi + lo), an
//                            11-term polynomial in odd / even halves.
//   lm_atan2 : e_atan2.c  -- the special cases, then atan(|y / x|) moved into the quadrant with pi's low word.
// The coefficient tables are fdlibm's (tests/test_libm_f64_cpu.py holds them to 2 ulp of the host's libm over dense sweeps,
// the quadrants, the axes, signed zeros, subnormals and the reduction breakpoints; special values exact).  Compiled without
// contraction (-ffp-contract=off) on both sides; '/' and sqrt are IEEE on both.
#pragma once
#include "libm_f32.hpp"  // lm_bits64, lm_double

namespace pcc {

__host__ __device__ inline int32_t lm_hi(double d) { return (int32_t)(lm_bits64(d) >> 32); }
__host__ __device__ inline uint32_t lm_lo(double d) { return (uint32_t)lm_bits64(d); }
__host__ __device__ inline double lm_abs(double d) { return lm_double(lm_bits64(d) & 0x7fffffffffffffffull); }
__host__ __device__ inline double lm_neg(double d) { return lm_double(lm_bits64(d) ^ 0x8000000000000000ull); }

// ---- acos (e_acos.c) ------------------------------------------------------------------------------------------------------
__host__ __device__ inline double lm_acos_r(double z) {
    const double pS0 = 1.66666666666666657415e-01, pS1 = -3.25565818622400915405e-01, pS2 = 2.01212532134862925881e-01,
                 pS3 = -4.00555345006794114027e-02, pS4 = 7.91534994289814532176e-04, pS5 = 3.47933107596021167570e-05,
                 qS1 = -2.40339491173441421878e+00, qS2 = 2.02094576023350569471e+00, qS3 = -6.88283971605453293030e-01,
                 qS4 = 7.70381505559019352791e-02;
    const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    return p / q;
}
__host__ __device__ inline double lm_acos(double x) {
    const double pi = 3.14159265358979311600e+00, pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17;
    const int32_t hx = lm_hi(x), ix = hx & 0x7fffffff;
    if (ix >= 0x3ff00000) {  // |x| >= 1
        if (((uint32_t)(ix - 0x3ff00000) | lm_lo(x)) == 0) return hx > 0 ? 0.0 : pi + 2.0 * pio2_lo;
        return lm_double(0x7ff8000000000000ull);  // |x| > 1 or NaN
    }
    if (ix < 0x3fe00000) {  // |x| < 0.5
        if (ix <= 0x3c600000) return pio2_hi + pio2_lo;
        const double r = lm_acos_r(x * x);
        return pio2_hi - (x - (pio2_lo - r * x));
    }
    if (hx < 0) {  // x < -0.5
        const double z = (1.0 + x) * 0.5, s = sqrt(z), r = lm_acos_r(z);
        const double w = r * s - pio2_lo;
        return pi - 2.0 * (s + w);
    }
    const double z = (1.0 - x) * 0.5, s = sqrt(z);
    const double df = lm_double(lm_bits64(s) & 0xffffffff00000000ull);
    const double c = (z - df * df) / (s + df);
    const double r = lm_acos_r(z);
    const double w = r * s + c;
    return 2.0 * (df + w);
}

// ---- atan (s_atan.c) ------------------------------------------------------------------------------------------------------
__host__ __device__ inline double lm_atan(double x) {
    const double aT0 = 3.33333333333329318027e-01, aT1 = -1.99999999998764832476e-01, aT2 = 1.42857142725034663711e-01,
                 aT3 = -1.11111104054623557880e-01, aT4 = 9.09088713343650656196e-02, aT5 = -7.69187620504482999495e-02,
                 aT6 = 6.66107313738753120669e-02, aT7 = -5.83357013379057348645e-02, aT8 = 4.97687799461593236017e-02,
                 aT9 = -3.65315727442169155270e-02, aT10 = 1.62858201153657823623e-02;
    const int32_t hx = lm_hi(x), ix = hx & 0x7fffffff;
    double hi = 0.0, lo = 0.0;
    bool reduced = true;
    if (ix >= 0x44100000) {  // |x| >= 2^66
        if (ix > 0x7ff00000 || (ix == 0x7ff00000 && lm_lo(x) != 0)) return x + x;  // NaN
        const double big = 1.57079632679489655800e+00 + 6.12323399573676603587e-17;
        return hx > 0 ? big : lm_neg(big);
    }
    if (ix < 0x3fdc0000) {  // |x| < 0.4375
        if (ix < 0x3e200000) return x;  // |x| < 2^-29
        reduced = false;
    } else {
        x = lm_abs(x);
        if (ix < 0x3ff30000) {      // |x| < 1.1875
            if (ix < 0x3fe60000) {  // 7/16 <= |x| < 11/16
                hi = 4.63647609000806093515e-01; lo = 2.26987774529616870924e-17;
                x = (2.0 * x - 1.0) / (2.0 + x);
            } else {                // 11/16 <= |x| < 19/16
                hi = 7.85398163397448278999e-01; lo = 3.06161699786838301793e-17;
                x = (x - 1.0) / (x + 1.0);
            }
        } else if (ix < 0x40038000) {  // |x| < 2.4375
            hi = 9.82793723247329054082e-01; lo = 1.39033110312309984516e-17;
            x = (x - 1.5) / (1.0 + 1.5 * x);
        } else {                       // 2.4375 <= |x| < 2^66
            hi = 1.57079632679489655800e+00; lo = 6.12323399573676603587e-17;
            x = -1.0 / x;
        }
    }
    const double z = x * x, w = z * z;
    const double s1 = z * (aT0 + w * (aT2 + w * (aT4 + w * (aT6 + w * (aT8 + w * aT10)))));
    const double s2 = w * (aT1 + w * (aT3 + w * (aT5 + w * (aT7 + w * aT9))));
    if (!reduced) return x - x * (s1 + s2);
    const double r = hi - ((x * (s1 + s2) - lo) - x);
    return hx < 0 ? lm_neg(r) : r;
}

// ---- atan2 (e_atan2.c) ----------------------------------------------------------------------------------------------------
__host__ __device__ inline double lm_atan2(double y, double x) {
    const double tiny = 1.0e-300, pi_o_4 = 7.8539816339744827900E-01, pi_o_2 = 1.5707963267948965580E+00,
                 pi = 3.1415926535897931160E+00, pi_lo = 1.2246467991473531772E-16;
    const int32_t hx = lm_hi(x), hy = lm_hi(y), ix = hx & 0x7fffffff, iy = hy & 0x7fffffff;
    const uint32_t lx = lm_lo(x), ly = lm_lo(y);
    if (ix > 0x7ff00000 || (ix == 0x7ff00000 && lx != 0) || iy > 0x7ff00000 || (iy == 0x7ff00000 && ly != 0)) return x + y;  // NaN
    if (hx == 0x3ff00000 && lx == 0) return lm_atan(y);               // x == 1.0
    const int m = ((hy >> 31) & 1) | ((hx >> 30) & 2);                // 2 * sign(x) + sign(y)
    if (((uint32_t)iy | ly) == 0) {                                   // y == 0
        if (m < 2) return y;                                          // atan(+-0, +anything) = +-0
        return m == 2 ? pi + tiny : -pi - tiny;                       // atan(+-0, -anything) = +-pi
    }
    if (((uint32_t)ix | lx) == 0) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;  // x == 0
    if (ix == 0x7ff00000) {                                           // x is INF
        if (iy == 0x7ff00000) {
            switch (m) {
                case 0: return pi_o_4 + tiny;
                case 1: return -pi_o_4 - tiny;
                case 2: return 3.0 * pi_o_4 + tiny;
                default: return -3.0 * pi_o_4 - tiny;
            }
        }
        switch (m) {
            case 0: return 0.0;
            case 1: return lm_neg(0.0);
            case 2: return pi + tiny;
            default: return -pi - tiny;
        }
    }
    if (iy == 0x7ff00000) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;  // y is INF
    const int k = (iy - ix) >> 20;
    double z;
    if (k > 60) z = pi_o_2 + 0.5 * pi_lo;         // |y / x| > 2^60
    else if (hx < 0 && k < -60) z = 0.0;          // |y| / x < -2^60
    else z = lm_atan(lm_abs(y / x));
    switch (m) {
        case 0: return z;
        case 1: return lm_neg(z);
        case 2: return pi - (z - pi_lo);
        default: return (z - pi_lo) - pi;
    }
}

}  // namespace pcc
