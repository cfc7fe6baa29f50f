// test_expf.cpp -- csrc/libm_f32.hpp's lm_expf (glibc 2.35's expf restated for the device) against the HOST's libm: the
// Gaussian weight of every row entry of the SIFT scale space (csrc/sift_math.hpp; reference src/comparator.cpp:435-469,
// pcl::SIFTKeypoint calls expf) must be the same float on the device and in the host mirror, and is meant to be the host
// libm's.  CPU only.
//   every float of [-4.5, 0] (1 083 179 009 arguments, the range the detector reaches: -0.5 d2 / sigma2 with
//   d2 <= 9 sigma2; `quick` takes every 16th), every 4099th float of [-104, 89], and the non-finite arguments
// prints "expf N arguments: B mismatches, max ulp distance U" and "expf ok" when U is within the value recorded when the
// file was written (0: all bits equal), so that a later edit cannot worsen it unnoticed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <cstring>
#include "libm_f32.hpp"

static const long RECORDED_MAX_ULP = 0;

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float flt(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

int main(int argc, char** argv) {
    const bool quick = argc > 1;
    unsigned long n = 0, bad = 0;
    long max_ulp = 0;
    auto one = [&](float f) {
        ++n;
        volatile float arg = f;  // (no constant folding of the libm call)
        const float a = expf(arg), b = pcc::lm_expf(f);
        if (a != a && b != b) return;
        if (bits(a) == bits(b)) return;
        const long d = (a != a || b != b) ? 0x7fffffffL : labs((long)(int32_t)bits(a) - (long)(int32_t)bits(b));
        if (d > max_ulp) max_ulp = d;
        if (bad++ < 5) printf("expf(%a): libm %a restated %a\n", f, a, b);
    };
    const uint32_t step = quick ? 16 : 1;
    for (uint32_t u = 0x80000000u; u <= bits(-4.5f); u += step) one(flt(u));  // -0 ... -4.5
    one(0.0f); one(-4.5f);
    for (uint32_t u = 0; u <= bits(89.0f); u += 4099u) one(flt(u));
    for (uint32_t u = 0x80000000u; u <= bits(-104.0f); u += 4099u) one(flt(u));
    for (float f : {88.0f, 0x1.62e42ep6f, 0x1.62e430p6f, 89.0f, -87.0f, -88.0f, -0x1.9fe368p6f, -0x1.9fe36ap6f, -0x1.9d1d9ep6f, -104.0f, 1.0f, -1.0f})
        one(f);
    for (uint32_t u : {0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u, 0x00000001u, 0x80000001u}) one(flt(u));
    printf("expf %lu arguments: %lu mismatches, max ulp distance %ld\n", n, bad, max_ulp);
    if (max_ulp > RECORDED_MAX_ULP) return 1;
    printf("expf ok\n");
    return 0;
}
