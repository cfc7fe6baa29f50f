// test_acosf.cpp -- csrc/libm_f32.hpp's lm_acosf (glibc 2.35's acosf restated for the device) against the HOST's libm: the
// angle of every RIFT vote (csrc/rift_math.hpp; reference src/comparator.cpp:590-684, pcl::RIFTEstimation calls acosf) must
// be the same float on the device and in the host mirror, and is meant to be the host libm's.  CPU only.
//   every float of [-1, 1] (2 130 706 433 arguments; `quick` takes every 16th), the non-finite arguments, and arguments
//   beyond 1 in magnitude (NaN on both sides)
// prints "acosf N arguments: B mismatches, max ulp distance U" and "acosf ok" when U is within the value recorded when the
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
        const float a = acosf(f), b = pcc::lm_acosf(f);
        if (a != a && b != b) return;
        if (bits(a) == bits(b)) return;
        const long d = (a != a || b != b) ? 0x7fffffffL : labs((long)(int32_t)bits(a) - (long)(int32_t)bits(b));
        if (d > max_ulp) max_ulp = d;
        if (bad++ < 5) printf("acosf(%a): libm %a restated %a\n", f, a, b);
    };
    const uint32_t step = quick ? 16 : 1;
    for (uint32_t u = 0; u <= 0x3f800000u; u += step) { one(flt(u)); one(flt(u | 0x80000000u)); }
    one(1.0f); one(-1.0f);
    // out of range and non-finite: NaN everywhere
    for (uint32_t u = 0x3f800001u; u < 0x7f800000u; u += 0x10001u) { one(flt(u)); one(flt(u | 0x80000000u)); }
    for (uint32_t u : {0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u, 0x3f800001u, 0xbf800001u}) one(flt(u));
    printf("acosf %lu arguments: %lu mismatches, max ulp distance %ld\n", n, bad, max_ulp);
    if (max_ulp > RECORDED_MAX_ULP) return 1;
    printf("acosf ok\n");
    return 0;
}
