// test_device_math.hip -- the shared __host__ __device__ arithmetic (csrc/libm_f32.hpp, plane_fit.hpp, rift_math.hpp,
// sift_math.hpp, rigid_solve.hpp) as the gfx950 compile evaluates it against the host compile of the same text, function
// by function and word for word.  Built with the library's own HIPFLAGS (`make build/test_device_math`): the point is the
// library's code generation.
//   test_device_math         every case set through a kernel (one thread per case, 256 per block) and through the host
//                            pass of the same functor (at most 16 threads); outputs agree when their bits are equal or
//                            both are NaN.  One line per function, `name: N cases, M mismatches`, up to five offending
//                            cases; last line `device math: 0 mismatches`, exit status 0 only then.
//   test_device_math --host  no HIP call at all: the host pass of every lm_* function against this machine's libm on the
//                            same sets (which pins the reference of the device run to what tests/cpp/test_libm.cpp,
//                            test_acosf.cpp and test_expf.cpp pin), and per family of the composite functions how many
//                            cases ended in each observable class (tests/test_device_math_cpu.py asserts that the classes
//                            a family aims at are not empty).  Last line `host math: 0 mismatches against libm`.
// All case sets are generated here from fixed seeds.  Composite functions also emit their intermediates so that a mismatch
// names the stage (plane_from_covariance: the covariance, the three roots of pf_roots3 on the scaled matrix, n, curvature;
// rift_vote: the raw acosf, d, g, mag, the bin ranges and four vote terms; rigid_from_sums: return value, T, the eigenvector).
// Cases per function (223.8 M in all):
//   lm_sinf 34 813 715, lm_cosf 34 813 715, lm_atanf 16 945 178, lm_acosf 50 171 924, lm_expf 33 804 308, lm_atan2f 10 000 225,
//   pf_roots2 400 000, plane_from_sums 500 000 (five families), plane_from_covariance 1 800 011 (ten families),
//   rift_solve3 1 087 500 (ten families), rift_project 200 000, rift_vote 900 000 (five families), rift_vote_bins 300 000,
//   rift_norm 200 000, rift_intensity 16 777 216, sift_intensity 16 777 216, sift_weight 1 489 021, sift_response 500 000,
//   sift_dog 500 000, sift_is_keypoint 1 000 000, sym4_max_eigvec 200 000, rigid_from_sums 360 000 (nine families, with and
//   without a centre), mat4_mul_f 300 000.
// Measured: --host takes 6.5 s of wall time on an 8-core host (11 s of CPU time; the host passes themselves 2.5 s, the rest
// is generating the cases and libm); the device run, both passes and the comparison, took 6 s on an MI355X machine.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include "libm_f32.hpp"
#include "plane_fit.hpp"
#include "rift_math.hpp"
#include "sift_math.hpp"
#include "rigid_solve.hpp"
using namespace pcc;

#define HD __host__ __device__

// ---- harness ------------------------------------------------------------------------------------------------------------
static bool g_host_only = false;
static unsigned long g_total_bad = 0;

#define HIP_OK(call)                                                                              \
    do {                                                                                          \
        const hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                                   \
            std::printf("%s: %s\n", #call, hipGetErrorString(e_));                                \
            std::fflush(stdout);                                                                  \
            std::_Exit(3); /* no further GPU call, no destructor that could make one */           \
        }                                                                                         \
    } while (0)

// fn(begin, end, thread) over [0, n) on at most 16 threads
template <typename Fn>
static void parallel_for(size_t n, Fn fn) {
    const unsigned nt = 16;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) th.emplace_back([&fn, n, t] { fn(n * t / nt, n * (t + 1) / nt, t); });
    for (auto& x : th) x.join();
}

template <typename W, int NI, int NO, typename F>
__global__ void k_eval(const W* in, W* out, size_t n, F f) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        W a[NI], o[NO];
        for (int j = 0; j < NI; ++j) a[j] = in[i * NI + j];
        for (int j = 0; j < NO; ++j) o[j] = 0;
        f(a, o);
        for (int j = 0; j < NO; ++j) out[i * NO + j] = o[j];
    }
}

static bool word_nan(uint32_t u) { return (u & 0x7fffffffu) > 0x7f800000u; }
static bool word_nan(uint64_t u) { return (u & 0x7fffffffffffffffull) > 0x7ff0000000000000ull; }
static void print_word(uint32_t u) { std::printf(" %08x(%a)", u, (double)lm_float(u)); }
static void print_word(uint64_t u) { std::printf(" %016llx(%a)", (unsigned long long)u, lm_double(u)); }

// NI input words and NO output words per case; fam[i] names the family a case belongs to (host-side bookkeeping only)
template <typename W, int NI, int NO>
struct Cases {
    std::vector<W> in;
    std::vector<uint8_t> fam;
    std::vector<W> host;  // the host pass's outputs, kept for the class counts and the libm comparison
    size_t n() const { return fam.size(); }
    W* add(int family) {
        if (in.size() + NI > in.capacity()) { in.reserve(in.capacity() * 2 + 4096 * NI); fam.reserve(fam.capacity() * 2 + 4096); }
        in.resize(in.size() + NI);
        fam.push_back((uint8_t)family);
        return in.data() + in.size() - NI;
    }
};

// NaNs compare equal wherever they are floats; `float_mask` has bit j set when output word j is a float (all, by default)
template <typename W, int NI, int NO, typename F>
static void run(const char* name, Cases<W, NI, NO>& c, F f, uint64_t float_mask = ~0ull) {
    const size_t n = c.n();
    const auto t_start = std::chrono::steady_clock::now();
    c.host.assign(n * NO, 0);
    parallel_for(n, [&](size_t b, size_t e, unsigned) {
        for (size_t i = b; i < e; ++i) f(c.in.data() + i * NI, c.host.data() + i * NO);
    });
    if (g_host_only) {
        std::printf("%s: %zu cases, host pass [%.2f s]\n", name, n, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count());
        return;
    }
    if (n == 0) { std::printf("%s: 0 cases, 0 mismatches\n", name); return; }
    W *din = nullptr, *dout = nullptr;
    std::vector<W> dev(n * NO);
    HIP_OK(hipMalloc(&din, n * NI * sizeof(W)));
    HIP_OK(hipMalloc(&dout, n * NO * sizeof(W)));
    HIP_OK(hipMemcpy(din, c.in.data(), n * NI * sizeof(W), hipMemcpyHostToDevice));
    hipLaunchKernelGGL((k_eval<W, NI, NO, F>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, din, dout, n, f);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(dev.data(), dout, n * NO * sizeof(W), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(din));
    HIP_OK(hipFree(dout));
    unsigned long bad = 0;
    for (size_t i = 0; i < n; ++i) {
        int first = -1;
        for (int j = 0; j < NO && first < 0; ++j) {
            const W h = c.host[i * NO + j], d = dev[i * NO + j];
            if (h != d && !(((float_mask >> j) & 1) && word_nan(h) && word_nan(d))) first = j;
        }
        if (first < 0) continue;
        if (bad++ < 5) {
            std::printf("  %s case %zu (family %d), first differing output word %d\n    in:", name, i, (int)c.fam[i], first);
            for (int j = 0; j < NI; ++j) print_word(c.in[i * NI + j]);
            std::printf("\n    host:");
            for (int j = 0; j < NO; ++j) print_word(c.host[i * NO + j]);
            std::printf("\n    device:");
            for (int j = 0; j < NO; ++j) print_word(dev[i * NO + j]);
            std::printf("\n");
        }
    }
    std::printf("%s: %zu cases, %lu mismatches\n", name, n, bad);
    std::fflush(stdout);
    g_total_bad += bad;
}

// ---- evaluators ---------------------------------------------------------------------------------------------------------
#define UNARY_EVAL(NAME, FN)                                                                  \
    struct NAME {                                                                             \
        HD void operator()(const uint32_t* in, uint32_t* out) const { out[0] = lm_bits(FN(lm_float(in[0]))); } \
    };
UNARY_EVAL(EvSin, lm_sinf)
UNARY_EVAL(EvCos, lm_cosf)
UNARY_EVAL(EvAtan, lm_atanf)
UNARY_EVAL(EvAcos, lm_acosf)
UNARY_EVAL(EvExp, lm_expf)
struct EvAtan2 {
    HD void operator()(const uint32_t* in, uint32_t* out) const { out[0] = lm_bits(lm_atan2f(lm_float(in[0]), lm_float(in[1]))); }
};
struct EvRoots2 {
    HD void operator()(const uint32_t* in, uint32_t* out) const {
        float r[3];
        pf_roots2(lm_float(in[0]), lm_float(in[1]), r);
        for (int j = 0; j < 3; ++j) out[j] = lm_bits(r[j]);
    }
};
// cov[9] -> roots of the scaled matrix (plane_from_covariance's own first stage, restated), n[3], curvature: 7 words at o
HD inline void plane_stages(const float cov[9], uint32_t* o) {
    float scale = 0.f;
    for (int j = 0; j < 9; ++j) scale = fmaxf(scale, fabsf(cov[j]));
    if (scale <= FLT_MIN) scale = 1.f;
    float sm[9], ev[3], n[3], curv;
    for (int j = 0; j < 9; ++j) sm[j] = cov[j] / scale;
    pf_roots3(sm, ev);
    plane_from_covariance(cov, n, &curv);
    for (int j = 0; j < 3; ++j) { o[j] = lm_bits(ev[j]); o[3 + j] = lm_bits(n[j]); }
    o[6] = lm_bits(curv);
}
struct EvPlaneCov {  // in: cov[9]; out: roots[3] n[3] curvature
    HD void operator()(const uint32_t* in, uint32_t* out) const {
        float cov[9];
        for (int j = 0; j < 9; ++j) cov[j] = lm_float(in[j]);
        plane_stages(cov, out);
    }
};
struct EvPlaneSums {  // in: the nine sums, count; out: cov[9] roots[3] n[3] curvature
    HD void operator()(const uint32_t* in, uint32_t* out) const {
        float a[9], cov[9];
        for (int j = 0; j < 9; ++j) a[j] = lm_float(in[j]);
        covariance_from_sums(a, in[9], cov);
        for (int j = 0; j < 9; ++j) out[j] = lm_bits(cov[j]);
        plane_stages(cov, out + 9);
    }
};
struct EvSolve3 {  // in: a[6] b[3]; out: x[3]
    HD void operator()(const uint32_t* in, uint32_t* out) const {
        float a[6], b[3], x[3];
        for (int j = 0; j < 6; ++j) a[j] = lm_float(in[j]);
        for (int j = 0; j < 3; ++j) b[j] = lm_float(in[6 + j]);
        rift_solve3(a, b, x);
        for (int j = 0; j < 3; ++j) out[j] = lm_bits(x[j]);
    }
};
struct EvProject {  // in: n[3] x[3]; out: g[3]
    HD void operator()(const uint32_t* in, uint32_t* out) const {
        float n[3], x[3], g[3];
        for (int j = 0; j < 3; ++j) { n[j] = lm_float(in[j]); x[j] = lm_float(in[3 + j]); }
        rift_project(n, x, g);
        for (int j = 0; j < 3; ++j) out[j] = lm_bits(g[j]);
    }
};
// the bin ranges (4 ints) and the vote terms of the four corner bins: 8 words at o
HD inline void vote_bins(const RiftVote& v, uint32_t* o) {
    int dl, dh, gl, gh;
    rift_vote_range(v, &dl, &dh, &gl, &gh);
    o[0] = (uint32_t)dl; o[1] = (uint32_t)dh; o[2] = (uint32_t)gl; o[3] = (uint32_t)gh;
    o[4] = lm_bits(rift_vote_term(v, dl, gl));
    o[5] = lm_bits(rift_vote_term(v, dh, gh));
    o[6] = lm_bits(rift_vote_term(v, dl, gh));
    o[7] = lm_bits(rift_vote_term(v, dh, gl));
}
struct EvVote {  // in: p0[3] p[3] gv[3] d2 radius; out: raw acosf, d, g, mag, ranges[4], terms[4]
    HD void operator()(const uint32_t* in, uint32_t* out) const {
        float p0[3], p[3], gv[3];
        for (int j = 0; j < 3; ++j) { p0[j] = lm_float(in[j]); p[j] = lm_float(in[3 + j]); gv[j] = lm_float(in[6 + j]); }
        // (rift_vote's own angle before the reset to 0, restated: the stage a mismatch in g would come from)
        const float mag = sqrtf((gv[0] * gv[0] + gv[1] * gv[1]) + gv[2] * gv[2]);
        const float ex = p[0] - p0[0], ey = p[1] - p0[1], ez = p[2] - p0[2];
        const float en = sqrtf((ex * ex + ey * ey) + ez * ez);
        const float ux = ex / en, uy = ey / en, uz = ez / en;
        out[0] = lm_bits(lm_acosf(((gv[0] * ux + gv[1] * uy) + gv[2] * uz) / mag));
        const RiftVote v = rift_vote(p0, p, gv, lm_float(in[9]), lm_float(in[10]));
        out[1] = lm_bits(v.d); out[2] = lm_bits(v.g); out[3] = lm_bits(v.mag);
        vote_bins(v, out + 4);
    }
};
constexpr uint64_t VOTE_FLOATS = 0xf0full, BINS_FLOATS = 0xf0ull;  // (the ranges are integers)
struct EvVoteBins {  // in: d g mag; out: ranges[4], terms[4]
    HD void operator()(const uint32_t* in, uint32_t* out) const {
        RiftVote v;
        v.d = lm_float(in[0]); v.g = lm_float(in[1]); v.mag = lm_float(in[2]);
        vote_bins(v, out);
    }
};
struct EvNorm {
    HD void operator()(const uint32_t* in, uint32_t* out) const {
        float h[RIFT_BINS];
        for (int j = 0; j < RIFT_BINS; ++j) h[j] = lm_float(in[j]);
        out[0] = lm_bits(rift_norm(h));
    }
};
struct EvRiftIntensity {
    HD void operator()(const uint32_t* in, uint32_t* out) const { out[0] = lm_bits(rift_intensity(in[0])); }
};
struct EvSiftIntensity {
    HD void operator()(const uint32_t* in, uint32_t* out) const { out[0] = lm_bits(sift_intensity(in[0])); }
};
struct EvSiftWeight {
    HD void operator()(const uint32_t* in, uint32_t* out) const { out[0] = lm_bits(sift_weight(lm_float(in[0]), lm_float(in[1]))); }
};
struct EvSiftResponse {
    HD void operator()(const uint32_t* in, uint32_t* out) const { out[0] = lm_bits(sift_response(lm_float(in[0]), lm_float(in[1]))); }
};
struct EvSiftDog {
    HD void operator()(const uint32_t* in, uint32_t* out) const { out[0] = lm_bits(sift_dog(lm_float(in[0]), lm_float(in[1]))); }
};
struct EvSiftKeypoint {
    HD void operator()(const uint32_t* in, uint32_t* out) const {
        float a[8];
        for (int j = 0; j < 8; ++j) a[j] = lm_float(in[j]);
        out[0] = sift_is_keypoint(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]) ? 1u : 0u;
    }
};
struct EvEig4 {  // in: the upper triangle of a symmetric 4x4 (10 words); out: v[4] and the rotated diagonal
    HD void operator()(const uint64_t* in, uint64_t* out) const {
        double A[4][4], v[4];
        int w = 0;
        for (int p = 0; p < 4; ++p)
            for (int q = p; q < 4; ++q) { A[p][q] = A[q][p] = lm_double(in[w]); ++w; }
        sym4_max_eigvec(A, v);
        for (int j = 0; j < 4; ++j) { out[j] = lm_bits64(v[j]); out[4 + j] = lm_bits64(A[j][j]); }
    }
};
struct EvRigid {  // in: sums[17] center[3] use_center; out: return value, T[16] (float bits), eigenvector[4]
    HD void operator()(const uint64_t* in, uint64_t* out) const {
        double sums[17], center[3];
        for (int j = 0; j < 17; ++j) sums[j] = lm_double(in[j]);
        for (int j = 0; j < 3; ++j) center[j] = lm_double(in[17 + j]);
        float T[16];
        for (int j = 0; j < 16; ++j) T[j] = 0.f;
        out[0] = (uint64_t)(int64_t)rigid_from_sums(sums, T, in[20] ? center : nullptr);
        // (T travels as float bits in 64-bit words: its NaNs are folded to one pattern here, x86 and gfx950 differ in the sign)
        for (int j = 0; j < 16; ++j) out[1 + j] = (lm_bits(T[j]) & 0x7fffffffu) > 0x7f800000u ? 0x7fc00000u : lm_bits(T[j]);
        // (the matrix rigid_from_sums hands to sym4_max_eigvec, restated, for the eigenvector stage)
        const double n = sums[16];
        if (n < 3) return;
        double pm[3], qm[3], S[3][3];
        for (int a = 0; a < 3; ++a) { pm[a] = sums[a] / n; qm[a] = sums[3 + a] / n; }
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) S[a][b] = sums[6 + b * 3 + a] - n * pm[a] * qm[b];
        double N[4][4] = {
            {S[0][0] + S[1][1] + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0]},
            {S[1][2] - S[2][1], S[0][0] - S[1][1] - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2]},
            {S[2][0] - S[0][2], S[0][1] + S[1][0], -S[0][0] + S[1][1] - S[2][2], S[1][2] + S[2][1]},
            {S[0][1] - S[1][0], S[2][0] + S[0][2], S[1][2] + S[2][1], -S[0][0] - S[1][1] + S[2][2]}};
        double qv[4];
        sym4_max_eigvec(N, qv);
        for (int j = 0; j < 4; ++j) out[17 + j] = lm_bits64(qv[j]);
    }
};
struct EvMat4 {
    HD void operator()(const uint32_t* in, uint32_t* out) const {
        float A[16], B[16], C[16];
        for (int j = 0; j < 16; ++j) { A[j] = lm_float(in[j]); B[j] = lm_float(in[16 + j]); }
        mat4_mul_f(A, B, C);
        for (int j = 0; j < 16; ++j) out[j] = lm_bits(C[j]);
    }
};

// ---- case generation ----------------------------------------------------------------------------------------------------
struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9e3779b97f4a7c15ull + 88172645463325252ull) {}
    uint64_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }  // [0, 1)
    double sym() { return 2.0 * uni() - 1.0; }                                     // [-1, 1)
    int below(int n) { return (int)(next() % (uint64_t)n); }
    double gauss() { return std::sqrt(-2.0 * std::log(1.0 - uni())) * std::cos(6.283185307179586 * uni()); }
};
static uint32_t fb(float f) { return lm_bits(f); }
static float bf(uint32_t u) { return lm_float(u); }

typedef Cases<uint32_t, 1, 1> Unary;
static void un_add(Unary& c, uint32_t u, int fam) { *c.add(fam) = u; }
static void un_window(Unary& c, uint32_t centre, int fam) {
    for (int d = -4096; d <= 4096; ++d) {
        const uint32_t u = centre + (uint32_t)d;
        un_add(c, u, fam);
        un_add(c, u ^ 0x80000000u, fam);
    }
}
// lo, lo + step, ... up to hi, each ORed with or_mask (filled on all threads: these are the long runs)
static void un_stride(Unary& c, uint64_t lo, uint64_t hi, uint32_t step, uint32_t or_mask, int fam) {
    const size_t cnt = (size_t)((hi - lo) / step + 1), base = c.n();
    c.in.resize(base + cnt);
    c.fam.resize(base + cnt, (uint8_t)fam);
    uint32_t* dst = c.in.data() + base;
    parallel_for(cnt, [=](size_t b, size_t e, unsigned) {
        for (size_t i = b; i < e; ++i) dst[i] = (uint32_t)(lo + i * step) | or_mask;
    });
}
// what every unary set shares: every 256th pattern, the short denormals, zeros, infinities, NaNs
static void un_common(Unary& c) {
    un_stride(c, 0, 0xffffffffull, 256, 0, 0);
    for (int s = 0; s < 23; ++s)
        for (uint32_t m = 1; m < 4096; m += 2) {
            const uint32_t u = m << s;
            if (u >= 0x00800000u) break;
            un_add(c, u, 1);
            un_add(c, u | 0x80000000u, 1);
        }
    for (uint32_t u : {0x00000000u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7fc00001u, 0x7fffffffu,
                       0xffffffffu, 0x7f800001u, 0xff800001u, 0x7fa00000u, 0xffa00000u, 0x7fbfffffu})
        un_add(c, u, 2);
}
static void un_range(Unary& c, uint32_t hi_bits, bool negative_too, bool negative_only = false) {
    if (!negative_only) un_stride(c, 0, hi_bits, 64, 0, 4);
    if (negative_too || negative_only) un_stride(c, 0, hi_bits, 64, 0x80000000u, 4);
}
static void gen_sincos(Unary& c) {
    un_common(c);
    for (uint32_t u : {fb(0x1p-12f), 0x3f490fdbu, fb(1.2f), fb(120.0f)}) un_window(c, u, 3);
    for (int n = 1; n <= 76; ++n) un_window(c, fb((float)(n * 1.5707963267948966)), 3);
    un_range(c, fb(1.2f), false);
}
static void gen_atan(Unary& c) {
    un_common(c);
    for (uint32_t u : {0x31000000u, 0x3ee00000u, 0x3f300000u, 0x3f980000u, 0x401c0000u, 0x4c000000u, 0x7f800000u}) un_window(c, u, 3);
}
static void gen_acos(Unary& c) {
    un_common(c);
    for (uint32_t u : {0x32800000u, fb(0.5f), fb(1.0f)}) un_window(c, u, 3);
    un_range(c, fb(1.0f), true);
}
static void gen_exp(Unary& c) {
    un_common(c);
    for (uint32_t u : {fb(88.0f), fb(0x1.62e42ep6f), fb(-0x1.9fe368p6f) & 0x7fffffffu}) un_window(c, u, 3);
    un_range(c, fb(4.5f), false, true);
    un_add(c, 0u, 4);
}

typedef Cases<uint32_t, 2, 1> Pairs;
static void pair_add(Pairs& c, float y, float x, int fam) {
    uint32_t* w = c.add(fam);
    w[0] = fb(y);
    w[1] = fb(x);
}
static void gen_atan2(Pairs& c) {
    const float sp[] = {0.f, -0.f, 1.f, -1.f, INFINITY, -INFINITY, NAN, 1e-45f, -1e-45f, 3.4e38f, -3.4e38f, 1e-30f, 1e30f, 0.5f, 2.f};
    for (float y : sp) for (float x : sp) pair_add(c, y, x, 0);
    Rng g(1);
    for (long i = 0; i < 4000000L; ++i) {  // the generator of tests/cpp/test_libm.cpp
        const uint64_t r = g.next();
        float y = bf((uint32_t)r), x = bf((uint32_t)(r >> 32));
        if (i & 1) {
            const int ey = (int)((fb(y) >> 23) & 0xff);
            int ex = ey + (int)((r >> 20) % 9) - 4;
            ex = ex < 1 ? 1 : (ex > 254 ? 254 : ex);
            x = bf((fb(x) & 0x807fffffu) | ((uint32_t)ex << 23));
        }
        pair_add(c, y, x, 1);
        pair_add(c, fabsf(y), x, 1);
    }
    for (long i = 0; i < 1000000L; ++i) {  // one or both operands denormal
        const uint64_t r = g.next();
        uint32_t y = (uint32_t)r, x = (uint32_t)(r >> 32);
        const int which = (int)(i % 3);
        if (which != 1) y &= 0x807fffffu;
        if (which != 0) x &= 0x807fffffu;
        if (which == 0 && (i & 4)) x = (x & 0x807fffffu) | ((uint32_t)(1 + (int)((r >> 13) % 30)) << 23);  // a small normal beside it
        pair_add(c, bf(y), bf(x), 2);
    }
    for (long i = 0; i < 1000000L; ++i) {  // exponents 58..62 apart, either way round: the k > 60 / k < -60 cut-offs
        const uint64_t r = g.next();
        const int diff = 58 + (int)((r >> 40) % 5);
        const int e_lo = 1 + (int)((r >> 48) % (uint64_t)(254 - diff)), e_hi = e_lo + diff;
        const bool y_big = (r >> 63) != 0;
        const uint32_t y = ((uint32_t)r & 0x807fffffu) | ((uint32_t)(y_big ? e_hi : e_lo) << 23);
        const uint32_t x = ((uint32_t)(r >> 9) & 0x807fffffu) | ((uint32_t)(y_big ? e_lo : e_hi) << 23);
        pair_add(c, bf(y), bf(x), 3);
    }
}

// -- plane fit --
// families of the plane-fit sets (the class counts of --host are printed per family under these names)
enum { PF_BLOB, PF_OFFSET, PF_PLANE, PF_LINE, PF_SAME, PF_ISO, PF_TWO_EQUAL, PF_DENORMAL, PF_NONFINITE, PF_C0_EDGE, PF_FAMILIES };
static const char* const PF_NAME[PF_FAMILIES] = {"blob", "offset1000", "plane", "line", "identical", "isotropic", "two_equal",
                                                 "denormal", "nonfinite", "c0_edge"};
typedef Cases<uint32_t, 10, 16> PlaneSums;
typedef Cases<uint32_t, 9, 7> PlaneCov;
static const int PF_K[5] = {3, 4, 5, 10, 50};

static void points_of(Rng& g, int fam, int k, float (*p)[3]) {
    const double size = std::ldexp(1.0, -g.below(8));
    switch (fam) {
    case PF_BLOB:
        for (int i = 0; i < k; ++i) for (int a = 0; a < 3; ++a) p[i][a] = (float)(g.sym() * size);
        break;
    case PF_OFFSET:
        for (int i = 0; i < k; ++i) for (int a = 0; a < 3; ++a) p[i][a] = (float)(1000.0 + g.sym() * size * 0.5);
        break;
    case PF_PLANE: {  // dyadic coordinates: axis-aligned (one constant coordinate) or x = y
        const int mode = g.below(4);
        const float c0 = (float)g.below(64) / 16.0f;
        for (int i = 0; i < k; ++i) {
            const float u = (float)(g.below(129) - 64) / 64.0f, v = (float)(g.below(129) - 64) / 64.0f;
            if (mode == 3) { p[i][0] = u; p[i][1] = u; p[i][2] = v; }
            else { p[i][mode] = c0; p[i][(mode + 1) % 3] = u; p[i][(mode + 2) % 3] = v; }
        }
        break;
    }
    case PF_LINE: {
        int d[3] = {g.below(9) - 4, g.below(9) - 4, g.below(9) - 4};
        if (!d[0] && !d[1] && !d[2]) d[g.below(3)] = 1;
        const int o[3] = {g.below(17) - 8, g.below(17) - 8, g.below(17) - 8};
        for (int i = 0; i < k; ++i) {
            const int t = g.below(33) - 16;
            for (int a = 0; a < 3; ++a) p[i][a] = (float)(o[a] * 4 + t * d[a]) / 4.0f;
        }
        break;
    }
    default: {  // PF_SAME: one point k times, dyadic or not
        float q[3];
        const bool dyadic = g.below(2) != 0;
        for (int a = 0; a < 3; ++a) q[a] = dyadic ? (float)(g.below(257) - 128) / 16.0f : (float)(g.sym() * 10.0);
        for (int i = 0; i < k; ++i) for (int a = 0; a < 3; ++a) p[i][a] = q[a];
    }
    }
}
static void sums_of(const float (*p)[3], int k, float a[9]) {
    for (int j = 0; j < 9; ++j) a[j] = 0.f;
    for (int i = 0; i < k; ++i) {
        const float x = p[i][0], y = p[i][1], z = p[i][2];
        a[0] += x * x; a[1] += x * y; a[2] += x * z; a[3] += y * y; a[4] += y * z; a[5] += z * z;
        a[6] += x; a[7] += y; a[8] += z;
    }
}
static void cov_add(PlaneCov& c, const float cov[9], int fam) {
    uint32_t* w = c.add(fam);
    for (int j = 0; j < 9; ++j) w[j] = fb(cov[j]);
}
static void cov_add_scaled(PlaneCov& c, const float cov[9], float s, int fam) {
    float m[9];
    for (int j = 0; j < 9; ++j) m[j] = cov[j] * s;
    cov_add(c, m, fam);
}
static void sym_from6(const float u[6], float m[9]) {  // xx xy xz yy yz zz
    m[0] = u[0]; m[1] = m[3] = u[1]; m[2] = m[6] = u[2]; m[4] = u[3]; m[5] = m[7] = u[4]; m[8] = u[5];
}
// pf_roots3's c0, restated: only to steer the c0_edge family and to count which of its cases take which path
static float c0_of(const float m[9]) {
    return m[0] * m[4] * m[8] + 2.f * m[1] * m[2] * m[5] - m[0] * m[5] * m[5] - m[4] * m[2] * m[2] - m[8] * m[1] * m[1];
}
// which way pf_roots3 went on the scaled matrix of cov, told from the inputs and the smallest root it returned: 0 = |c0| below
// FLT_EPSILON (pf_roots2 at once), 1 = the cubic's roots kept, 2 = the cubic's smallest root was <= 0 and pf_roots2 replaced
// them (it returns r[0] = 0 exactly, which the kept path never does)
static int root_path(const float cov[9], uint32_t root0_bits) {
    float scale = 0.f, sm[9];
    for (int j = 0; j < 9; ++j) scale = fmaxf(scale, fabsf(cov[j]));
    if (scale <= FLT_MIN) scale = 1.f;
    for (int j = 0; j < 9; ++j) sm[j] = cov[j] / scale;
    if (fabsf(c0_of(sm)) < FLT_EPSILON) return 0;
    return (root0_bits & 0x7fffffffu) == 0 ? 2 : 1;
}
static void gen_plane(PlaneSums& cs, PlaneCov& cc, long per_family) {
    Rng g(2);
    const float up = 0x1p100f, down = 0x1p-100f;
    // from sums; the same covariances (taken by the host pass of covariance_from_sums) scaled by 2^-100 and 2^+100
    for (int fam = PF_BLOB; fam <= PF_SAME; ++fam)
        for (long i = 0; i < per_family; ++i) {
            const int k = PF_K[i % 5];
            float p[50][3], a[9], cov[9];
            points_of(g, fam, k, p);
            sums_of(p, k, a);
            uint32_t* w = cs.add(fam);
            for (int j = 0; j < 9; ++j) w[j] = fb(a[j]);
            w[9] = (uint32_t)k;
            covariance_from_sums(a, (unsigned)k, cov);
            cov_add_scaled(cc, cov, down, fam);
            cov_add_scaled(cc, cov, up, fam);
            if (fam == PF_BLOB) {
                if (i & 1) cov_add_scaled(cc, cov, std::ldexp(1.f, -120 - g.below(28)), PF_DENORMAL);
                else {  // one entry (and its mirror) NaN or +-Inf
                    float u[6] = {cov[0], cov[1], cov[2], cov[4], cov[5], cov[8]}, m[9];
                    const float v[3] = {NAN, INFINITY, -INFINITY};
                    u[g.below(6)] = v[g.below(3)];
                    sym_from6(u, m);
                    cov_add(cc, m, PF_NONFINITE);
                }
            }
        }
    for (long i = 0; i < per_family; ++i) {  // isotropic diagonals: a triple root
        const float s = (i & 1) ? std::ldexp(1.f, g.below(41) - 20) : (float)(g.uni() * 10.0 + 1e-3);
        const float m[9] = {s, 0, 0, 0, s, 0, 0, 0, s};
        cov_add(cc, m, PF_ISO);
        cov_add_scaled(cc, m, down, PF_ISO);
        cov_add_scaled(cc, m, up, PF_ISO);
    }
    for (long i = 0; i < per_family; ++i) {  // two equal eigenvalues: diag(a, a, b) in any order, or turned 45 degrees in a plane
        const float a = (float)(g.uni() + 0.01), b = (i & 2) ? a * (float)(1.0 + g.uni()) : (float)(g.uni() + 0.01);
        float m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        const int odd = g.below(3), o1 = (odd + 1) % 3, o2 = (odd + 2) % 3;
        m[odd * 4] = b; m[o1 * 4] = a; m[o2 * 4] = a;
        if (i & 1) {  // rotate b's axis and o1 by 45 degrees: [[(a+b)/2, (b-a)/2], [(b-a)/2, (a+b)/2]], eigenvalues still a, a, b up to rounding
            m[odd * 4] = m[o1 * 4] = 0.5f * (a + b);
            m[odd * 3 + o1] = m[o1 * 3 + odd] = 0.5f * (b - a);
        }
        cov_add(cc, m, PF_TWO_EQUAL);
        cov_add_scaled(cc, m, down, PF_TWO_EQUAL);
        cov_add_scaled(cc, m, up, PF_TWO_EQUAL);
    }
    // c0 within +-8 ulp of +-FLT_EPSILON: the largest entry is m[0] = 1 (so the scaled matrix is the matrix), m[8] is steered
    for (long i = 0; i < per_family / 17 + 1; ++i) {
        float u[6] = {1.f, 0.f, 0.f, (float)(0.1 + 0.9 * g.uni()), 0.f, 0.f}, m[9];
        if (i & 1) { u[1] = (float)(g.sym() * 0x1p-7); u[2] = (float)(g.sym() * 0x1p-7); u[4] = (float)(g.sym() * 0x1p-7); }
        const float target = (i & 2) ? -FLT_EPSILON : FLT_EPSILON;
        sym_from6(u, m);
        m[8] = 0.f;
        const double base = c0_of(m), slope = (double)m[0] * m[4] - (double)m[1] * m[1];
        m[8] = (float)((target - base) / slope);
        for (int it = 0; it < 8; ++it) {  // walk m[8] until the float c0 lands on the target
            const int32_t off = (int32_t)(fb(fabsf(c0_of(m))) - fb(FLT_EPSILON));
            if (off == 0) break;
            const double step = ((double)target - (double)c0_of(m)) / slope;
            const float next = (float)((double)m[8] + step);
            m[8] = next != m[8] ? next : std::nextafterf(m[8], step > 0 ? INFINITY : -INFINITY);
        }
        const uint32_t centre = fb(m[8]);
        for (int d = -8; d <= 8; ++d) {
            m[8] = bf(centre + (uint32_t)d);
            cov_add(cc, m, PF_C0_EDGE);
        }
    }
}

// -- rift_solve3 --
enum { S3_RANDOM, S3_RANK0, S3_RANK1, S3_RANK2, S3_DIAGONAL, S3_EQUAL_NORMS, S3_TAIL0_STEP0, S3_TAIL0_STEP1, S3_PIVOT_EDGE, S3_EXTREME, S3_FAMILIES };
static const char* const S3_NAME[S3_FAMILIES] = {"random", "rank0", "rank1", "rank2", "diagonal", "equal_norms", "tail0_step0",
                                                 "tail0_step1", "pivot_edge", "extreme"};
typedef Cases<uint32_t, 9, 3> Solve3;
static void s3_add(Solve3& c, const float a[6], Rng& g, int fam, float bscale = 1.f) {
    uint32_t* w = c.add(fam);
    for (int j = 0; j < 6; ++j) w[j] = fb(a[j]);
    for (int j = 0; j < 3; ++j) w[6 + j] = fb((float)(g.uni() + 0.25) * (g.below(2) ? bscale : -bscale));  // never 0: a solved unknown shows
}
static void outer_add(float a[6], const int v[3], float s) {
    a[0] += s * v[0] * v[0]; a[1] += s * v[0] * v[1]; a[2] += s * v[0] * v[2];
    a[3] += s * v[1] * v[1]; a[4] += s * v[1] * v[2]; a[5] += s * v[2] * v[2];
}
static void gen_solve3(Solve3& c, long per_family) {
    Rng g(3);
    for (long i = 0; i < per_family; ++i) {
        float a[6];
        for (int j = 0; j < 6; ++j) a[j] = (float)g.sym();
        s3_add(c, a, g, S3_RANDOM);
        const float zero[6] = {0, 0, 0, 0, 0, 0};
        if (i % 16 == 0) s3_add(c, zero, g, S3_RANK0);
        int u[3], v[3];
        do { for (int j = 0; j < 3; ++j) { u[j] = g.below(9) - 4; v[j] = g.below(9) - 4; } }
        while ((!u[0] && !u[1] && !u[2]) || (u[1] * v[2] == u[2] * v[1] && u[2] * v[0] == u[0] * v[2] && u[0] * v[1] == u[1] * v[0]));
        const float s = std::ldexp(1.f, g.below(21) - 10);
        float r1[6] = {0, 0, 0, 0, 0, 0}, r2[6] = {0, 0, 0, 0, 0, 0};
        outer_add(r1, u, s);
        s3_add(c, r1, g, S3_RANK1);
        outer_add(r2, u, s); outer_add(r2, v, s);
        s3_add(c, r2, g, S3_RANK2);
        {   // diagonal, entries from a short list so that zeros and equal entries are frequent
            const float pick[6] = {0.f, 1.f, -1.f, 0.5f, (float)g.sym(), (float)g.sym() * 100.f};
            const float d[6] = {pick[g.below(6)], 0, 0, pick[g.below(6)], 0, pick[g.below(6)]};
            s3_add(c, d, g, S3_DIAGONAL);
        }
        {   // equal column norms: a b b / b a b / b b a, permutation matrices, the all-equal matrix
            const float x = (float)g.sym(), y = (float)g.sym();
            const float circ[6] = {x, y, y, x, y, x}, perm[6] = {0, x, 0, 0, 0, x}, perm2[6] = {0, 0, x, x, 0, 0}, all[6] = {x, x, x, x, x, x};
            const int m = (int)(i % 4);
            s3_add(c, m == 0 ? circ : m == 1 ? perm : m == 2 ? perm2 : all, g, S3_EQUAL_NORMS);
        }
        {   // nothing below the first pivot: a 0 0 / 0 d e / 0 e f with |a| the largest column norm
            const float t0[6] = {(float)(2.0 + g.uni()) * (g.below(2) ? 1.f : -1.f), 0, 0, (float)g.sym(), (float)g.sym(), (float)g.sym()};
            s3_add(c, t0, g, S3_TAIL0_STEP0);
            // nothing below the second pivot: a b 0 / b d 0 / 0 0 f with |f| small
            const float t1[6] = {(float)(1.0 + g.uni()), (float)g.sym(), 0, (float)(1.0 + g.uni()), 0, (float)(g.sym() * 0.25)};
            s3_add(c, t1, g, S3_TAIL0_STEP1);
        }
        {   // pivots a few ulp around eps * 3 * |r00|, on diagonals (the pivots are then the entries themselves)
            const float r00 = (i & 1) ? 1.f : (float)(0.5 + g.uni() * 100.0) * (g.below(2) ? 1.f : -1.f);
            const float thr = fabsf(r00) * (RIFT_EPS * 3.0f);
            const uint32_t e1 = fb(thr) + (uint32_t)(g.below(9) - 4), e2 = fb(thr) + (uint32_t)(g.below(9) - 4);
            const float big = 0.5f * fabsf(r00);
            const float second = (i & 2) ? bf(e1) * (g.below(2) ? 1.f : -1.f) : big;
            const float d[6] = {r00, 0, 0, second, 0, bf(e2) * (g.below(2) ? 1.f : -1.f)};
            s3_add(c, d, g, S3_PIVOT_EDGE);
        }
        {   // huge, tiny and denormal entries: squares that overflow, underflow to denormals or to zero
            static const int EXPO[6] = {60, 70, -60, -70, -75, -140};
            const int e = EXPO[i % 6];
            float x[6];
            for (int j = 0; j < 6; ++j) x[j] = std::ldexp((float)g.sym(), e);
            s3_add(c, x, g, S3_EXTREME, std::ldexp(1.f, e));
        }
    }
}

// -- rift_vote --
enum { RV_RANDOM, RV_SELF, RV_ZERO_GRADIENT, RV_PARALLEL, RV_D2_EDGE, RV_FAMILIES };
static const char* const RV_NAME[RV_FAMILIES] = {"random", "self", "zero_gradient", "parallel", "d2_edge"};
typedef Cases<uint32_t, 11, 12> Votes;
static void gen_votes(Votes& c, long per_family) {
    Rng g(4);
    for (long i = 0; i < per_family; ++i)
        for (int fam = 0; fam < RV_FAMILIES; ++fam) {
            const float radius = (float)(0.01 + g.uni());
            float p0[3], p[3], gv[3];
            for (int a = 0; a < 3; ++a) {
                p0[a] = (float)(g.sym() * 5.0);
                p[a] = p0[a] + (float)(g.sym() * radius * 0.57);
                gv[a] = (float)(g.sym() * 50.0);
            }
            float ex = p[0] - p0[0], ey = p[1] - p0[1], ez = p[2] - p0[2];
            float d2 = (ex * ex + ey * ey) + ez * ez;
            if (fam == RV_SELF) { for (int a = 0; a < 3; ++a) p[a] = p0[a]; d2 = 0.f; }
            if (fam == RV_ZERO_GRADIENT) for (int a = 0; a < 3; ++a) gv[a] = (i & 1) ? 0.f : -0.f;
            if (fam == RV_PARALLEL) {  // the gradient is the edge itself times +-2^e (exact), or times any factor (rounded)
                const float s = ((i & 1) ? std::ldexp(1.f, g.below(21) - 10) : (float)(g.uni() * 100.0 + 0.01)) * ((i & 2) ? -1.f : 1.f);
                gv[0] = ex * s; gv[1] = ey * s; gv[2] = ez * s;
            }
            if (fam == RV_D2_EDGE) {
                const float r2 = radius * radius;
                d2 = (i % 3 == 0) ? 0.f : bf(fb(r2) + (uint32_t)(g.below(9) - 4));
                if (i % 3 == 2) d2 = bf((uint32_t)g.below(16));  // 0 and the first denormals
            }
            uint32_t* w = c.add(fam);
            for (int a = 0; a < 3; ++a) { w[a] = fb(p0[a]); w[3 + a] = fb(p[a]); w[6 + a] = fb(gv[a]); }
            w[9] = fb(d2);
            w[10] = fb(radius);
        }
}
typedef Cases<uint32_t, 3, 8> VoteBins;
static void gen_vote_bins(VoteBins& c, long n) {
    Rng g(5);
    for (long i = 0; i < n; ++i) {
        // d in [0, 4], g in [0, 8]; two thirds of them an integer +- up to 2 ulp, where ceilf and floorf sit on their edges
        float d = (float)(g.uni() * 4.0), gg = (float)(g.uni() * 8.0);
        if (i % 3 != 0) d = bf(fb((float)g.below(5)) + (uint32_t)(g.below(5) - 2));
        if (i % 3 != 1) gg = bf(fb((float)g.below(9)) + (uint32_t)(g.below(5) - 2));
        if (fb(d) > 0xff000000u) d = 0.f;   // (0 minus an ulp wrapped round: keep the conversions to int defined)
        if (fb(gg) > 0xff000000u) gg = 0.f;
        uint32_t* w = c.add(0);
        w[0] = fb(d); w[1] = fb(gg); w[2] = fb((float)(g.uni() * 100.0));
    }
}

static float pick_special(Rng& g, float ordinary) {
    const float sp[8] = {NAN, INFINITY, -INFINITY, 0.f, -0.f, 1e-45f, 3.4e38f, -3.4e38f};
    return g.below(16) == 0 ? sp[g.below(8)] : ordinary;
}

int main(int argc, char** argv) {
    g_host_only = argc > 1 && std::string(argv[1]) == "--host";
    if (argc > 1 && !g_host_only) { std::printf("usage: test_device_math [--host]\n"); return 2; }
    if (!g_host_only) {
        int ndev = 0;
        HIP_OK(hipGetDeviceCount(&ndev));
        hipDeviceProp_t prop;
        HIP_OK(hipGetDeviceProperties(&prop, 0));  // (fails where there is no device, whatever the count says)
        std::printf("device: %s %s\n", prop.name, prop.gcnArchName);
    }
    unsigned long libm_bad = 0;
    const bool have_fma = __builtin_cpu_supports("fma");

    // ---- libm_f32.hpp ----
    // the host pass against this machine's libm: ref(case) gives libm's bits, skip(case) leaves a case out
    auto against_libm = [&](const char* name, size_t n, const uint32_t* in, int ni, const uint32_t* host, auto ref, auto skip) {
        unsigned long bad[16] = {}, checked[16] = {};
        size_t first[16];
        parallel_for(n, [&](size_t b, size_t e, unsigned t) {
            first[t] = n;
            for (size_t i = b; i < e; ++i) {
                if (skip(i)) continue;
                ++checked[t];
                const uint32_t want = ref(i), got = host[i];
                if (want != got && !(word_nan(want) && word_nan(got)) && bad[t]++ == 0) first[t] = i;
            }
        });
        unsigned long nb = 0, nc = 0;
        for (int t = 0; t < 16; ++t) {
            nb += bad[t]; nc += checked[t];
            if (first[t] < n) {
                std::printf("  %s(", name);
                for (int j = 0; j < ni; ++j) std::printf("%s%a", j ? ", " : "", bf(in[first[t] * ni + j]));
                std::printf("): libm %a restated %a\n", bf(ref(first[t])), bf(host[first[t]]));
            }
        }
        std::printf("%s against libm: %lu cases, %lu mismatches\n", name, nc, nb);
        libm_bad += nb;
    };
    auto unary = [&](const char* name, Unary& c, auto ev, float (*ref)(float), bool sincos) {
        run(name, c, ev);
        if (!g_host_only) return;
        // (beyond the callers' range glibc's FMA build and its baseline build differ for one argument in two million: the
        // restatement follows the FMA build, as in tests/cpp/test_libm.cpp)
        against_libm(name, c.n(), c.in.data(), 1, c.host.data(), [&](size_t i) { return fb(ref(bf(c.in[i]))); },
                     [&](size_t i) { return sincos && !have_fma && !(fabsf(bf(c.in[i])) <= 1.2f); });
    };
    { Unary c; gen_sincos(c); unary("lm_sinf", c, EvSin(), sinf, true); unary("lm_cosf", c, EvCos(), cosf, true); }
    { Unary c; gen_atan(c); unary("lm_atanf", c, EvAtan(), atanf, false); }
    { Unary c; gen_acos(c); unary("lm_acosf", c, EvAcos(), acosf, false); }
    { Unary c; gen_exp(c); unary("lm_expf", c, EvExp(), expf, false); }
    {
        Pairs c;
        gen_atan2(c);
        run("lm_atan2f", c, EvAtan2());
        if (g_host_only)
            against_libm("lm_atan2f", c.n(), c.in.data(), 2, c.host.data(), [&](size_t i) { return fb(atan2f(bf(c.in[2 * i]), bf(c.in[2 * i + 1]))); },
                         [](size_t) { return false; });
    }

    // ---- plane_fit.hpp ----
    {
        Cases<uint32_t, 2, 3> c;
        Rng g(6);
        for (long i = 0; i < 400000L; ++i) {
            uint32_t* w = c.add(0);
            float b = (float)(g.sym() * 3.0), cc = (float)(g.sym() * 3.0);
            if (i % 4 == 1) cc = 0.25f * b * b;                                   // d = 0 up to rounding
            if (i % 4 == 2) cc = bf(fb(0.25f * b * b) + (uint32_t)(g.below(9) - 4));  // d a few ulp either side of 0
            if (i % 4 == 3) { b = pick_special(g, b); cc = pick_special(g, std::ldexp(cc, -130)); }
            w[0] = fb(b); w[1] = fb(cc);
        }
        run("pf_roots2", c, EvRoots2());
    }
    {
        PlaneSums cs;
        PlaneCov cc;
        gen_plane(cs, cc, 100000L);
        run("plane_from_sums", cs, EvPlaneSums());
        run("plane_from_covariance", cc, EvPlaneCov());
        if (g_host_only) {
            // classes per family: curvature exactly 0, NaN normal, finite normal; negative or zero variances of the covariance
            // (from sums only); and which root path the case took (root_path)
            unsigned long cls[2][PF_FAMILIES][7] = {};
            for (size_t i = 0; i < cs.n(); ++i) {
                const uint32_t* o = cs.host.data() + i * 16;
                unsigned long* k = cls[0][cs.fam[i]];
                k[0] += (o[15] & 0x7fffffffu) == 0;
                const bool nan_n = word_nan(o[12]) || word_nan(o[13]) || word_nan(o[14]);
                k[1] += nan_n; k[2] += !nan_n;
                k[3] += bf(o[0]) <= 0.f || bf(o[4]) <= 0.f || bf(o[8]) <= 0.f;
                float m[9];
                for (int j = 0; j < 9; ++j) m[j] = bf(o[j]);
                ++k[4 + root_path(m, o[9])];
            }
            for (size_t i = 0; i < cc.n(); ++i) {
                const uint32_t* o = cc.host.data() + i * 7;
                unsigned long* k = cls[1][cc.fam[i]];
                k[0] += (o[6] & 0x7fffffffu) == 0;
                const bool nan_n = word_nan(o[3]) || word_nan(o[4]) || word_nan(o[5]);
                k[1] += nan_n; k[2] += !nan_n;
                float m[9];
                for (int j = 0; j < 9; ++j) m[j] = bf(cc.in[i * 9 + j]);
                ++k[4 + root_path(m, o[0])];
            }
            for (int f = 0; f <= PF_SAME; ++f)
                std::printf("class plane_from_sums %s: curvature0 %lu nan_normal %lu finite_normal %lu nonpositive_variance %lu roots2_path %lu cubic_path %lu cubic_fallback %lu\n",
                            PF_NAME[f], cls[0][f][0], cls[0][f][1], cls[0][f][2], cls[0][f][3], cls[0][f][4], cls[0][f][5], cls[0][f][6]);
            for (int f = 0; f < PF_FAMILIES; ++f)
                std::printf("class plane_from_covariance %s: curvature0 %lu nan_normal %lu finite_normal %lu roots2_path %lu cubic_path %lu cubic_fallback %lu\n",
                            PF_NAME[f], cls[1][f][0], cls[1][f][1], cls[1][f][2], cls[1][f][4], cls[1][f][5], cls[1][f][6]);
        }
    }

    // ---- rift_math.hpp ----
    {
        Solve3 c;
        gen_solve3(c, 120000L);
        run("rift_solve3", c, EvSolve3());
        if (g_host_only) {
            // the right-hand sides are never 0, so a solved unknown is non-zero (or NaN): their number is the rank taken
            unsigned long cls[S3_FAMILIES][4] = {};
            for (size_t i = 0; i < c.n(); ++i) {
                int r = 0;
                for (int j = 0; j < 3; ++j) r += (c.host[i * 3 + j] & 0x7fffffffu) != 0;
                ++cls[c.fam[i]][r];
            }
            for (int f = 0; f < S3_FAMILIES; ++f)
                std::printf("class rift_solve3 %s: rank0 %lu rank1 %lu rank2 %lu rank3 %lu\n", S3_NAME[f], cls[f][0], cls[f][1], cls[f][2], cls[f][3]);
        }
    }
    {
        Cases<uint32_t, 6, 3> c;
        Rng g(7);
        for (long i = 0; i < 200000L; ++i) {
            uint32_t* w = c.add(0);
            double n[3] = {g.gauss(), g.gauss(), g.gauss()};
            const double l = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            for (int a = 0; a < 3; ++a) {
                w[a] = fb(i % 8 == 7 ? pick_special(g, (float)(n[a] / l)) : (float)(n[a] / l));
                w[3 + a] = fb(i % 8 == 6 ? pick_special(g, (float)g.sym()) : (float)(g.sym() * 100.0));
            }
        }
        run("rift_project", c, EvProject());
    }
    {
        Votes c;
        gen_votes(c, 180000L);
        run("rift_vote", c, EvVote(), VOTE_FLOATS);
        if (g_host_only) {
            unsigned long reset[RV_FAMILIES] = {}, cnt[RV_FAMILIES] = {}, total = 0;
            for (size_t i = 0; i < c.n(); ++i) {
                const bool r = !rift_finite(bf(c.host[i * 12]));
                reset[c.fam[i]] += r; ++cnt[c.fam[i]]; total += r;
            }
            for (int f = 0; f < RV_FAMILIES; ++f) std::printf("class rift_vote %s: angle_reset %lu kept %lu\n", RV_NAME[f], reset[f], cnt[f] - reset[f]);
            std::printf("rift_vote: %lu votes had the angle reset to 0\n", total);
        }
    }
    {
        VoteBins c;
        gen_vote_bins(c, 300000L);
        run("rift_vote_bins", c, EvVoteBins(), BINS_FLOATS);
    }
    {
        Cases<uint32_t, 32, 1> c;
        Rng g(8);
        for (long i = 0; i < 200000L; ++i) {
            uint32_t* w = c.add(0);
            const int mode = (int)(i % 8);
            const float s = mode == 5 ? 0x1p60f : mode == 6 ? 0x1p-70f : mode == 7 ? 0x1p-140f : 1.f;
            for (int j = 0; j < 32; ++j) w[j] = fb(mode == 4 ? 0.f : (float)(g.uni() * 40.0) * s * (g.below(4) ? 1.f : 0.f));
        }
        run("rift_norm", c, EvNorm());
    }
    {
        Unary c;
        un_stride(c, 0, 0xffffffu, 1, 0, 0);
        run("rift_intensity", c, EvRiftIntensity());
        run("sift_intensity", c, EvSiftIntensity());
    }

    // ---- sift_math.hpp ----
    {
        Pairs c;
        Rng g(9);
        for (int e = -40; e <= 40; e += 4)           // the grid: ratios through [0, 9], sigma2 over 80 binades
            for (int q = 0; q <= 9000; ++q) {
                const float sigma2 = std::ldexp((float)(1.0 + g.uni()), e);
                pair_add(c, (float)(q * 1e-3) * sigma2, sigma2, 0);
            }
        for (long i = 0; i < 400000L; ++i) {
            const float sigma2 = std::ldexp((float)(1.0 + g.uni()), g.below(41) - 20), cut = sift_cut(sigma2);
            pair_add(c, (float)(g.uni() * 9.0) * sigma2, sigma2, 0);
            pair_add(c, i & 1 ? bf(fb(cut) + (uint32_t)g.below(64)) : (float)(9.0 + g.uni() * 200.0) * sigma2, sigma2, 1);  // just beyond 9, and far
            pair_add(c, i % 4 == 0 ? 0.f : (float)g.uni() * bf((uint32_t)g.next() & 0x00ffffffu), bf((uint32_t)g.next() & 0x007fffffu), 2);  // sigma2 denormal (or 0)
            if (i % 4 == 0) pair_add(c, i & 4 ? 0.f : -0.f, pick_special(g, sigma2), 3);  // d2 = 0
        }
        run("sift_weight", c, EvSiftWeight());
    }
    {
        Pairs resp, dog;
        Rng g(10);
        for (long i = 0; i < 500000L; ++i) {
            const float den = (float)(g.uni() * 30.0), num = (float)(g.sym() * 255.0) * den;
            if (i % 4 == 0) pair_add(resp, pick_special(g, num), i & 4 ? 0.f : -0.f, 1);  // den = 0: x / 0 and 0 / 0
            else if (i % 4 == 1) pair_add(resp, pick_special(g, num), pick_special(g, den), 2);
            else pair_add(resp, num, i % 4 == 2 ? den : std::ldexp(den, -140), 0);
            const float a = (float)(g.uni() * 255.0), b = i % 4 == 3 ? a : i % 4 == 2 ? bf(fb(a) + (uint32_t)(g.below(9) - 4)) : (float)(g.uni() * 255.0);
            pair_add(dog, i % 8 == 1 ? pick_special(g, a) : a, i % 8 == 5 ? pick_special(g, b) : b, 0);
        }
        run("sift_response", resp, EvSiftResponse());
        run("sift_dog", dog, EvSiftDog());
    }
    {
        Cases<uint32_t, 8, 1> c;
        Rng g(11);
        for (long i = 0; i < 1000000L; ++i) {
            // every operand from one short pool: ties v == min, |v| at min_contrast and an ulp either side, NaN in each position
            const float mc = (float)(0.001 + g.uni() * 0.1), x = (float)(g.sym() * 0.2);
            const float pool[12] = {mc, -mc, bf(fb(mc) + 1), bf(fb(mc) - 1), -bf(fb(mc) + 1), x, x, -x, 2.f * mc, -2.f * mc, 0.f, NAN};
            uint32_t* w = c.add(0);
            for (int j = 0; j < 7; ++j) w[j] = fb(pool[g.below(g.below(8) ? 11 : 12)]);
            w[7] = fb(i % 64 == 0 ? NAN : i % 64 == 1 ? 0.f : mc);
        }
        run("sift_is_keypoint", c, EvSiftKeypoint(), 0);
        if (g_host_only) {
            unsigned long yes = 0;
            for (size_t i = 0; i < c.n(); ++i) yes += c.host[i] != 0;
            std::printf("class sift_is_keypoint pool: keypoint %lu not_keypoint %lu\n", yes, (unsigned long)c.n() - yes);
        }
    }

    // ---- rigid_solve.hpp ----
    {
        Cases<uint64_t, 10, 8> c;
        Rng g(12);
        for (long i = 0; i < 200000L; ++i) {
            uint64_t* w = c.add(0);
            const int mode = (int)(i % 8);
            const double s = mode == 5 ? 1e150 : mode == 6 ? 1e-150 : 1.0;
            for (int j = 0; j < 10; ++j) w[j] = lm_bits64(g.sym() * s);
            if (mode == 3) for (int j : {1, 2, 3, 5, 6, 8}) w[j] = lm_bits64(0.0);          // already diagonal
            if (mode == 4) for (int j = 0; j < 10; ++j) w[j] = lm_bits64(0.0);               // the zero matrix
            if (mode == 7) for (int j : {0, 4, 7, 9}) w[j] = w[0];                          // equal diagonal: theta = 0
        }
        run("sym4_max_eigvec", c, EvEig4());
    }
    {
        enum { RG_ROTATION, RG_IDENTITY, RG_HALF_TURN, RG_COPLANAR, RG_COLLINEAR, RG_FEW, RG_ZERO, RG_FAR_CENTRE, RG_HUGE, RG_FAMILIES };
        static const char* const RG_NAME[RG_FAMILIES] = {"rotation", "identity", "half_turn", "coplanar", "collinear", "few", "zero", "far_centre", "huge"};
        Cases<uint64_t, 21, 21> c;
        Rng g(13);
        for (long i = 0; i < 20000L; ++i)
            for (int fam = 0; fam < RG_FAMILIES; ++fam)
                for (int use_centre = 0; use_centre < 2; ++use_centre) {
                    double q4[4] = {g.gauss(), g.gauss(), g.gauss(), g.gauss()};
                    if (fam == RG_IDENTITY) { q4[0] = 1; q4[1] = q4[2] = q4[3] = 0; }
                    if (fam == RG_HALF_TURN) {
                        q4[0] = 0;
                        if (i & 1) { q4[1] = q4[2] = q4[3] = 0; q4[1 + (int)(i / 2 % 3)] = 1; }  // about an axis: R = diag(+1, -1, -1) exactly
                    }
                    const double l = std::sqrt(q4[0] * q4[0] + q4[1] * q4[1] + q4[2] * q4[2] + q4[3] * q4[3]);
                    const double w = q4[0] / l, x = q4[1] / l, y = q4[2] / l, z = q4[3] / l;
                    const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)},
                                            {2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)},
                                            {2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)}};
                    const double t[3] = {g.sym(), g.sym(), g.sym()};
                    const double centre[3] = {fam == RG_FAR_CENTRE ? 1e6 : g.sym() * 10, fam == RG_FAR_CENTRE ? -1e6 : g.sym() * 10,
                                              fam == RG_FAR_CENTRE ? 1e6 : g.sym() * 10};
                    int m = 3 + g.below(48);
                    if (fam == RG_FEW) m = g.below(3);
                    const bool noisy = (i & 4) != 0 && fam != RG_IDENTITY;
                    double sums[17] = {0};
                    const double dir[3] = {g.sym(), g.sym(), g.sym()};
                    for (int k = 0; k < m; ++k) {
                        // float coordinates, as the kernels sum them; relative to the centre where one is used
                        float p[3] = {(float)g.sym(), (float)g.sym(), (float)g.sym()}, q[3];
                        if (fam == RG_COPLANAR) p[2] = 0.25f;
                        if (fam == RG_COLLINEAR) { const double s = g.sym(); for (int a = 0; a < 3; ++a) p[a] = (float)(s * dir[a]); }
                        for (int a = 0; a < 3; ++a)
                            q[a] = (float)(R[a][0] * p[0] + R[a][1] * p[1] + R[a][2] * p[2] + t[a] + (noisy ? g.sym() * 1e-3 : 0.0));
                        if (fam == RG_IDENTITY) for (int a = 0; a < 3; ++a) q[a] = p[a];
                        double e2 = 0;
                        for (int a = 0; a < 3; ++a) {
                            sums[a] += p[a]; sums[3 + a] += q[a];
                            for (int b = 0; b < 3; ++b) sums[6 + b * 3 + a] += (double)p[a] * q[b];
                            e2 += ((double)p[a] - q[a]) * ((double)p[a] - q[a]);
                        }
                        sums[15] += e2;
                        sums[16] += 1;
                    }
                    if (fam == RG_ZERO) { for (int j = 0; j < 16; ++j) sums[j] = 0; if (i & 1) sums[16] = 0; }
                    if (fam == RG_HUGE) for (int j = 0; j < 16; ++j) sums[j] *= (i & 1) ? 1e300 : 1e150;
                    uint64_t* wds = c.add(fam);
                    for (int j = 0; j < 17; ++j) wds[j] = lm_bits64(sums[j]);
                    for (int a = 0; a < 3; ++a) wds[17 + a] = lm_bits64(centre[a]);
                    wds[20] = (uint64_t)use_centre;
                }
        run("rigid_from_sums", c, EvRigid(), 0x1e0000ull);
        if (g_host_only) {
            unsigned long cls[RG_FAMILIES][4] = {};
            for (size_t i = 0; i < c.n(); ++i) {
                const uint64_t* o = c.host.data() + i * 21;
                bool nan_t = false, inf_t = false;
                for (int j = 1; j <= 16; ++j) { nan_t |= word_nan((uint32_t)o[j]); inf_t |= ((uint32_t)o[j] & 0x7fffffffu) == 0x7f800000u; }
                ++cls[c.fam[i]][o[0] != 0 ? 0 : nan_t ? 1 : inf_t ? 2 : 3];
            }
            for (int f = 0; f < RG_FAMILIES; ++f)
                std::printf("class rigid_from_sums %s: refused %lu nan_transform %lu inf_transform %lu finite_transform %lu\n", RG_NAME[f], cls[f][0],
                            cls[f][1], cls[f][2], cls[f][3]);
        }
    }
    {
        Cases<uint32_t, 32, 16> c;
        Rng g(14);
        for (long i = 0; i < 300000L; ++i) {
            uint32_t* w = c.add(0);
            for (int j = 0; j < 32; ++j) {
                const float v = (float)(g.sym() * (i % 4 == 1 ? 1e20 : 2.0));
                w[j] = fb(i % 4 >= 2 ? pick_special(g, v) : v);
            }
        }
        run("mat4_mul_f", c, EvMat4());
    }

    if (g_host_only) {
        std::printf("host math: %lu mismatches against libm\n", libm_bad);
        return libm_bad != 0;
    }
    std::printf("device math: %lu mismatches\n", g_total_bad);
    return g_total_bad != 0;
}
