// rift_host.cpp -- the RIFT descriptor pipeline of pcc_rift_descriptors on the CPU, one core: the arithmetic of
// csrc/rift_math.hpp and csrc/plane_fit.hpp (the headers the kernels are built from) over EXHAUSTIVE sorted radius rows.
// Test infrastructure (tests/test_rift_cpu.py, tests/test_rift_gpu.py, tools/exp_rift.py): the library does not link it.
//   stages (reference src/comparator.cpp:590-684): intensity; normals at normal_radius, viewpoint origin; points without a
//   finite normal leave (cloud2); intensity gradient over the rows of cloud2 at gradient_radius; RIFT 4 x 8 over the rows of
//   cloud2 at rift_radius; descriptors whose first bin is not finite leave.
// usage: rift_host IN OUT [normal_radius gradient_radius rift_radius]
//   IN : int32 n, then n records (float x, y, z; uint32 colour word, bytes b g r a)
//   OUT: int32 n_out, n_out x 32 floats, n_out x int32 original point indices
//        rift_host --self OUT   a built-in 240-point cloud with duplicates, isolated and non-finite points (`make asan`)
// prints "rift_host n=.. kept=.. ms=.." (the pipeline alone, no file I/O)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "plane_fit.hpp"
#include "rift_math.hpp"

namespace {

struct Rec {
    float x, y, z;
    uint32_t bgra;
};
struct Entry {
    float d2;
    int32_t j;
};
struct Rows {
    std::vector<size_t> off;
    std::vector<Entry> e;
};

bool finite3(const Rec& p) { return pcc::rift_finite(p.x) && pcc::rift_finite(p.y) && pcc::rift_finite(p.z); }

// sorted radius rows of every point against every point: d2 < float(r * r), ascending (d2, index), FLANN's L2_Simple sum
Rows radius_rows(const std::vector<Rec>& c, double radius) {
    const float r2 = (float)(radius * radius);
    const size_t n = c.size();
    Rows rows;
    rows.off.assign(n + 1, 0);
    std::vector<Entry> row;
    for (size_t i = 0; i < n; ++i) {
        row.clear();
        if (finite3(c[i]))
            for (size_t j = 0; j < n; ++j) {
                if (!finite3(c[j])) continue;
                float d, s = 0.f;
                d = c[i].x - c[j].x; s += d * d;
                d = c[i].y - c[j].y; s += d * d;
                d = c[i].z - c[j].z; s += d * d;
                if (s < r2) row.push_back({s, (int32_t)j});
            }
        std::sort(row.begin(), row.end(), [](const Entry& a, const Entry& b) { return a.d2 < b.d2 || (a.d2 == b.d2 && a.j < b.j); });
        rows.e.insert(rows.e.end(), row.begin(), row.end());
        rows.off[i + 1] = rows.e.size();
    }
    return rows;
}

}  // namespace

int main(int argc, char** argv) {
    const bool self = argc == 3 && std::string(argv[1]) == "--self";
    if (argc != 3 && argc != 6) { fprintf(stderr, "usage: rift_host IN OUT [normal_radius gradient_radius rift_radius]\n"); return 2; }
    const double normal_radius = argc == 6 ? atof(argv[3]) : 0.03, gradient_radius = argc == 6 ? atof(argv[4]) : 0.03,
                 rift_radius = argc == 6 ? atof(argv[5]) : 0.05;
    FILE* f = nullptr;
    std::vector<Rec> c;
    if (self) {
        uint64_t st = 0x9E3779B97F4A7C15ull;
        auto rnd = [&]() { st = st * 6364136223846793005ull + 1442695040888963407ull; return (float)((st >> 40) * (1.0 / (1 << 24))); };
        for (int i = 0; i < 240; ++i) {
            Rec r{rnd() * 0.08f, rnd() * 0.08f, rnd() * 0.08f, (uint32_t)(st >> 20)};
            if (i % 40 == 7) r = c[(size_t)i - 1];                    // a duplicate
            if (i % 60 == 11) r.x += 1.0f + (float)i;                  // isolated
            if (i % 80 == 13) r.y = pcc::lm_float(0x7fc00000u);        // not finite
            c.push_back(r);
        }
    } else {
        int32_t n32 = 0;
        f = fopen(argv[1], "rb");
        if (!f || fread(&n32, 4, 1, f) != 1 || n32 < 0) { fprintf(stderr, "rift_host: cannot read %s\n", argv[1]); return 2; }
        c.resize((size_t)n32);
        if (n32 && fread(c.data(), sizeof(Rec), c.size(), f) != c.size()) { fprintf(stderr, "rift_host: %s is short\n", argv[1]); return 2; }
        fclose(f);
    }
    const size_t n = c.size();

    const auto t0 = std::chrono::steady_clock::now();
    const float qnan = pcc::lm_float(0x7fc00000u);
    // normals (NormalEstimation, setRadiusSearch), viewpoint origin
    Rows rn = radius_rows(c, normal_radius);
    std::vector<float> nrm(n * 3, qnan);
    std::vector<char> in2(n, 0);  // member of cloud2
    for (size_t i = 0; i < n; ++i) {
        const size_t beg = rn.off[i], cnt = rn.off[i + 1] - beg;
        if (cnt < 3) continue;
        float acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, cov[9], nv[3], curv;
        for (size_t k = 0; k < cnt; ++k) {
            const Rec& p = c[rn.e[beg + k].j];
            acc[0] += p.x * p.x; acc[1] += p.x * p.y; acc[2] += p.x * p.z;
            acc[3] += p.y * p.y; acc[4] += p.y * p.z; acc[5] += p.z * p.z;
            acc[6] += p.x; acc[7] += p.y; acc[8] += p.z;
        }
        pcc::covariance_from_sums(acc, (unsigned int)cnt, cov);
        pcc::plane_from_covariance(cov, nv, &curv);
        const float dx = 0.f - c[i].x, dy = 0.f - c[i].y, dz = 0.f - c[i].z;
        if (dx * nv[0] + dy * nv[1] + dz * nv[2] < 0) { nv[0] *= -1; nv[1] *= -1; nv[2] *= -1; }
        nrm[i * 3] = nv[0]; nrm[i * 3 + 1] = nv[1]; nrm[i * 3 + 2] = nv[2];
        in2[i] = pcc::rift_finite(nv[0]) && pcc::rift_finite(nv[1]) && pcc::rift_finite(nv[2]);
    }
    // intensity
    std::vector<float> inten(n);
    for (size_t i = 0; i < n; ++i) inten[i] = pcc::rift_intensity(c[i].bgra);
    // intensity gradient over the rows of cloud2
    if (gradient_radius != normal_radius) rn = radius_rows(c, gradient_radius);
    std::vector<float> grad(n * 3, qnan);
    for (size_t i = 0; i < n; ++i) {
        if (!in2[i]) continue;
        const size_t beg = rn.off[i], end = rn.off[i + 1];
        float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;
        unsigned int cnt = 0;
        for (size_t k = beg; k < end; ++k) {
            const int32_t j = rn.e[k].j;
            if (!in2[j]) continue;
            sx += c[j].x; sy += c[j].y; sz += c[j].z; si += inten[j];
            ++cnt;
        }
        if (cnt < 3) continue;
        const float fc = (float)cnt, cx = sx / fc, cy = sy / fc, cz = sz / fc, mi = si / fc;
        float a[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0}, x[3];
        for (size_t k = beg; k < end; ++k) {
            const int32_t j = rn.e[k].j;
            if (!in2[j]) continue;
            const float px = c[j].x - cx, py = c[j].y - cy, pz = c[j].z - cz, di = inten[j] - mi;
            a[0] += px * px; a[1] += px * py; a[2] += px * pz; a[3] += py * py; a[4] += py * pz; a[5] += pz * pz;
            b[0] += px * di; b[1] += py * di; b[2] += pz * di;
        }
        pcc::rift_solve3(a, b, x);
        pcc::rift_project(&nrm[i * 3], x, &grad[i * 3]);
    }
    // RIFT over the rows of cloud2
    Rows rr = radius_rows(c, rift_radius);
    const float radius_f = (float)rift_radius;
    std::vector<float> hist;
    std::vector<int32_t> kept;
    for (size_t i = 0; i < n; ++i) {
        if (!in2[i]) continue;
        float h[pcc::RIFT_D_BINS][pcc::RIFT_G_BINS] = {};
        const float p0[3] = {c[i].x, c[i].y, c[i].z};
        for (size_t k = rr.off[i]; k < rr.off[i + 1]; ++k) {
            const int32_t j = rr.e[k].j;
            if (!in2[j]) continue;
            const float p[3] = {c[j].x, c[j].y, c[j].z};
            const pcc::RiftVote v = pcc::rift_vote(p0, p, &grad[(size_t)j * 3], rr.e[k].d2, radius_f);
            int d_lo, d_hi, g_lo, g_hi;
            pcc::rift_vote_range(v, &d_lo, &d_hi, &g_lo, &g_hi);
            for (int g = g_lo; g <= g_hi; ++g)
                for (int d = d_lo; d <= d_hi; ++d) h[d][(g + pcc::RIFT_G_BINS) % pcc::RIFT_G_BINS] += pcc::rift_vote_term(v, d, g);
        }
        float o[pcc::RIFT_BINS];
        for (int g = 0; g < pcc::RIFT_G_BINS; ++g)
            for (int d = 0; d < pcc::RIFT_D_BINS; ++d) o[g * pcc::RIFT_D_BINS + d] = h[d][g];
        const float nr = pcc::rift_norm(o);
        for (int k = 0; k < pcc::RIFT_BINS; ++k) o[k] = o[k] / nr;
        if (!pcc::rift_finite(o[0])) continue;
        hist.insert(hist.end(), o, o + pcc::RIFT_BINS);
        kept.push_back((int32_t)i);
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

    f = fopen(argv[2], "wb");
    const int32_t n_out = (int32_t)kept.size();
    if (!f || fwrite(&n_out, 4, 1, f) != 1 || fwrite(hist.data(), 4, hist.size(), f) != hist.size() ||
        fwrite(kept.data(), 4, kept.size(), f) != kept.size() || fclose(f) != 0) {
        fprintf(stderr, "rift_host: cannot write %s\n", argv[2]);
        return 2;
    }
    printf("rift_host n=%zu kept=%d ms=%.3f\n", n, n_out, ms);
    return 0;
}
