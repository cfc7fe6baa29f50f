// fpfh_host.cpp -- the FPFH descriptor pipeline of pcc_fpfh_descriptors on the CPU, one core: the arithmetic of
// csrc/fpfh_math.hpp and csrc/plane_fit.hpp (the headers the kernels are built from) over EXHAUSTIVE sorted radius rows.
// Test infrastructure (tests/test_fpfh_cpu.py, tests/test_fpfh_gpu.py, tools/exp_fpfh.py): the library does not link it.
//   stages (reference src/comparator.cpp:824-875): normals at normal_radius, viewpoint origin; points without a finite normal
//   leave (cloud2); SPFH signatures over the rows of cloud2 at fpfh_radius; their weighted sums over the same rows.
// usage: fpfh_host IN OUT [--radii NORMAL_RADIUS FPFH_RADIUS] [--normals FILE] [--counts FILE]
//   IN : int32 n, then n records (float x, y, z; uint32 colour word, not read)
//   OUT: int32 m, m x 33 floats, m x int32 original point indices
//   --normals FILE : float[n][3] read instead of fitted (a non-finite component: the point is not in cloud2)
//   --counts FILE  : written, int32[n][33]: the votes every SPFH bin received (zeros outside cloud2)
//        fpfh_host --pairs IN NORMALS PAIRS OUT   the pair features alone: PAIRS = int32 m, m x (int32 p, int32 q);
//                                                 OUT = m x (float f1, f2, f3, f4; int32 ok, swapped)
//        fpfh_host --self OUT   a built-in 240-point cloud with duplicates, isolated and non-finite points (`make asan`)
// prints "fpfh_host n=.. kept=.. ms=.." (the pipeline alone, no file I/O)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "fpfh_math.hpp"
#include "plane_fit.hpp"

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

bool finite3(const float* p) { return pcc::fpfh_finite(p[0]) && pcc::fpfh_finite(p[1]) && pcc::fpfh_finite(p[2]); }
bool finite3(const Rec& p) { return finite3(&p.x); }

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

bool read_cloud(const char* path, std::vector<Rec>* c) {
    int32_t n32 = 0;
    FILE* f = fopen(path, "rb");
    if (!f || fread(&n32, 4, 1, f) != 1 || n32 < 0) { fprintf(stderr, "fpfh_host: cannot read %s\n", path); if (f) fclose(f); return false; }
    c->resize((size_t)n32);
    const bool ok = !n32 || fread(c->data(), sizeof(Rec), c->size(), f) == c->size();
    fclose(f);
    if (!ok) fprintf(stderr, "fpfh_host: %s is short\n", path);
    return ok;
}
bool read_floats(const char* path, std::vector<float>* v, size_t count) {
    v->resize(count);
    FILE* f = fopen(path, "rb");
    const bool ok = f && (!count || fread(v->data(), 4, count, f) == count);
    if (f) fclose(f);
    if (!ok) fprintf(stderr, "fpfh_host: cannot read %zu floats from %s\n", count, path);
    return ok;
}

int pairs_mode(char** argv) {
    std::vector<Rec> c;
    std::vector<float> nrm;
    if (!read_cloud(argv[2], &c) || !read_floats(argv[3], &nrm, c.size() * 3)) return 2;
    FILE* f = fopen(argv[4], "rb");
    int32_t m = 0;
    if (!f || fread(&m, 4, 1, f) != 1 || m < 0) { fprintf(stderr, "fpfh_host: cannot read %s\n", argv[4]); if (f) fclose(f); return 2; }
    std::vector<int32_t> pq((size_t)m * 2);
    const bool got = !m || fread(pq.data(), 4, pq.size(), f) == pq.size();
    fclose(f);
    if (!got) { fprintf(stderr, "fpfh_host: %s is short\n", argv[4]); return 2; }
    struct Out { float f[4]; int32_t ok, swapped; };
    std::vector<Out> out((size_t)m);
    for (int32_t k = 0; k < m; ++k) {
        const int32_t p = pq[(size_t)k * 2], q = pq[(size_t)k * 2 + 1];
        if (p < 0 || q < 0 || (size_t)p >= c.size() || (size_t)q >= c.size()) { fprintf(stderr, "fpfh_host: pair %d out of range\n", k); return 2; }
        const pcc::FpfhPair r = pcc::fpfh_pair(&c[p].x, &nrm[(size_t)p * 3], &c[q].x, &nrm[(size_t)q * 3]);
        out[k] = {{r.f1, r.f2, r.f3, r.f4}, r.ok, r.swapped};
    }
    f = fopen(argv[5], "wb");
    if (!f || (m && fwrite(out.data(), sizeof(Out), out.size(), f) != out.size()) || fclose(f) != 0) {
        fprintf(stderr, "fpfh_host: cannot write %s\n", argv[5]);
        return 2;
    }
    printf("fpfh_host pairs=%d\n", m);
    return 0;
}

int usage() {
    fprintf(stderr, "usage: fpfh_host IN OUT [--radii NORMAL_RADIUS FPFH_RADIUS] [--normals FILE] [--counts FILE]\n"
                    "       fpfh_host --pairs IN NORMALS PAIRS OUT\n       fpfh_host --self OUT\n");
    return 2;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 6 && std::string(argv[1]) == "--pairs") return pairs_mode(argv);
    const bool self = argc == 3 && std::string(argv[1]) == "--self";
    if (argc < 3) return usage();
    double normal_radius = 0.03, fpfh_radius = 0.05;
    const char *normals_path = nullptr, *counts_path = nullptr;
    for (int a = 3; a < argc;) {
        const std::string opt = argv[a];
        if (opt == "--radii" && a + 2 < argc) { normal_radius = atof(argv[a + 1]); fpfh_radius = atof(argv[a + 2]); a += 3; }
        else if (opt == "--normals" && a + 1 < argc) { normals_path = argv[a + 1]; a += 2; }
        else if (opt == "--counts" && a + 1 < argc) { counts_path = argv[a + 1]; a += 2; }
        else return usage();
    }
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
    } else if (!read_cloud(argv[1], &c)) {
        return 2;
    }
    const size_t n = c.size();
    std::vector<float> nrm(n * 3, pcc::lm_float(0x7fc00000u));
    if (normals_path && !read_floats(normals_path, &nrm, n * 3)) return 2;

    const auto t0 = std::chrono::steady_clock::now();
    Rows rr;
    if (!normals_path) {
        // normals (NormalEstimation, setRadiusSearch), viewpoint origin
        rr = radius_rows(c, normal_radius);
        for (size_t i = 0; i < n; ++i) {
            const size_t beg = rr.off[i], cnt = rr.off[i + 1] - beg;
            if (cnt < 3) continue;
            float acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, cov[9], nv[3], curv;
            for (size_t k = 0; k < cnt; ++k) {
                const Rec& p = c[rr.e[beg + k].j];
                acc[0] += p.x * p.x; acc[1] += p.x * p.y; acc[2] += p.x * p.z;
                acc[3] += p.y * p.y; acc[4] += p.y * p.z; acc[5] += p.z * p.z;
                acc[6] += p.x; acc[7] += p.y; acc[8] += p.z;
            }
            pcc::covariance_from_sums(acc, (unsigned int)cnt, cov);
            pcc::plane_from_covariance(cov, nv, &curv);
            const float dx = 0.f - c[i].x, dy = 0.f - c[i].y, dz = 0.f - c[i].z;
            if (dx * nv[0] + dy * nv[1] + dz * nv[2] < 0) { nv[0] *= -1; nv[1] *= -1; nv[2] *= -1; }
            nrm[i * 3] = nv[0]; nrm[i * 3 + 1] = nv[1]; nrm[i * 3 + 2] = nv[2];
        }
    }
    std::vector<char> in2(n, 0);  // member of cloud2
    for (size_t i = 0; i < n; ++i) in2[i] = finite3(c[i]) && finite3(&nrm[i * 3]);
    // SPFH over the rows of cloud2 (computePointSPFHSignature)
    if (normals_path || fpfh_radius != normal_radius) rr = radius_rows(c, fpfh_radius);
    std::vector<int32_t> counts(n * pcc::FPFH_BINS, 0);
    std::vector<float> spfh(n * pcc::FPFH_BINS, 0.f);
    for (size_t i = 0; i < n; ++i) {
        if (!in2[i]) continue;
        int32_t* cnt = &counts[i * pcc::FPFH_BINS];
        unsigned int row_len = 0;
        for (size_t k = rr.off[i]; k < rr.off[i + 1]; ++k) {
            const int32_t j = rr.e[k].j;
            if (!in2[j]) continue;
            ++row_len;
            if ((size_t)j == i) continue;
            const pcc::FpfhPair f = pcc::fpfh_pair(&c[i].x, &nrm[i * 3], &c[j].x, &nrm[(size_t)j * 3]);
            if (!f.ok) continue;
            ++cnt[pcc::fpfh_bin_f1(f.f1)];
            ++cnt[pcc::FPFH_F_BINS + pcc::fpfh_bin_f23(f.f2)];
            ++cnt[2 * pcc::FPFH_F_BINS + pcc::fpfh_bin_f23(f.f3)];
        }
        const float incr = pcc::fpfh_incr(row_len);
        for (int b = 0; b < pcc::FPFH_BINS; ++b) spfh[i * pcc::FPFH_BINS + b] = pcc::fpfh_spfh_value((unsigned int)cnt[b], incr);
    }
    // the weighted sums over the same rows (weightPointSPFHSignature)
    std::vector<float> hist;
    std::vector<int32_t> kept;
    for (size_t i = 0; i < n; ++i) {
        if (!in2[i]) continue;
        float h[pcc::FPFH_BINS] = {}, sum[3] = {0.f, 0.f, 0.f};
        for (size_t k = rr.off[i]; k < rr.off[i + 1]; ++k) {
            const int32_t j = rr.e[k].j;
            if (!in2[j] || rr.e[k].d2 == 0.f) continue;
            const float w = pcc::fpfh_weight(rr.e[k].d2);
            const float* row = &spfh[(size_t)j * pcc::FPFH_BINS];
            for (int f = 0; f < 3; ++f)
                for (int b = 0; b < pcc::FPFH_F_BINS; ++b) {
                    const float val = row[f * pcc::FPFH_F_BINS + b] * w;
                    sum[f] += val;
                    h[f * pcc::FPFH_F_BINS + b] += val;
                }
        }
        for (int f = 0; f < 3; ++f) {
            const float factor = pcc::fpfh_norm_factor(sum[f]);
            for (int b = 0; b < pcc::FPFH_F_BINS; ++b) h[f * pcc::FPFH_F_BINS + b] = h[f * pcc::FPFH_F_BINS + b] * factor;
        }
        hist.insert(hist.end(), h, h + pcc::FPFH_BINS);
        kept.push_back((int32_t)i);
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

    FILE* f = fopen(argv[2], "wb");
    const int32_t n_out = (int32_t)kept.size();
    if (!f || fwrite(&n_out, 4, 1, f) != 1 || fwrite(hist.data(), 4, hist.size(), f) != hist.size() ||
        fwrite(kept.data(), 4, kept.size(), f) != kept.size() || fclose(f) != 0) {
        fprintf(stderr, "fpfh_host: cannot write %s\n", argv[2]);
        return 2;
    }
    if (counts_path) {
        f = fopen(counts_path, "wb");
        if (!f || fwrite(counts.data(), 4, counts.size(), f) != counts.size() || fclose(f) != 0) {
            fprintf(stderr, "fpfh_host: cannot write %s\n", counts_path);
            return 2;
        }
    }
    printf("fpfh_host n=%zu kept=%d ms=%.3f\n", n, n_out, ms);
    return 0;
}
