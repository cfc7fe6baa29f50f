// vfh_host.cpp -- pcc_vfh_descriptor and pcc_match_vfh on the CPU, one core: the arithmetic of csrc/vfh_math.hpp (with
// csrc/fpfh_math.hpp's pair features) and csrc/plane_fit.hpp, the headers the kernels are built from, over EXHAUSTIVE sorted
// radius rows.  Test infrastructure (tests/test_vfh_cpu.py, tests/test_vfh_gpu.py, tools/exp_vfh.py): the library does not link it.
//   stages (reference src/comparator.cpp:482-516, processVHF): normals at the radius, viewpoint origin -- every point stays,
//   whatever its normal holds; the xyz centroid and the centroid of the finite normals, float chains in index order; one vote
//   per point into 45 + 45 + 45 + 128 integer counters; every bin rebuilt from its count.
// usage: vfh_host IN OUT [--radius NORMAL_RADIUS] [--normals FILE] [--counts FILE] [--votes FILE]
//   IN : int32 n, then n records (float x, y, z; uint32 colour word, not read)
//   OUT: int32 m (1, or 0 for n < 2), m x 308 floats
//   --normals FILE : float[n][3] read instead of fitted
//   --counts FILE  : written, int32[263]: the votes of f1[45], f2[45], f3[45] and of the viewpoint component [128]
//   --votes FILE   : written, int32[n][4]: the f1, f2, f3 and viewpoint bin of every point (f1 .. f3 are -1: no vote)
//   exit status 3: the cloud holds a non-finite point (the library answers PCC_ERR_UNSUPPORTED)
//        vfh_host --match H1 H2 OUT   matchVHF of every pair: H1, H2 = int32 m, m x 308 floats; OUT = m1 x m2 doubles, row-major
//        vfh_host --self OUT          a built-in 240-point cloud with duplicates and isolated points (`make asan`)
// prints "vfh_host n=.. out=.. cp=.. ms=.." (the pipeline alone, no file I/O)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "vfh_math.hpp"
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

bool finite3(const float* p) { return pcc::fpfh_finite(p[0]) && pcc::fpfh_finite(p[1]) && pcc::fpfh_finite(p[2]); }

bool read_cloud(const char* path, std::vector<Rec>* c) {
    int32_t n32 = 0;
    FILE* f = fopen(path, "rb");
    if (!f || fread(&n32, 4, 1, f) != 1 || n32 < 0) { fprintf(stderr, "vfh_host: cannot read %s\n", path); if (f) fclose(f); return false; }
    c->resize((size_t)n32);
    const bool ok = !n32 || fread(c->data(), sizeof(Rec), c->size(), f) == c->size();
    fclose(f);
    if (!ok) fprintf(stderr, "vfh_host: %s is short\n", path);
    return ok;
}
bool read_floats(const char* path, std::vector<float>* v, size_t count) {
    v->resize(count);
    FILE* f = fopen(path, "rb");
    const bool ok = f && (!count || fread(v->data(), 4, count, f) == count);
    if (f) fclose(f);
    if (!ok) fprintf(stderr, "vfh_host: cannot read %zu floats from %s\n", count, path);
    return ok;
}
bool read_descriptors(const char* path, std::vector<float>* v, size_t* m) {
    int32_t m32 = 0;
    FILE* f = fopen(path, "rb");
    if (!f || fread(&m32, 4, 1, f) != 1 || m32 < 0) { fprintf(stderr, "vfh_host: cannot read %s\n", path); if (f) fclose(f); return false; }
    *m = (size_t)m32;
    v->resize(*m * pcc::VFH_BINS);
    const bool ok = v->empty() || fread(v->data(), 4, v->size(), f) == v->size();
    fclose(f);
    if (!ok) fprintf(stderr, "vfh_host: %s is short\n", path);
    return ok;
}
bool write_all(const char* path, const void* a, size_t a_bytes, const void* b = nullptr, size_t b_bytes = 0) {
    FILE* f = fopen(path, "wb");
    const bool ok = f && (!a_bytes || fwrite(a, 1, a_bytes, f) == a_bytes) && (!b_bytes || fwrite(b, 1, b_bytes, f) == b_bytes);
    if ((f && fclose(f) != 0) || !ok) { fprintf(stderr, "vfh_host: cannot write %s\n", path); return false; }
    return true;
}

// the plane fit over sorted radius rows of every point against every point: d2 < float(r * r), ascending (d2, index), FLANN's
// L2_Simple sum; a row of fewer than 3 entries leaves the NaN
void fit_normals(const std::vector<Rec>& c, double radius, std::vector<float>* nrm) {
    const float r2 = (float)(radius * radius);
    const size_t n = c.size();
    std::vector<Entry> row;
    for (size_t i = 0; i < n; ++i) {
        row.clear();
        for (size_t j = 0; j < n; ++j) {
            float d, s = 0.f;
            d = c[i].x - c[j].x; s += d * d;
            d = c[i].y - c[j].y; s += d * d;
            d = c[i].z - c[j].z; s += d * d;
            if (s < r2) row.push_back({s, (int32_t)j});
        }
        if (row.size() < 3) continue;
        std::sort(row.begin(), row.end(), [](const Entry& a, const Entry& b) { return a.d2 < b.d2 || (a.d2 == b.d2 && a.j < b.j); });
        float acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, cov[9], nv[3], curv;
        for (const Entry& e : row) {
            const Rec& p = c[e.j];
            acc[0] += p.x * p.x; acc[1] += p.x * p.y; acc[2] += p.x * p.z;
            acc[3] += p.y * p.y; acc[4] += p.y * p.z; acc[5] += p.z * p.z;
            acc[6] += p.x; acc[7] += p.y; acc[8] += p.z;
        }
        pcc::covariance_from_sums(acc, (unsigned int)row.size(), cov);
        pcc::plane_from_covariance(cov, nv, &curv);
        const float dx = 0.f - c[i].x, dy = 0.f - c[i].y, dz = 0.f - c[i].z;
        if (dx * nv[0] + dy * nv[1] + dz * nv[2] < 0) { nv[0] *= -1; nv[1] *= -1; nv[2] *= -1; }
        (*nrm)[i * 3] = nv[0]; (*nrm)[i * 3 + 1] = nv[1]; (*nrm)[i * 3 + 2] = nv[2];
    }
}

// the stages behind the normals (n >= 2): counters[263], hist[308]; returns cp
unsigned int vfh_of(const std::vector<Rec>& c, const std::vector<float>& nrm, unsigned int* counters, float* hist, std::vector<int32_t>* votes) {
    const size_t n = c.size();
    float sum[3] = {0.f, 0.f, 0.f}, nsum[3] = {0.f, 0.f, 0.f};
    unsigned int cp = 0;
    for (size_t i = 0; i < n; ++i) {
        sum[0] += c[i].x; sum[1] += c[i].y; sum[2] += c[i].z;
        if (!finite3(&nrm[i * 3])) continue;
        nsum[0] += nrm[i * 3]; nsum[1] += nrm[i * 3 + 1]; nsum[2] += nrm[i * 3 + 2];
        ++cp;
    }
    float centroid[3], ncentroid[3], d_vp_p[3];
    for (int k = 0; k < 3; ++k) { centroid[k] = sum[k] / (float)n; ncentroid[k] = nsum[k] / (float)cp; }
    pcc::vfh_view_direction(centroid, d_vp_p);
    for (int k = 0; k < pcc::VFH_COUNTERS; ++k) counters[k] = 0u;
    for (size_t i = 0; i < n; ++i) {
        const pcc::VfhVote v = pcc::vfh_vote(centroid, ncentroid, d_vp_p, &c[i].x, &nrm[i * 3]);
        if (v.f1 != pcc::VFH_NO_VOTE) {
            ++counters[v.f1];
            ++counters[pcc::VFH_F_BINS + v.f2];
            ++counters[2 * pcc::VFH_F_BINS + v.f3];
        }
        ++counters[3 * pcc::VFH_F_BINS + v.vp];
        if (votes) votes->insert(votes->end(), {v.f1, v.f2, v.f3, v.vp});
    }
    for (int b = 0; b < pcc::VFH_BINS; ++b) hist[b] = pcc::vfh_bin_value(counters, (unsigned int)n, b);
    return cp;
}

int match_mode(char** argv) {
    std::vector<float> h1, h2;
    size_t m1 = 0, m2 = 0;
    if (!read_descriptors(argv[2], &h1, &m1) || !read_descriptors(argv[3], &h2, &m2)) return 2;
    std::vector<double> out(m1 * m2);
    for (size_t i = 0; i < m1; ++i)
        for (size_t j = 0; j < m2; ++j) out[i * m2 + j] = pcc::vfh_distance(&h1[i * pcc::VFH_BINS], &h2[j * pcc::VFH_BINS]);
    if (!write_all(argv[4], out.data(), out.size() * sizeof(double))) return 2;
    printf("vfh_host match %zu x %zu\n", m1, m2);
    return 0;
}

int usage() {
    fprintf(stderr, "usage: vfh_host IN OUT [--radius NORMAL_RADIUS] [--normals FILE] [--counts FILE] [--votes FILE]\n"
                    "       vfh_host --match H1 H2 OUT\n       vfh_host --self OUT\n");
    return 2;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 5 && std::string(argv[1]) == "--match") return match_mode(argv);
    const bool self = argc == 3 && std::string(argv[1]) == "--self";
    if (argc < 3) return usage();
    double normal_radius = 0.03;
    const char *normals_path = nullptr, *counts_path = nullptr, *votes_path = nullptr;
    for (int a = 3; a < argc;) {
        const std::string opt = argv[a];
        if (opt == "--radius" && a + 1 < argc) { normal_radius = atof(argv[a + 1]); a += 2; }
        else if (opt == "--normals" && a + 1 < argc) { normals_path = argv[a + 1]; a += 2; }
        else if (opt == "--counts" && a + 1 < argc) { counts_path = argv[a + 1]; a += 2; }
        else if (opt == "--votes" && a + 1 < argc) { votes_path = argv[a + 1]; a += 2; }
        else return usage();
    }
    std::vector<Rec> c;
    if (self) {
        uint64_t st = 0x9E3779B97F4A7C15ull;
        auto rnd = [&]() { st = st * 6364136223846793005ull + 1442695040888963407ull; return (float)((st >> 40) * (1.0 / (1 << 24))); };
        for (int i = 0; i < 240; ++i) {
            Rec r{0.3f + rnd() * 0.08f, 0.2f + rnd() * 0.08f, 0.5f + rnd() * 0.08f, (uint32_t)(st >> 20)};
            if (i % 40 == 7) r = c[(size_t)i - 1];                    // a duplicate
            if (i % 60 == 11) r.x += 1.0f + (float)i;                  // isolated: a NaN normal that stays and votes
            c.push_back(r);
        }
    } else if (!read_cloud(argv[1], &c)) {
        return 2;
    }
    const size_t n = c.size();
    for (size_t i = 0; i < n; ++i)
        if (!finite3(&c[i].x)) { fprintf(stderr, "vfh_host: point %zu is not finite\n", i); return 3; }
    std::vector<float> nrm(n * 3, pcc::lm_float(0x7fc00000u));
    if (normals_path && !read_floats(normals_path, &nrm, n * 3)) return 2;

    const auto t0 = std::chrono::steady_clock::now();
    std::vector<unsigned int> counters(pcc::VFH_COUNTERS, 0u);
    std::vector<float> hist;
    std::vector<int32_t> votes;
    unsigned int cp = 0;
    if (n >= 2) {
        if (!normals_path) fit_normals(c, normal_radius, &nrm);
        hist.resize(pcc::VFH_BINS);
        cp = vfh_of(c, nrm, counters.data(), hist.data(), votes_path || self ? &votes : nullptr);
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

    const int32_t m = hist.empty() ? 0 : 1;
    if (!write_all(argv[2], &m, 4, hist.data(), hist.size() * 4)) return 2;
    if (counts_path && !write_all(counts_path, counters.data(), counters.size() * 4)) return 2;
    if (votes_path && !write_all(votes_path, votes.data(), votes.size() * 4)) return 2;
    if (self) {
        // the distance of the descriptor from itself and from a shifted copy (matchVHF)
        std::vector<float> other(hist);
        std::rotate(other.begin(), other.begin() + 1, other.end());
        const double d0 = pcc::vfh_distance(hist.data(), hist.data()), d1 = pcc::vfh_distance(hist.data(), other.data());
        if (d0 != 0.0 || !(d1 > 0.0)) { fprintf(stderr, "vfh_host: self distances %g %g\n", d0, d1); return 1; }
    }
    printf("vfh_host n=%zu out=%d cp=%u ms=%.3f\n", n, m, cp, ms);
    return 0;
}
