// shot_host.cpp -- the SHOT352 descriptor pipeline of pcc_shot_descriptors on the CPU, one core: the arithmetic of
// csrc/shot_math.hpp, csrc/libm_f64.hpp and csrc/plane_fit.hpp (the headers the kernels are built from) over EXHAUSTIVE sorted
// radius rows.  Test infrastructure (tests/test_shot_cpu.py, tests/test_shot_gpu.py, tools/exp_shot.py): the library does not
// link it.
//   stages (reference src/comparator.cpp:941-986): normals at normal_radius, viewpoint origin; points without a finite normal
//   leave (cloud2); the local reference frame of every point of cloud2 over its row at shot_radius; the 352 bins over the same row.
// usage: shot_host IN OUT [--radii NORMAL_RADIUS SHOT_RADIUS] [--normals FILE] [--rf FILE] [--lrf-out FILE]
//   IN : int32 n, then n records (float x, y, z; uint32 colour word, not read)
//   OUT: int32 m, m x 352 floats, m x 9 floats (the frames), m x int32 original point indices
//   --normals FILE : float[n][3] read instead of fitted (a non-finite component: the point is not in cloud2)
//   --rf FILE      : float[n][9] by original index, taken as the frames instead of estimated
//   --lrf-out FILE : written, float[n][9] by original index: the frames (NaN outside cloud2)
//        shot_host --self OUT            a built-in 240-point cloud with duplicates, isolated and non-finite points (`make asan`)
//        shot_host --libm acos IN OUT    IN = doubles x, OUT = doubles lm_acos(x)
//        shot_host --libm atan2 IN OUT   IN = pairs of doubles (y, x), OUT = doubles lm_atan2(y, x)
//        shot_host --jacobi IN OUT       IN = m x 6 doubles (xx, xy, xz, yy, yz, zz); OUT = m x 13 doubles: the 3 eigenvalues,
//                                        the 9 words of V row by row, the sweeps shot_jacobi3 returned
// prints "shot_host n=.. kept=.. ms=.." (the pipeline alone, no file I/O)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "plane_fit.hpp"
#include "shot_math.hpp"

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

bool finite3(const float* p) { return pcc::shot_finite(p[0]) && pcc::shot_finite(p[1]) && pcc::shot_finite(p[2]); }
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
    if (!f || fread(&n32, 4, 1, f) != 1 || n32 < 0) { fprintf(stderr, "shot_host: cannot read %s\n", path); if (f) fclose(f); return false; }
    c->resize((size_t)n32);
    const bool ok = !n32 || fread(c->data(), sizeof(Rec), c->size(), f) == c->size();
    fclose(f);
    if (!ok) fprintf(stderr, "shot_host: %s is short\n", path);
    return ok;
}
bool read_floats(const char* path, std::vector<float>* v, size_t count) {
    v->resize(count);
    FILE* f = fopen(path, "rb");
    const bool ok = f && (!count || fread(v->data(), 4, count, f) == count);
    if (f) fclose(f);
    if (!ok) fprintf(stderr, "shot_host: cannot read %zu floats from %s\n", count, path);
    return ok;
}
bool read_doubles(const char* path, std::vector<double>* v) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "shot_host: cannot read %s\n", path); return false; }
    double buf[4096];
    size_t got;
    while ((got = fread(buf, 8, 4096, f)) > 0) v->insert(v->end(), buf, buf + got);
    fclose(f);
    return true;
}
bool write_file(const char* path, const void* data, size_t bytes) {
    FILE* f = fopen(path, "wb");
    const bool ok = f && (!bytes || fwrite(data, 1, bytes, f) == bytes);
    if (f && fclose(f) != 0) { fprintf(stderr, "shot_host: cannot write %s\n", path); return false; }
    if (!ok) fprintf(stderr, "shot_host: cannot write %s\n", path);
    return ok;
}

int libm_mode(char** argv) {
    const std::string fn = argv[2];
    std::vector<double> in, out;
    if (!read_doubles(argv[3], &in)) return 2;
    if (fn == "acos") {
        for (double x : in) out.push_back(pcc::lm_acos(x));
    } else if (fn == "atan2" && in.size() % 2 == 0) {
        for (size_t k = 0; k < in.size(); k += 2) out.push_back(pcc::lm_atan2(in[k], in[k + 1]));
    } else {
        fprintf(stderr, "shot_host: --libm acos|atan2 IN OUT\n");
        return 2;
    }
    if (!write_file(argv[4], out.data(), out.size() * 8)) return 2;
    printf("shot_host libm %s values=%zu\n", fn.c_str(), out.size());
    return 0;
}

int jacobi_mode(char** argv) {
    std::vector<double> in, out;
    if (!read_doubles(argv[2], &in)) return 2;
    if (in.size() % 6) { fprintf(stderr, "shot_host: %s does not hold 6 doubles a matrix\n", argv[2]); return 2; }
    int worst = 0;
    for (size_t k = 0; k < in.size(); k += 6) {
        double d[3], V[3][3];
        const int sweeps = pcc::shot_jacobi3(&in[k], d, V);
        worst = std::max(worst, sweeps);
        out.insert(out.end(), d, d + 3);
        for (int i = 0; i < 3; ++i) out.insert(out.end(), V[i], V[i] + 3);
        out.push_back((double)sweeps);
    }
    if (!write_file(argv[3], out.data(), out.size() * 8)) return 2;
    printf("shot_host jacobi matrices=%zu sweeps_max=%d\n", in.size() / 6, worst);
    return 0;
}

int usage() {
    fprintf(stderr, "usage: shot_host IN OUT [--radii NORMAL_RADIUS SHOT_RADIUS] [--normals FILE] [--rf FILE] [--lrf-out FILE]\n"
                    "       shot_host --self OUT\n       shot_host --libm acos|atan2 IN OUT\n       shot_host --jacobi IN OUT\n");
    return 2;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 5 && std::string(argv[1]) == "--libm") return libm_mode(argv);
    if (argc == 4 && std::string(argv[1]) == "--jacobi") return jacobi_mode(argv);
    const bool self = argc == 3 && std::string(argv[1]) == "--self";
    if (argc < 3) return usage();
    double normal_radius = 0.05, shot_radius = 0.04;
    const char *normals_path = nullptr, *rf_path = nullptr, *lrf_out_path = nullptr;
    for (int a = 3; a < argc;) {
        const std::string opt = argv[a];
        if (opt == "--radii" && a + 2 < argc) { normal_radius = atof(argv[a + 1]); shot_radius = atof(argv[a + 2]); a += 3; }
        else if (opt == "--normals" && a + 1 < argc) { normals_path = argv[a + 1]; a += 2; }
        else if (opt == "--rf" && a + 1 < argc) { rf_path = argv[a + 1]; a += 2; }
        else if (opt == "--lrf-out" && a + 1 < argc) { lrf_out_path = argv[a + 1]; a += 2; }
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
            if (i % 80 == 13) r.y = pcc::shot_nan();                   // not finite
            c.push_back(r);
        }
    } else if (!read_cloud(argv[1], &c)) {
        return 2;
    }
    const size_t n = c.size();
    std::vector<float> nrm(n * 3, pcc::shot_nan()), rf_in;
    if (normals_path && !read_floats(normals_path, &nrm, n * 3)) return 2;
    if (rf_path && !read_floats(rf_path, &rf_in, n * 9)) return 2;

    const auto t0 = std::chrono::steady_clock::now();
    if (!normals_path) {
        // normals (NormalEstimation, setRadiusSearch), viewpoint origin
        const Rows rr = radius_rows(c, normal_radius);
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
    const Rows rr = radius_rows(c, shot_radius);
    // the frames (getLocalRF) over the rows of cloud2
    std::vector<float> rf(n * 9, pcc::shot_nan());
    std::vector<double> vs;
    for (size_t i = 0; i < n; ++i) {
        if (!in2[i]) continue;
        float* out = &rf[i * 9];
        if (rf_path) { std::copy(&rf_in[i * 9], &rf_in[i * 9] + 9, out); continue; }
        double acc[7] = {0, 0, 0, 0, 0, 0, 0}, v[3], x[3], z[3];
        vs.clear();
        for (size_t k = rr.off[i]; k < rr.off[i + 1]; ++k) {
            const int32_t j = rr.e[k].j;
            if (!in2[j] || rr.e[k].d2 == 0.f) continue;
            pcc::shot_lrf_accumulate(acc, &c[i].x, &c[j].x, rr.e[k].d2, shot_radius, v);
            vs.insert(vs.end(), v, v + 3);
        }
        const int valid = (int)(vs.size() / 3);
        if (valid < pcc::SHOT_MIN_NEIGHBOURS || !pcc::shot_lrf_axes(acc, x, z)) continue;  // (NaN)
        pcc::shot_lrf_signs(vs.data(), valid, x, z);
        pcc::shot_rf(x, z, out);
    }
    // the descriptors (computePointSHOT) over the same rows
    std::vector<float> desc, rf_kept;
    std::vector<int32_t> kept;
    for (size_t i = 0; i < n; ++i) {
        if (!in2[i]) continue;
        float h[pcc::SHOT_BINS];
        for (int b = 0; b < pcc::SHOT_BINS; ++b) h[b] = 0.f;
        const float* f = &rf[i * 9];
        unsigned int row_len = 0;
        for (size_t k = rr.off[i]; k < rr.off[i + 1]; ++k) row_len += in2[rr.e[k].j] ? 1u : 0u;
        bool frame = true;
        for (int k = 0; k < 9; ++k) frame = frame && pcc::shot_finite(f[k]);
        if (row_len < (unsigned int)pcc::SHOT_MIN_NEIGHBOURS || !frame) {
            for (int b = 0; b < pcc::SHOT_BINS; ++b) h[b] = pcc::shot_nan();
        } else {
            for (size_t k = rr.off[i]; k < rr.off[i + 1]; ++k) {
                const int32_t j = rr.e[k].j;
                if (!in2[j]) continue;
                int bin[5];
                float val[5];
                if (!pcc::shot_entry(&c[i].x, f, &c[j].x, &nrm[(size_t)j * 3], rr.e[k].d2, shot_radius, bin, val)) continue;
                for (int t = 0; t < 5; ++t)
                    if (bin[t] >= 0 && bin[t] < pcc::SHOT_BINS) h[bin[t]] += val[t];
            }
            const float norm = pcc::shot_norm(h);
            for (int b = 0; b < pcc::SHOT_BINS; ++b) h[b] = h[b] / norm;
        }
        desc.insert(desc.end(), h, h + pcc::SHOT_BINS);
        rf_kept.insert(rf_kept.end(), f, f + 9);
        kept.push_back((int32_t)i);
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

    FILE* f = fopen(argv[2], "wb");
    const int32_t n_out = (int32_t)kept.size();
    if (!f || fwrite(&n_out, 4, 1, f) != 1 || fwrite(desc.data(), 4, desc.size(), f) != desc.size() ||
        fwrite(rf_kept.data(), 4, rf_kept.size(), f) != rf_kept.size() || fwrite(kept.data(), 4, kept.size(), f) != kept.size() ||
        fclose(f) != 0) {
        fprintf(stderr, "shot_host: cannot write %s\n", argv[2]);
        return 2;
    }
    if (lrf_out_path && !write_file(lrf_out_path, rf.data(), rf.size() * 4)) return 2;
    printf("shot_host n=%zu kept=%d ms=%.3f\n", n, n_out, ms);
    return 0;
}
