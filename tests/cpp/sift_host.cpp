// sift_host.cpp -- the SIFT keypoint detector of pcc_sift_keypoints on the CPU, one core: the arithmetic of
// csrc/sift_math.hpp (the header the kernels are built from) over EXHAUSTIVE sorted radius rows and k-NN rows, and a voxel
// grid that accumulates in double like pcc_voxel_grid's.  Test infrastructure (tests/test_sift_cpu.py,
// tests/test_sift_gpu.py, tools/exp_sift.py): the library does not link it.
//   per octave (reference src/comparator.cpp:435-469, pcl::SIFTKeypoint): voxel grid at leaf = scale; fewer than 25 points
//   end the loop; scales; intensity; Gaussian responses over the rows at 3 x the largest scale, DoG columns; extrema over the
//   25 nearest neighbours; keypoints in (octave, point, column) order.
// usage: sift_host IN OUT [min_scale nr_octaves nr_scales_per_octave min_contrast [DUMP]]
//   IN  : int32 n, then n records (float x, y, z; uint32 colour word, bytes b g r a)
//   OUT : int32 m, m x (float x, y, z, scale), m x (int32 octave, point, column)
//   DUMP: int32 octaves processed; per octave int32 n, int32 scales, n records as in IN, n floats intensity,
//         n x (scales - 1) floats DoG, scales floats (the scales)
//        sift_host --self OUT   a built-in 400-point cloud with duplicates and non-finite points (`make asan`)
// prints "sift_host n=.. keypoints=.. octaves=.. sizes=a/b/.. stop=gate|count rows_min=.. rows_max=.. ms=.." (no file I/O in ms)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "sift_math.hpp"

namespace {

struct Rec {
    float x, y, z;
    uint32_t bgra;
};
struct Entry {
    float d2;
    int32_t j;
};
bool entry_less(const Entry& a, const Entry& b) { return a.d2 < b.d2 || (a.d2 == b.d2 && a.j < b.j); }
bool finite3(const Rec& p) { return std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z); }

// pcl::VoxelGrid as pcc_voxel_grid computes it: the leaf lattice from the float bounding box of the finite points, voxel
// floor(p * inverse_leaf) - min_b, output in ascending voxel index; centroid sums in double rounded once, colour sums in
// integers divided in float and truncated.  false: more than 2^26 voxels.
bool voxel_grid(const std::vector<Rec>& in, float leaf, std::vector<Rec>* out) {
    out->clear();
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    size_t valid = 0;
    for (const Rec& p : in) {
        if (!finite3(p)) continue;
        ++valid;
        const float v[3] = {p.x, p.y, p.z};
        for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], v[a]); hi[a] = std::max(hi[a], v[a]); }
    }
    if (!valid) return true;
    const float inv = 1.0f / leaf;
    float org[3];
    int dim[3];
    double cells = 1;
    for (int a = 0; a < 3; ++a) {
        const int mn = (int)std::floor(lo[a] * inv), mx = (int)std::floor(hi[a] * inv);
        org[a] = (float)mn;
        dim[a] = mx - mn + 1;
        cells *= (double)dim[a];
    }
    if (cells > (double)(1u << 26)) return false;
    std::vector<std::pair<uint32_t, uint32_t>> order;  // (voxel, point)
    order.reserve(valid);
    for (size_t i = 0; i < in.size(); ++i) {
        const Rec& p = in[i];
        if (!finite3(p)) continue;
        const int i0 = std::min(std::max((int)(floorf(p.x * inv) - org[0]), 0), dim[0] - 1);
        const int i1 = std::min(std::max((int)(floorf(p.y * inv) - org[1]), 0), dim[1] - 1);
        const int i2 = std::min(std::max((int)(floorf(p.z * inv) - org[2]), 0), dim[2] - 1);
        order.push_back({((uint32_t)i2 * (uint32_t)dim[1] + (uint32_t)i1) * (uint32_t)dim[0] + (uint32_t)i0, (uint32_t)i});
    }
    std::sort(order.begin(), order.end());
    for (size_t t = 0; t < order.size();) {
        double sx = 0, sy = 0, sz = 0;
        unsigned int sr = 0, sg = 0, sb = 0, cnt = 0;
        size_t u = t;
        for (; u < order.size() && order[u].first == order[t].first; ++u) {
            const Rec& p = in[order[u].second];
            sx += p.x; sy += p.y; sz += p.z;
            sr += (p.bgra >> 16) & 0xffu; sg += (p.bgra >> 8) & 0xffu; sb += p.bgra & 0xffu;
            ++cnt;
        }
        const float fc = (float)cnt;
        const int r = (int)((float)sr / fc), g = (int)((float)sg / fc), b = (int)((float)sb / fc);
        out->push_back({(float)(sx / cnt), (float)(sy / cnt), (float)(sz / cnt), ((uint32_t)r << 16) | ((uint32_t)g << 8) | (uint32_t)b});
        t = u;
    }
    return true;
}

void put(FILE* f, const void* p, size_t bytes) {
    if (bytes && fwrite(p, 1, bytes, f) != bytes) { fprintf(stderr, "sift_host: short write\n"); exit(2); }
}

}  // namespace

int main(int argc, char** argv) {
    const bool self = argc == 3 && std::string(argv[1]) == "--self";
    if (argc != 3 && argc != 7 && argc != 8) {
        fprintf(stderr, "usage: sift_host IN OUT [min_scale nr_octaves nr_scales_per_octave min_contrast [DUMP]]\n");
        return 2;
    }
    const float min_scale = argc >= 7 ? (float)atof(argv[3]) : 0.005f, min_contrast = argc >= 7 ? (float)atof(argv[6]) : 0.001f;
    const int nr_octaves = argc >= 7 ? atoi(argv[4]) : 5, nspo = argc >= 7 ? atoi(argv[5]) : 5;
    if (!(min_scale > 0.f) || nr_octaves < 1 || nspo < pcc::SIFT_MIN_SCALES_PER_OCTAVE || nspo > pcc::SIFT_MAX_SCALES_PER_OCTAVE) {
        fprintf(stderr, "sift_host: bad parameters\n");
        return 2;
    }
    std::vector<Rec> input;
    if (self) {
        uint64_t st = 0x9E3779B97F4A7C15ull;
        auto rnd = [&]() { st = st * 6364136223846793005ull + 1442695040888963407ull; return (float)((st >> 40) * (1.0 / (1 << 24))); };
        for (int i = 0; i < 400; ++i) {
            Rec r{rnd() * 0.1f, rnd() * 0.1f, rnd() * 0.1f, (uint32_t)(st >> 20)};
            if (i % 40 == 7) r = input[(size_t)i - 1];                  // a duplicate
            if (i % 80 == 13) r.y = pcc::lm_float(0x7fc00000u);        // not finite
            input.push_back(r);
        }
    } else {
        int32_t n32 = 0;
        FILE* f = fopen(argv[1], "rb");
        if (!f || fread(&n32, 4, 1, f) != 1 || n32 < 0) { fprintf(stderr, "sift_host: cannot read %s\n", argv[1]); return 2; }
        input.resize((size_t)n32);
        if (n32 && fread(input.data(), sizeof(Rec), input.size(), f) != input.size()) { fprintf(stderr, "sift_host: %s is short\n", argv[1]); return 2; }
        fclose(f);
    }
    FILE* dump = argc == 8 ? fopen(argv[7], "wb") : nullptr;
    if (argc == 8 && !dump) { fprintf(stderr, "sift_host: cannot write %s\n", argv[7]); return 2; }
    int32_t octaves_done = 0;
    if (dump) put(dump, &octaves_done, 4);  // (rewritten at the end)

    const auto t0 = std::chrono::steady_clock::now();
    std::vector<float> kp;        // x, y, z, scale
    std::vector<int32_t> kp_id;   // octave, point, column
    std::vector<Rec> cloud = input, next;
    std::string sizes;
    const char* stop = "count";
    size_t rows_min = (size_t)-1, rows_max = 0;
    float scale = min_scale;
    for (int o = 0; o < nr_octaves; ++o, scale *= 2.0f) {
        if (!voxel_grid(cloud, scale, &next)) { fprintf(stderr, "sift_host: leaf %g too small\n", scale); return 3; }
        cloud.swap(next);
        const size_t n = cloud.size();
        sizes += (sizes.empty() ? "" : "/") + std::to_string(n);
        if (n < (size_t)pcc::SIFT_MIN_POINTS) { stop = "gate"; break; }
        pcc::SiftOctave oc;
        pcc::sift_octave_scales(scale, nspo, min_contrast, &oc);
        const int S = oc.n_scales, D = S - 1;
        std::vector<float> inten(n);
        for (size_t i = 0; i < n; ++i) inten[i] = pcc::sift_intensity(cloud[i].bgra);
        const float radius = 3.0f * oc.scales[S - 1];
        const float r2 = (float)((double)radius * (double)radius);
        const size_t K = std::min<size_t>(pcc::SIFT_NEIGHBOURS, n);
        std::vector<float> dog(n * (size_t)D);
        std::vector<int32_t> nbr(n * K);
        std::vector<Entry> all(n), row;
        for (size_t i = 0; i < n; ++i) {
            row.clear();
            for (size_t j = 0; j < n; ++j) {
                float d, s = 0.f;  // FLANN's L2_Simple sum
                d = cloud[i].x - cloud[j].x; s += d * d;
                d = cloud[i].y - cloud[j].y; s += d * d;
                d = cloud[i].z - cloud[j].z; s += d * d;
                all[j] = {s, (int32_t)j};
                if (s < r2) row.push_back(all[j]);
            }
            std::sort(row.begin(), row.end(), entry_less);
            std::partial_sort(all.begin(), all.begin() + (long)K, all.end(), entry_less);
            for (size_t k = 0; k < K; ++k) nbr[i * K + k] = all[k].j;
            rows_min = std::min(rows_min, row.size());
            rows_max = std::max(rows_max, row.size());
            float prev = 0.f;
            for (int s = 0; s < S; ++s) {
                float num = 0.f, den = 0.f;
                for (const Entry& e : row) {
                    if (!(e.d2 <= oc.cut[s])) break;
                    pcc::sift_accumulate(inten[(size_t)e.j], pcc::sift_weight(e.d2, oc.sigma2[s]), &num, &den);
                }
                const float resp = pcc::sift_response(num, den);
                if (s > 0) dog[i * (size_t)D + (size_t)(s - 1)] = pcc::sift_dog(resp, prev);
                prev = resp;
            }
        }
        for (size_t i = 0; i < n; ++i) {
            float mn[pcc::SIFT_MAX_DOG], mx[pcc::SIFT_MAX_DOG];
            for (int c = 0; c < D; ++c) { mn[c] = 3.402823466e38f; mx[c] = -3.402823466e38f; }
            for (size_t k = 0; k < K; ++k) {
                const float* dj = &dog[(size_t)nbr[i * K + k] * (size_t)D];
                for (int c = 0; c < D; ++c) { mn[c] = fminf(mn[c], dj[c]); mx[c] = fmaxf(mx[c], dj[c]); }
            }
            for (int c = 1; c < D - 1; ++c) {
                if (!pcc::sift_is_keypoint(dog[i * (size_t)D + (size_t)c], mn[c - 1], mn[c], mn[c + 1], mx[c - 1], mx[c], mx[c + 1], min_contrast)) continue;
                kp.insert(kp.end(), {cloud[i].x, cloud[i].y, cloud[i].z, oc.scales[c]});
                kp_id.insert(kp_id.end(), {(int32_t)o, (int32_t)i, (int32_t)c});
            }
        }
        ++octaves_done;
        if (dump) {
            const int32_t hdr[2] = {(int32_t)n, (int32_t)S};
            put(dump, hdr, 8);
            put(dump, cloud.data(), n * sizeof(Rec));
            put(dump, inten.data(), n * 4);
            put(dump, dog.data(), dog.size() * 4);
            put(dump, oc.scales, (size_t)S * 4);
        }
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (dump) {
        if (fseek(dump, 0, SEEK_SET) != 0) return 2;
        put(dump, &octaves_done, 4);
        if (fclose(dump) != 0) return 2;
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f) { fprintf(stderr, "sift_host: cannot write %s\n", argv[2]); return 2; }
    const int32_t m = (int32_t)(kp.size() / 4);
    put(f, &m, 4);
    put(f, kp.data(), kp.size() * 4);
    put(f, kp_id.data(), kp_id.size() * 4);
    if (fclose(f) != 0) return 2;
    if (rows_min == (size_t)-1) rows_min = 0;
    printf("sift_host n=%zu keypoints=%d octaves=%d sizes=%s stop=%s rows_min=%zu rows_max=%zu ms=%.3f\n", input.size(), m, octaves_done,
           sizes.c_str(), stop, rows_min, rows_max, ms);
    return 0;
}
