// changes_host.cpp -- dev helper of tools/exp_changes.py (not part of `all`): pcc_change_detection's contract on ONE host core,
// from csrc/change_plan.hpp -- the same anchor, the same voxel coordinates, the same 64-bit keys -- with std::unordered_set for
// the voxels of A and std::unordered_map for the counts of B.  No library, no GPU.
//   changes_host a.f32 b.f32 out.i32 resolution min_points_per_leaf
// a.f32, b.f32: n x 3 floats; out.i32: the indices into b, ascending.  Prints the milliseconds of the work between the reads and
// the write.
#include "change_plan.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <unordered_map>
#include <unordered_set>
#include <vector>

using namespace pcc;
struct P3 { float x, y, z; };

static bool load(const char* path, std::vector<P3>& pts) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const size_t n = (size_t)std::ftell(f) / 12;
    std::fseek(f, 0, SEEK_SET);
    pts.resize(n);
    const bool ok = n == 0 || std::fread(pts.data(), 12, n, f) == n;
    std::fclose(f);
    return ok;
}
static bool finite(const P3& p) { return std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z); }

int main(int argc, char** argv) {
    if (argc < 6) { std::printf("usage: changes_host a.f32 b.f32 out.i32 resolution min_points_per_leaf\n"); return 2; }
    std::vector<P3> a, b;
    if (!load(argv[1], a) || !load(argv[2], b)) return 1;
    const double res = std::atof(argv[4]);
    const size_t min_points = (size_t)std::atoll(argv[5]);
    const auto t0 = std::chrono::steady_clock::now();
    const P3* first = nullptr;
    for (const std::vector<P3>* c : {&a, &b}) {
        for (const P3& p : *c)
            if (finite(p)) { first = &p; break; }
        if (first) break;
    }
    std::vector<int32_t> out;
    if (first) {
        const double anc[3] = {change_anchor(first->x, res), change_anchor(first->y, res), change_anchor(first->z, res)};
        int64_t mn[3] = {INT64_MAX, INT64_MAX, INT64_MAX}, mx[3] = {INT64_MIN, INT64_MIN, INT64_MIN};
        auto coords = [&](const P3& p, int64_t k[3]) {
            return change_coord(p.x, anc[0], res, &k[0]) && change_coord(p.y, anc[1], res, &k[1]) && change_coord(p.z, anc[2], res, &k[2]);
        };
        for (const std::vector<P3>* c : {&a, &b})
            for (const P3& p : *c) {
                int64_t k[3];
                if (!finite(p)) continue;
                if (!coords(p, k)) { std::printf("a voxel coordinate beyond 2^31\n"); return 1; }
                for (int ax = 0; ax < 3; ++ax) { mn[ax] = std::min(mn[ax], k[ax]); mx[ax] = std::max(mx[ax], k[ax]); }
            }
        for (int ax = 0; ax < 3; ++ax)
            if (!change_span_ok(mn[ax], mx[ax])) { std::printf("more than 2^21 voxels along an axis\n"); return 1; }
        std::unordered_set<uint64_t> in_a;
        std::unordered_map<uint64_t, uint32_t> in_b;
        in_a.reserve(a.size());
        in_b.reserve(b.size());
        int64_t k[3];
        for (const P3& p : a)
            if (finite(p) && coords(p, k)) in_a.insert(change_key(k, mn));
        std::vector<uint64_t> key_b(b.size(), CHANGE_EMPTY_KEY);
        for (size_t i = 0; i < b.size(); ++i)
            if (finite(b[i]) && coords(b[i], k)) ++in_b[key_b[i] = change_key(k, mn)];
        for (size_t i = 0; i < b.size(); ++i)
            if (key_b[i] != CHANGE_EMPTY_KEY && !in_a.count(key_b[i]) && in_b[key_b[i]] >= min_points) out.push_back((int32_t)i);
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::printf("total %.3f ms, reported %zu\n", ms, out.size());
    FILE* f = std::fopen(argv[3], "wb");
    if (!f) return 1;
    if (!out.empty()) std::fwrite(out.data(), 4, out.size(), f);
    std::fclose(f);
    return 0;
}
