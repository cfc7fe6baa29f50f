// ground_host.cpp -- dev helper of tools/exp_ground.py (not part of `all`): the progressive morphological filter on ONE host core,
// lattice-accelerated, from csrc/ground_plan.hpp -- the same window table, the same lattice and the same walk the kernels of
// ground.hip do (interior cells by their aggregate, rim rows point by point).  No library, no GPU.
//   ground_host in.f32 out.i32 max_window slope initial_distance max_distance cell_size base exponential
// in.f32: n x 3 floats (x, y, z, finite); out.i32: the ground indices, ascending.  Prints the milliseconds of every window.
#include "ground_plan.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace pcc;
struct P3 { float x, y, z; };

static void pass(const std::vector<P3>& pts, const GroundLattice& L, const std::vector<int>& cell, const std::vector<unsigned>& start,
                 const std::vector<unsigned>& order, const std::vector<float>& vals, bool take_max, std::vector<float>& out) {
    const size_t m = pts.size(), nc = ground_table_cells(L);
    const float none = take_max ? -INFINITY : INFINITY;
    auto better = [&](float a, float b) { return take_max ? std::max(a, b) : std::min(a, b); };
    std::vector<float> tab(nc, none);
    float all = none;
    for (size_t i = 0; i < m; ++i) { tab[cell[i]] = better(tab[cell[i]], vals[i]); all = better(all, vals[i]); }
    // cell order, as the device walks it: xy and values side by side
    std::vector<P3> s(m);
    for (size_t j = 0; j < m; ++j) s[j] = {pts[order[j]].x, pts[order[j]].y, vals[order[j]]};
    out.resize(m);
    for (size_t j = 0; j < m; ++j) {
        if (L.whole) { out[order[j]] = all; continue; }
        const float lo_x = s[j].x - L.half, hi_x = s[j].x + L.half, lo_y = s[j].y - L.half, hi_y = s[j].y + L.half;
        const int cx0 = ground_cell(lo_x, L.x0, L.inv, L.nx), cx1 = ground_cell(hi_x, L.x0, L.inv, L.nx);
        const int cy0 = ground_cell(lo_y, L.y0, L.inv, L.ny), cy1 = ground_cell(hi_y, L.y0, L.inv, L.ny);
        float acc = none;
        auto range = [&](unsigned b, unsigned e) {
            for (unsigned k = b; k < e; ++k)
                if (lo_x <= s[k].x && s[k].x <= hi_x && lo_y <= s[k].y && s[k].y <= hi_y) acc = better(acc, s[k].z);
        };
        for (int cy = cy0; cy <= cy1; ++cy) {
            const int row = cy * L.nx;
            if (cy == cy0 || cy == cy1) { range(start[row + cx0], start[row + cx1 + 1]); continue; }
            range(start[row + cx0], start[row + cx0 + 1]);
            for (int cx = cx0 + 1; cx < cx1; ++cx) acc = better(acc, tab[row + cx]);
            if (cx1 != cx0) range(start[row + cx1], start[row + cx1 + 1]);
        }
        out[order[j]] = acc;
    }
}

int main(int argc, char** argv) {
    if (argc < 10) { std::printf("usage: ground_host in.f32 out.i32 max_window slope initial max cell base exponential\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 1;
    std::fseek(f, 0, SEEK_END);
    const size_t n = (size_t)std::ftell(f) / 12;
    std::fseek(f, 0, SEEK_SET);
    std::vector<P3> pts(n);
    if (n && std::fread(pts.data(), 12, n, f) != n) return 1;
    std::fclose(f);
    const PmfParams p{std::atoi(argv[3]), (float)std::atof(argv[4]), (float)std::atof(argv[5]), (float)std::atof(argv[6]),
                      (float)std::atof(argv[7]), (float)std::atof(argv[8]), std::atoi(argv[9])};
    float w[PMF_MAX_WINDOWS], h[PMF_MAX_WINDOWS];
    size_t nw = 0;
    if (pmf_windows(p, PMF_MAX_WINDOWS, w, h, &nw) != GROUND_PLAN_OK) { std::printf("bad parameters\n"); return 1; }
    std::vector<int32_t> ground(n);
    for (size_t i = 0; i < n; ++i) ground[i] = (int32_t)i;
    double total = 0;
    for (size_t it = 0; it < nw && !pts.empty(); ++it) {
        const auto t0 = std::chrono::steady_clock::now();
        const size_t m = pts.size();
        float xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
        for (const P3& q : pts) { xmin = std::min(xmin, q.x); xmax = std::max(xmax, q.x); ymin = std::min(ymin, q.y); ymax = std::max(ymax, q.y); }
        const GroundLattice L = ground_lattice(xmin, xmax, ymin, ymax, w[it], m);
        const size_t nc = ground_table_cells(L);
        std::vector<int> cell(m);
        std::vector<unsigned> start(nc + 1, 0), order(m);
        for (size_t i = 0; i < m; ++i) {
            cell[i] = ground_cell(pts[i].y, L.y0, L.inv, L.ny) * L.nx + ground_cell(pts[i].x, L.x0, L.inv, L.nx);
            ++start[cell[i] + 1];
        }
        for (size_t c = 0; c < nc; ++c) start[c + 1] += start[c];
        std::vector<unsigned> fill(start.begin(), start.end() - 1);
        for (size_t i = 0; i < m; ++i) order[fill[cell[i]]++] = (unsigned)i;
        std::vector<float> z(m), eroded, opened;
        for (size_t i = 0; i < m; ++i) z[i] = pts[i].z;
        pass(pts, L, cell, start, order, z, false, eroded);
        pass(pts, L, cell, start, order, eroded, true, opened);
        size_t k = 0;
        for (size_t i = 0; i < m; ++i)
            if ((z[i] - opened[i]) < h[it]) { pts[k] = pts[i]; ground[k] = ground[i]; ++k; }
        pts.resize(k);
        ground.resize(k);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        total += ms;
        std::printf("window %zu w %g h %g lattice %d x %d whole %d: %zu -> %zu  %.3f ms\n", it, w[it], h[it], L.nx, L.ny, L.whole, m, k, ms);
    }
    std::printf("total %.3f ms, ground %zu\n", total, ground.size());
    f = std::fopen(argv[2], "wb");
    if (!f) return 1;
    if (!ground.empty()) std::fwrite(ground.data(), 4, ground.size(), f);
    std::fclose(f);
    return 0;
}
