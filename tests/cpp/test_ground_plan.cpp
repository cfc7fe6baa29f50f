// test_ground_plan.cpp -- csrc/ground_plan.hpp on the CPU (no library, no GPU):
//   1. the window table: the reference's parameters, the linear form, the cap at max_distance, capacity and the library's cap
//   2. every refusal
//   3. the lattice: its size stays under the cap, ground_cell is monotone and stays inside the table, the whole-cloud test
//   4. the walk the kernels do over such a lattice (interior cells by their aggregate, rim rows point by point) against the
//      brute-force box test, on scenes whose box edges fall on points and on geo-referenced coordinates
#include "ground_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

using namespace pcc;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static void test_windows() {
    float w[PMF_MAX_WINDOWS], h[PMF_MAX_WINDOWS];
    size_t n = 0;
    const PmfParams ref{20, 1.f, 0.5f, 3.f, 1.f, 2.f, 1};
    CHECK(pmf_windows(ref, PMF_MAX_WINDOWS, w, h, &n) == GROUND_PLAN_OK && n == 5);
    const float ew[5] = {3, 5, 9, 17, 33}, eh[5] = {0.5f, 2.5f, 3.f, 3.f, 3.f};
    for (int i = 0; i < 5; ++i) CHECK(w[i] == ew[i] && h[i] == eh[i]);
    PmfParams lin = ref;
    lin.exponential = 0;
    CHECK(pmf_windows(lin, PMF_MAX_WINDOWS, w, h, &n) == GROUND_PLAN_OK);            // 5, 9, 13, 17, 21: 21 is pushed
    CHECK(n == 5 && w[0] == 5.f && w[4] == 21.f && h[0] == 0.5f && h[1] == 3.f);     // 1 * 4 * 1 + 0.5 = 4.5 -> 3
    // capacity: the first entries are written, the length is reported
    float w3[3] = {-1, -1, -1}, h3[3] = {-1, -1, -1};
    CHECK(pmf_windows(ref, 2, w3, h3, &n) == GROUND_PLAN_OVERFLOW && n == 5 && w3[0] == 3.f && w3[1] == 5.f && w3[2] == -1.f && h3[2] == -1.f);
    CHECK(pmf_windows(ref, 0, nullptr, nullptr, &n) == GROUND_PLAN_OVERFLOW && n == 5);
    // the library's cap
    PmfParams slow = ref;
    slow.base = 1.0001f;
    slow.max_window_size = 1000;
    CHECK(pmf_windows(slow, PMF_MAX_WINDOWS, w, h, &n) == GROUND_PLAN_OVERFLOW && n == (size_t)PMF_MAX_WINDOWS + 1);
    PmfParams none = ref;
    none.max_window_size = 0;
    CHECK(pmf_windows(none, PMF_MAX_WINDOWS, w, h, &n) == GROUND_PLAN_OK && n == 0);
}

static void test_refusals() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const PmfParams ok{20, 1.f, 0.5f, 3.f, 1.f, 2.f, 1};
    CHECK(pmf_refusal(ok) == nullptr);
    for (float bad : {nan, inf, -inf}) {
        PmfParams p = ok; p.slope = bad; CHECK(pmf_refusal(p));
        p = ok; p.initial_distance = bad; CHECK(pmf_refusal(p));
        p = ok; p.max_distance = bad; CHECK(pmf_refusal(p));
        p = ok; p.cell_size = bad; CHECK(pmf_refusal(p));
        p = ok; p.base = bad; CHECK(pmf_refusal(p));
    }
    PmfParams p = ok; p.cell_size = 0.f; CHECK(pmf_refusal(p));
    p = ok; p.cell_size = -1.f; CHECK(pmf_refusal(p));
    p = ok; p.base = 1.f; CHECK(pmf_refusal(p));
    p = ok; p.base = 1.f; p.exponential = 0; CHECK(!pmf_refusal(p));
    p = ok; p.base = 0.f; p.exponential = 0; CHECK(pmf_refusal(p));
    float w[4], h[4];
    size_t n = 9;
    p = ok; p.base = 0.5f;
    CHECK(pmf_windows(p, 4, w, h, &n) == GROUND_PLAN_INVALID && n == 0);
}

struct P3 { float x, y, z; };

// the operator pass as the kernels run it, min (flip false) or max
static std::vector<float> lattice_pass(const std::vector<P3>& pts, const std::vector<float>& vals, float window, bool take_max,
                                       GroundLattice* used) {
    const size_t m = pts.size();
    float xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
    for (const P3& p : pts) { xmin = std::min(xmin, p.x); xmax = std::max(xmax, p.x); ymin = std::min(ymin, p.y); ymax = std::max(ymax, p.y); }
    const GroundLattice L = ground_lattice(xmin, xmax, ymin, ymax, window, m);
    *used = L;
    const size_t nc = ground_table_cells(L);
    std::vector<int> cell(m);
    std::vector<unsigned> start(nc + 1, 0);
    for (size_t i = 0; i < m; ++i) {
        cell[i] = ground_cell(pts[i].y, L.y0, L.inv, L.ny) * L.nx + ground_cell(pts[i].x, L.x0, L.inv, L.nx);
        ++start[cell[i] + 1];
    }
    for (size_t c = 0; c < nc; ++c) start[c + 1] += start[c];
    std::vector<unsigned> fill(start.begin(), start.end() - 1), order(m);
    for (size_t i = 0; i < m; ++i) order[fill[cell[i]]++] = (unsigned)i;
    const float none = take_max ? -INFINITY : INFINITY;
    auto better = [&](float a, float b) { return take_max ? std::max(a, b) : std::min(a, b); };
    std::vector<float> tab(nc, none);
    float all = none;
    for (size_t i = 0; i < m; ++i) { tab[cell[i]] = better(tab[cell[i]], vals[i]); all = better(all, vals[i]); }
    std::vector<float> out(m);
    for (size_t i = 0; i < m; ++i) {
        if (L.whole) { out[i] = all; continue; }
        const float lo_x = pts[i].x - L.half, hi_x = pts[i].x + L.half, lo_y = pts[i].y - L.half, hi_y = pts[i].y + L.half;
        const int cx0 = ground_cell(lo_x, L.x0, L.inv, L.nx), cx1 = ground_cell(hi_x, L.x0, L.inv, L.nx);
        const int cy0 = ground_cell(lo_y, L.y0, L.inv, L.ny), cy1 = ground_cell(hi_y, L.y0, L.inv, L.ny);
        float acc = none;
        auto range = [&](unsigned b, unsigned e) {
            for (unsigned k = b; k < e; ++k) {
                const P3& q = pts[order[k]];
                if (lo_x <= q.x && q.x <= hi_x && lo_y <= q.y && q.y <= hi_y) acc = better(acc, vals[order[k]]);
            }
        };
        for (int cy = cy0; cy <= cy1; ++cy) {
            const int row = cy * L.nx;
            if (cy == cy0 || cy == cy1) { range(start[row + cx0], start[row + cx1 + 1]); continue; }
            range(start[row + cx0], start[row + cx0 + 1]);
            for (int cx = cx0 + 1; cx < cx1; ++cx) acc = better(acc, tab[row + cx]);
            if (cx1 != cx0) range(start[row + cx1], start[row + cx1 + 1]);
        }
        out[i] = acc;
    }
    return out;
}

static std::vector<float> brute_pass(const std::vector<P3>& pts, const std::vector<float>& vals, float window, bool take_max) {
    const float half = window / 2.0f;
    std::vector<float> out(pts.size());
    for (size_t i = 0; i < pts.size(); ++i) {
        const float lo_x = pts[i].x - half, hi_x = pts[i].x + half, lo_y = pts[i].y - half, hi_y = pts[i].y + half;
        float acc = take_max ? -INFINITY : INFINITY;
        for (size_t j = 0; j < pts.size(); ++j)
            if (lo_x <= pts[j].x && pts[j].x <= hi_x && lo_y <= pts[j].y && pts[j].y <= hi_y)
                acc = take_max ? std::max(acc, vals[j]) : std::min(acc, vals[j]);
        out[i] = acc;
    }
    return out;
}

static void check_scene(const char* name, const std::vector<P3>& pts, float window, bool expect_whole) {
    std::vector<float> z(pts.size());
    for (size_t i = 0; i < pts.size(); ++i) z[i] = pts[i].z;
    for (int mx = 0; mx < 2; ++mx) {
        GroundLattice L;
        const std::vector<float> a = lattice_pass(pts, z, window, mx != 0, &L), b = brute_pass(pts, z, window, mx != 0);
        size_t bad = 0;
        for (size_t i = 0; i < pts.size(); ++i) bad += a[i] != b[i];
        if (bad) std::printf("%s window %g max %d: %zu of %zu differ (lattice %d x %d)\n", name, window, mx, bad, pts.size(), L.nx, L.ny);
        CHECK(bad == 0);
        CHECK(ground_table_cells(L) <= (size_t)GROUND_MAX_CELLS && L.nx >= 1 && L.ny >= 1);
        CHECK((L.whole != 0) == expect_whole);
    }
}

static void test_lattice() {
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> u(0.f, 1.f);
    // monotone and inside the table, whatever the arguments
    const GroundLattice L = ground_lattice(-3.f, 40.f, 512000.f, 512007.f, 0.7f, 1000);
    CHECK(ground_table_cells(L) <= (size_t)GROUND_MAX_CELLS && !L.whole);
    float prev = -INFINITY;
    int pc = 0;
    for (float v : {-INFINITY, -1e30f, -4.f, -3.f, -2.99f, 0.f, 0.0875f, 0.175f, 5.f, 39.99f, 40.f, 41.f, 1e30f, INFINITY}) {
        const int c = ground_cell(v, L.x0, L.inv, L.nx);
        CHECK(c >= 0 && c < L.nx && c >= pc && v >= prev);
        pc = c; prev = v;
    }
    CHECK(ground_cell(NAN, L.x0, L.inv, L.nx) == 0);
    // no finite point, one point, a window that underflows, coordinates at the float range's ends
    GroundLattice E = ground_lattice(INFINITY, -INFINITY, INFINITY, -INFINITY, 1.f, 0);
    CHECK(E.nx == 1 && E.ny == 1 && !E.whole);
    E = ground_lattice(2.f, 2.f, 3.f, 3.f, 1.f, 1);
    CHECK(E.whole == 1);
    E = ground_lattice(-3e38f, 3e38f, -3e38f, 3e38f, 1e-30f, 5000000);
    CHECK(ground_table_cells(E) <= (size_t)GROUND_MAX_CELLS && !E.whole && E.nx >= 1 && E.ny >= 1);
    CHECK(ground_cell(3e38f, E.x0, E.inv, E.nx) < E.nx && ground_cell(-3e38f, E.x0, E.inv, E.nx) == 0);
    E = ground_lattice(0.f, 1.f, 0.f, 1.f, 1e-44f, 100);
    CHECK(ground_table_cells(E) <= (size_t)GROUND_MAX_CELLS);

    // scenes
    std::vector<P3> terrain(1500);
    for (P3& p : terrain) p = {4.f * u(rng), 4.f * u(rng), u(rng)};
    check_scene("terrain", terrain, 1e-4f, false);
    check_scene("terrain", terrain, 0.1f, false);
    check_scene("terrain", terrain, 0.3f, false);
    check_scene("terrain", terrain, 1.7f, false);
    check_scene("terrain", terrain, 7.9f, false);
    check_scene("terrain", terrain, 8.5f, true);
    std::vector<P3> lat;
    for (int y = 0; y < 9; ++y)
        for (int x = 0; x < 12; ++x) lat.push_back({0.25f * x, 0.25f * y, u(rng)});
    check_scene("lattice", lat, 0.5f, false);
    check_scene("lattice", lat, 0.25f, false);
    std::vector<P3> geo(800);
    for (P3& p : geo) p = {512000.f + 30.f * u(rng), 4400000.f + 30.f * u(rng), u(rng)};
    check_scene("geo", geo, 0.7f, false);
    check_scene("geo", geo, 3.f, false);
    check_scene("geo", geo, 33.f, false);
    std::vector<P3> rowpts(300);
    for (P3& p : rowpts) p = {-50.f + 100.f * u(rng), 7.f, u(rng)};
    check_scene("row", rowpts, 0.5f, false);
    std::vector<P3> dup(200);
    for (size_t i = 0; i < dup.size(); ++i) dup[i] = {(float)(i % 5), (float)(i % 3), u(rng)};
    check_scene("duplicates", dup, 1.f, false);
    check_scene("one", std::vector<P3>{{1.f, 2.f, 3.f}}, 1.f, true);
}

int main() {
    test_windows();
    test_refusals();
    test_lattice();
    if (failures) { std::printf("test_ground_plan: %d failures\n", failures); return 1; }
    std::printf("test_ground_plan: ok\n");
    return 0;
}
