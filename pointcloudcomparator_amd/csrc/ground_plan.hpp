// ground_plan.hpp -- the host decisions of the morphological ground filter (ground.hip): the window table of
// pcl::ProgressiveMorphologicalFilter::extract, the refusals of its parameters, and the xy lattice one operator pass bins its
// points into.  Plain C++ (no HIP needed: tests/cpp/test_ground_plan.cpp compiles it on its own); the lattice functions are also
// compiled for the device, where k_ground_plan sizes the lattice from the bounds a kernel has just reduced, without a host wait.
//
// The reference's ground_segmentation (src/segmentation.cpp:330-387) runs VoxelGrid -> ProgressiveMorphologicalFilter (max
// window 20, slope 1, initial distance 0.5, max distance 3; PCL's defaults cell 1, base 2, exponential) -> ExtractIndices.
// PCL 1.7's filter is restated here as recalled from its published source.
#pragma once
#include <math.h>
#include <cmath>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PCC_GROUND_HD __host__ __device__
#else
#define PCC_GROUND_HD
#endif

namespace pcc {

constexpr int PMF_MAX_WINDOWS = 64;        // the library's cap on the window table
// The lattice table: nx * ny <= min(GROUND_MAX_CELLS, max(GROUND_MIN_CELLS, GROUND_CELLS_PER_POINT * points)).  The first is what
// the buffers hold and the radix partition's keys span (three 8-bit digits); the rest keeps a table in proportion to its cloud.
// The cell side is window / GROUND_CELLS_PER_WINDOW before coarsening.  Measured: EXPERIMENTS.md, "Ground filter".
#ifndef PCC_GROUND_MAX_CELLS
#define PCC_GROUND_MAX_CELLS (1 << 20)
#endif
#ifndef PCC_GROUND_CELLS_PER_WINDOW
#define PCC_GROUND_CELLS_PER_WINDOW 8
#endif
#ifndef PCC_GROUND_CELLS_PER_POINT
#define PCC_GROUND_CELLS_PER_POINT 1.0
#endif
constexpr int GROUND_MAX_CELLS = PCC_GROUND_MAX_CELLS;
constexpr int GROUND_MIN_CELLS = 16384;
constexpr double GROUND_CELLS_PER_POINT = PCC_GROUND_CELLS_PER_POINT;
constexpr int GROUND_CELLS_PER_WINDOW = PCC_GROUND_CELLS_PER_WINDOW;

enum { GROUND_PLAN_OK = 0, GROUND_PLAN_INVALID = 1, GROUND_PLAN_OVERFLOW = 2 };

// the seven parameters of the filter (PCL's setters)
struct PmfParams {
    int max_window_size;
    float slope, initial_distance, max_distance, cell_size, base;
    int exponential;
};

// nullptr when the parameters are taken; else why not.  PCL's loop never ends on the last three.
inline const char* pmf_refusal(const PmfParams& p) {
    if (!std::isfinite(p.slope) || !std::isfinite(p.initial_distance) || !std::isfinite(p.max_distance) || !std::isfinite(p.cell_size) || !std::isfinite(p.base))
        return "slope, distances, cell size and base must be finite";
    if (!(p.cell_size > 0.f)) return "cell size must be positive";
    if (p.exponential && !(p.base > 1.f)) return "base must exceed 1 for exponential windows";
    if (!p.exponential && !(p.base > 0.f)) return "base must be positive for linear windows";
    return nullptr;
}

// The first loop of ProgressiveMorphologicalFilter::extract.  windows / thresholds take min(*n_windows, capacity) entries;
// *n_windows is the table's length, PMF_MAX_WINDOWS + 1 standing for "more than the cap".  GROUND_PLAN_OVERFLOW when the table
// is longer than capacity or than PMF_MAX_WINDOWS.
inline int pmf_windows(const PmfParams& p, size_t capacity, float* windows, float* thresholds, size_t* n_windows) {
    *n_windows = 0;
    if (pmf_refusal(p)) return GROUND_PLAN_INVALID;
    size_t it = 0;
    float w = 0.0f, prev = 0.0f;
    while (w < (float)p.max_window_size) {
        if (it == (size_t)PMF_MAX_WINDOWS) { ++it; break; }
        w = p.exponential ? (float)((double)p.cell_size * (2.0 * std::pow((double)p.base, (double)it) + 1.0))
                          : (float)((double)p.cell_size * (2.0 * (double)(it + 1) * (double)p.base + 1.0));
        float h = p.initial_distance;
        if (it != 0) {
            const float dw = w - prev;        // three float operations, each rounded on its own
            const float sl = p.slope * dw;
            const float sc = sl * p.cell_size;
            h = sc + p.initial_distance;
        }
        if (h > p.max_distance) h = p.max_distance;
        if (it < capacity) { windows[it] = w; thresholds[it] = h; }
        prev = w;
        ++it;
    }
    *n_windows = it;
    return it > capacity || it > (size_t)PMF_MAX_WINDOWS ? GROUND_PLAN_OVERFLOW : GROUND_PLAN_OK;
}

// ---- the lattice of one operator pass ---------------------------------------------------------------------------------------
// Exactness never rests on how the lattice rounds: ground_cell is MONOTONE in v (a float subtraction, a multiplication by a
// value >= 0, two clamps, a truncation), so every point of the box [lo, hi] of an axis lies in the cells [cell(lo), cell(hi)],
// and a cell strictly between the two holds only points strictly inside the box.  The points, lo and hi all go through this
// one function.
struct GroundLattice {
    float x0, y0;   // the smallest finite x and y of the current points
    float inv;      // cells per unit, both axes
    float half;     // window / 2.0f
    int nx, ny;     // nx * ny <= ground_cell_cap(points) <= GROUND_MAX_CELLS
    int whole;      // 1: every point's box holds the whole cloud -- the pass is one global min / max
};

PCC_GROUND_HD inline int ground_cell(float v, float v0, float inv, int n) {
    float t = (v - v0) * inv;
    t = t > 0.f ? t : 0.f;  // (a NaN, inf * 0, lands here too)
    const float top = (float)(n - 1);
    t = t < top ? t : top;
    return (int)t;
}

PCC_GROUND_HD inline double ground_cell_cap(size_t points) {
    double cap = floor(GROUND_CELLS_PER_POINT * (double)points);
    if (cap < (double)GROUND_MIN_CELLS) cap = (double)GROUND_MIN_CELLS;
    return cap < (double)GROUND_MAX_CELLS ? cap : (double)GROUND_MAX_CELLS;
}

// bounds of the finite points (min > max: there is none), the window and the number of points -> the lattice
PCC_GROUND_HD inline GroundLattice ground_lattice(float xmin, float xmax, float ymin, float ymax, float window, size_t points) {
    GroundLattice L;
    L.x0 = xmin; L.y0 = ymin;
    L.half = window / 2.0f;
    L.nx = L.ny = 1;
    L.inv = 0.f;
    L.whole = 0;
    if (!(xmin <= xmax) || !(ymin <= ymax)) { L.x0 = L.y0 = 0.f; return L; }
    // float subtraction and addition are monotone in the point, so the extreme points decide for all
    L.whole = (xmax - L.half <= xmin && xmin + L.half >= xmax && ymax - L.half <= ymin && ymin + L.half >= ymax) ? 1 : 0;
    const double ex = (double)xmax - (double)xmin, ey = (double)ymax - (double)ymin;
    double side = (double)window / GROUND_CELLS_PER_WINDOW;
    if (!(side > 0.0) || L.whole) return L;  // (the whole-cloud pass reads no table)
    const double cap = ground_cell_cap(points);
    for (int i = 0; i < 2200; ++i) {  // side doubles: at most the exponent range of a double
        const double fx = floor(ex / side) + 1.0, fy = floor(ey / side) + 1.0;
        if (fx * fy <= cap) {
            const float inv = (float)(1.0 / side);
            if (inv > 0.f && inv <= 3.0e38f) { L.nx = (int)fx; L.ny = (int)fy; L.inv = inv; }
            return L;
        }
        side *= 2.0;
    }
    return L;
}

// lattice sizing for the host (tests and the host mirror of the measurement tool)
inline size_t ground_table_cells(const GroundLattice& L) { return (size_t)L.nx * (size_t)L.ny; }

}  // namespace pcc
