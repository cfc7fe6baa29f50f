// ground.hip -- the reference's ground_segmentation (src/segmentation.cpp:330-387) on the device (gfx950): pcl::VoxelGrid ->
// pcl::ProgressiveMorphologicalFilter -> pcl::ExtractIndices, and the filter's operator on its own.
//
// One operator pass is order-independent min / max of z over axis-aligned xy boxes.  Per window the current points are binned
// into an xy lattice (ground_plan.hpp: sized on the device from bounds a kernel has just reduced -- no host wait), sorted by cell
// with the stable radix partition of segment.hip (extract_order: the cell is the label, the cell starts are its offsets, a
// non-finite point is a point left out), and copied once into cell order.  Then, per min or max:
//   k_ground_agg   one lane per point in cell order: the lanes of a wave that share a cell reduce among themselves (the order is
//                  sorted, so they are neighbours) and the last of them does ONE integer atomicMin on the cell's table word
//   k_ground_box   one lane per point in cell order: the cells strictly inside the box's cell range give their aggregate, the
//                  rim cells have their points tested against the box's edges -- a rim row of cells is one contiguous range of
//                  the sorted copy
// Values travel as integer keys whose order is the floats' order (max: the complement), so both directions are a min, the
// atomics are integer and the result does not depend on their order.  ground_cell is monotone: the lattice decides only how
// much work a box takes, never what it holds.
#include "entry.hpp"
#include "ground_plan.hpp"
#include <algorithm>
#include <cmath>
#include <vector>

namespace pcc {

struct GroundState {         // device words of the pass in flight
    unsigned int bounds[4];  // keys of min x, max x (complement), min y, max y (complement) over the finite points
    GroundLattice lat;
};

struct GroundScratch : Scratch {
    static constexpr ScratchSlot slot = SCRATCH_GROUND;
    DevBuf xy[2], z[2], idx[2];  // the current points of the filter: float2[m], float[m], their original indices; ping-pong
    DevBuf cell;                 // int32[m]: the lattice cell of every point, -1 for a non-finite one
    DevBuf sxy, scell, skey;     // float2[m], uint32[m], uint32[m]: xy, the cells and the value keys in cell order
    DevBuf eroded, opened;       // float[m]: the first pass of OPEN / CLOSE; the operator's result inside the filter
    DevBuf keep;                 // int32[m]: 0 keep, -1 drop; pcc_ground_segmentation: 0 ground, 1 object
    DevBuf tab, start;           // uint32[cap + 1] each: the cells' aggregates, then the whole cloud's; the cell starts
    DevBuf state;                // GroundState
    DevBuf cloud, out_rec;       // pcc_ground_segmentation: the filtered cloud; the gathered records of a caller in host memory
    DevBuf out_z, out_index;     // results staged for a caller in host memory
};

namespace {

constexpr unsigned int KEY_NONE = 0xffffffffu;  // the identity of min over keys

// an integer whose unsigned order is the float's order (-0 below +0); finite values only
__device__ __forceinline__ unsigned int ord_key(float f) {
    const unsigned int u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord_val(unsigned int k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ unsigned int umin(unsigned int a, unsigned int b) { return a < b ? a : b; }

inline int ground_blocks(size_t n) {
    const size_t b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

__global__ void __launch_bounds__(256)
k_ground_load(const char* __restrict__ raw, size_t stride, size_t n, float2* __restrict__ xy, float* __restrict__ z,
              int32_t* __restrict__ idx) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float* p = reinterpret_cast<const float*>(raw + i * stride);
        xy[i] = make_float2(p[0], p[1]);
        z[i] = p[2];
        idx[i] = (int32_t)i;
    }
}

// bounds of the finite points: every lane keeps four keys, the workgroup reduces them, one atomicMin per key and workgroup
__global__ void __launch_bounds__(256)
k_ground_bounds(const float2* __restrict__ xy, const float* __restrict__ z, size_t m, GroundState* __restrict__ st) {
    __shared__ unsigned int part[4][4];
    unsigned int k0 = KEY_NONE, k1 = KEY_NONE, k2 = KEY_NONE, k3 = KEY_NONE;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (size_t)gridDim.x * blockDim.x) {
        const float2 p = xy[i];
        if (!finite3(p.x, p.y, z[i])) continue;
        const unsigned int kx = ord_key(p.x), ky = ord_key(p.y);
        k0 = umin(k0, kx); k1 = umin(k1, ~kx); k2 = umin(k2, ky); k3 = umin(k3, ~ky);
    }
    for (int d = 1; d < 64; d <<= 1) {
        k0 = umin(k0, (unsigned int)__shfl_xor((int)k0, d));
        k1 = umin(k1, (unsigned int)__shfl_xor((int)k1, d));
        k2 = umin(k2, (unsigned int)__shfl_xor((int)k2, d));
        k3 = umin(k3, (unsigned int)__shfl_xor((int)k3, d));
    }
    const unsigned int lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) { part[wave][0] = k0; part[wave][1] = k1; part[wave][2] = k2; part[wave][3] = k3; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const unsigned int k = umin(umin(part[0][threadIdx.x], part[1][threadIdx.x]), umin(part[2][threadIdx.x], part[3][threadIdx.x]));
        if (k != KEY_NONE) atomicMin(&st->bounds[threadIdx.x], k);
    }
}

// the lattice of this window from the bounds (one lane)
__global__ void k_ground_plan(GroundState* __restrict__ st, float window, size_t m) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const unsigned int b0 = st->bounds[0], b1 = st->bounds[1], b2 = st->bounds[2], b3 = st->bounds[3];
    const bool none = b0 == KEY_NONE;  // (the key of no finite value)
    const float xmin = none ? INFINITY : ord_val(b0), xmax = none ? -INFINITY : ord_val(~b1);
    const float ymin = none ? INFINITY : ord_val(b2), ymax = none ? -INFINITY : ord_val(~b3);
    st->lat = ground_lattice(xmin, xmax, ymin, ymax, window, m);
}

__global__ void __launch_bounds__(256)
k_ground_bin(const float2* __restrict__ xy, const float* __restrict__ z, size_t m, const GroundState* __restrict__ st,
             int32_t* __restrict__ cell) {
    const GroundLattice L = st->lat;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (size_t)gridDim.x * blockDim.x) {
        const float2 p = xy[i];
        int32_t c = -1;
        if (finite3(p.x, p.y, z[i])) c = ground_cell(p.y, L.y0, L.inv, L.ny) * L.nx + ground_cell(p.x, L.x0, L.inv, L.nx);
        cell[i] = c;  // (0 <= c < nx * ny <= GROUND_MAX_CELLS)
    }
}

// xy and the cells in cell order; a non-finite point, which lies behind the finite ones, carries the cell `cap`
__global__ void __launch_bounds__(256)
k_ground_sorted(const float2* __restrict__ xy, const int32_t* __restrict__ cell, const unsigned int* __restrict__ order, size_t m,
                unsigned int cap, float2* __restrict__ sxy, unsigned int* __restrict__ scell) {
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (size_t)gridDim.x * blockDim.x) {
        const unsigned int p = order[j];
        const int32_t c = cell[p];
        sxy[j] = xy[p];
        scell[j] = c < 0 ? cap : (unsigned int)c;
    }
}

// start[c] = the first sorted position whose cell is >= c, c = 0 .. cap: every cell looks its own start up (a binary search
// over the sorted cells), so empty cells cost what full ones do.  start[cap] counts the finite points.
__global__ void __launch_bounds__(256)
k_ground_starts(const unsigned int* __restrict__ scell, size_t m, unsigned int cap, unsigned int* __restrict__ start) {
    for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c <= cap; c += (size_t)gridDim.x * blockDim.x) {
        size_t lo = 0, hi = m;  // (at most 32 halvings: m < 2^31)
        while (lo < hi) {
            const size_t mid = (lo + hi) >> 1;
            if (scell[mid] < c) lo = mid + 1;
            else hi = mid;
        }
        start[c] = (unsigned int)lo;
    }
}

// skey[j] = key of vals[order[j]] (flip = ~0: its complement, so that min is max); tab[c] = min over cell c; tab[cap] = min over
// all.  tab holds KEY_NONE everywhere before.
__global__ void __launch_bounds__(256)
k_ground_agg(const float* __restrict__ vals, const unsigned int* __restrict__ order, const unsigned int* __restrict__ scell,
             const unsigned int* __restrict__ start, size_t m, unsigned int cap, unsigned int flip, unsigned int* __restrict__ skey,
             unsigned int* __restrict__ tab) {
    __shared__ unsigned int part[4];
    const size_t nf = start[cap] < m ? start[cap] : m;
    const unsigned int lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned int all = KEY_NONE;
    // (the trip count is uniform over the workgroup: every lane takes part in the exchanges)
    for (size_t base = (size_t)blockIdx.x * blockDim.x; base < nf; base += (size_t)gridDim.x * blockDim.x) {
        const size_t j = base + threadIdx.x;
        const bool valid = j < nf;
        int c = -1;
        unsigned int v = KEY_NONE;
        if (valid) {
            c = (int)scell[j];  // (< cap: a finite point)
            v = ord_key(vals[order[j]]) ^ flip;
            skey[j] = v;
        }
        all = umin(all, v);
        // the lanes of a cell are neighbours: an inclusive min scan that stops at the cell's first lane
        for (int d = 1; d < 64; d <<= 1) {
            const int c2 = __shfl_up(c, d);
            const unsigned int v2 = (unsigned int)__shfl_up((int)v, d);
            if ((int)lane >= d && c2 == c) v = umin(v, v2);
        }
        const int next = __shfl_down(c, 1);
        if (valid && (lane == 63u || next != c)) atomicMin(&tab[c], v);  // (the cell's last lane of this wave holds its minimum)
    }
    for (int d = 1; d < 64; d <<= 1) all = umin(all, (unsigned int)__shfl_xor((int)all, d));
    if (lane == 0) part[wave] = all;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int k = umin(umin(part[0], part[1]), umin(part[2], part[3]));
        if (k != KEY_NONE) atomicMin(&tab[cap], k);
    }
}

// the points sxy[b .. e) against the box, their keys into acc
__device__ __forceinline__ unsigned int box_range(const float2* __restrict__ sxy, const unsigned int* __restrict__ skey, unsigned int b,
                                                  unsigned int e, float lo_x, float hi_x, float lo_y, float hi_y, unsigned int acc) {
    for (unsigned int k = b; k < e; ++k) {
        const float2 q = sxy[k];
        if (lo_x <= q.x && q.x <= hi_x && lo_y <= q.y && q.y <= hi_y) acc = umin(acc, skey[k]);
    }
    return acc;
}

// out[order[j]] = the min (flip: max) over the box of sorted point j; the non-finite points behind them keep their input
__global__ void __launch_bounds__(256)
k_ground_box(const float2* __restrict__ sxy, const unsigned int* __restrict__ skey, const unsigned int* __restrict__ order,
             const unsigned int* __restrict__ start, const unsigned int* __restrict__ tab, const GroundState* __restrict__ st,
             const float* __restrict__ vals, size_t m, unsigned int cap, unsigned int flip, float* __restrict__ out) {
    const GroundLattice L = st->lat;
    const size_t nf = start[cap] < m ? start[cap] : m;
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (size_t)gridDim.x * blockDim.x) {
        const unsigned int p = order[j];
        if (j >= nf) { out[p] = vals[p]; continue; }
        unsigned int acc = KEY_NONE;
        if (L.whole) {
            acc = tab[cap];
        } else {
            const float2 c = sxy[j];
            const float lo_x = c.x - L.half, hi_x = c.x + L.half, lo_y = c.y - L.half, hi_y = c.y + L.half;
            // the cells of the edges, by the function that binned the points: 0 <= cx0 <= cx1 < nx, 0 <= cy0 <= cy1 < ny
            const int cx0 = ground_cell(lo_x, L.x0, L.inv, L.nx), cx1 = ground_cell(hi_x, L.x0, L.inv, L.nx);
            const int cy0 = ground_cell(lo_y, L.y0, L.inv, L.ny), cy1 = ground_cell(hi_y, L.y0, L.inv, L.ny);
            for (int cy = cy0; cy <= cy1; ++cy) {
                const int row = cy * L.nx;
                if (cy == cy0 || cy == cy1) {  // a rim row: its cells cx0 .. cx1 are one range of the sorted copy
                    acc = box_range(sxy, skey, start[row + cx0], start[row + cx1 + 1], lo_x, hi_x, lo_y, hi_y, acc);
                    continue;
                }
                acc = box_range(sxy, skey, start[row + cx0], start[row + cx0 + 1], lo_x, hi_x, lo_y, hi_y, acc);
                for (int cx = cx0 + 1; cx < cx1; ++cx) acc = umin(acc, tab[row + cx]);  // wholly inside the box
                if (cx1 != cx0) acc = box_range(sxy, skey, start[row + cx1], start[row + cx1 + 1], lo_x, hi_x, lo_y, hi_y, acc);
            }
        }
        out[p] = ord_val(acc ^ flip);  // (the point itself lies in its box: acc is a key)
    }
}

// keep[i] = 0 when point i stays ground under threshold h, else -1 (opened == nullptr: every finite point stays)
__global__ void __launch_bounds__(256)
k_ground_keep(const float2* __restrict__ xy, const float* __restrict__ z, const float* __restrict__ opened, size_t m, float h,
              int32_t* __restrict__ keep) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (size_t)gridDim.x * blockDim.x) {
        const float zi = z[i];
        const float2 p = xy[i];
        bool k = finite3(p.x, p.y, zi);
        if (k && opened) k = (zi - opened[i]) < h;
        keep[i] = k ? 0 : -1;
    }
}

__global__ void __launch_bounds__(256)
k_ground_compact(const unsigned int* __restrict__ order, size_t count, const float2* __restrict__ xy_in, const float* __restrict__ z_in,
                 const int32_t* __restrict__ idx_in, float2* __restrict__ xy_out, float* __restrict__ z_out,
                 int32_t* __restrict__ idx_out) {
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < count; j += (size_t)gridDim.x * blockDim.x) {
        const unsigned int p = order[j];
        xy_out[j] = xy_in[p];
        z_out[j] = z_in[p];
        idx_out[j] = idx_in[p];
    }
}

// label[i] = 1 for all i < n (ground == nullptr), or label[ground[j]] = 0 for j < count
__global__ void __launch_bounds__(256)
k_ground_mark(const int32_t* __restrict__ ground, size_t count, int32_t* __restrict__ label) {
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < count; j += (size_t)gridDim.x * blockDim.x) {
        if (ground) label[ground[j]] = 0;
        else label[j] = 1;
    }
}

#define GROUND_LAUNCH(kernel, blocks, ...)                                                   \
    do {                                                                                     \
        hipLaunchKernelGGL(kernel, dim3((unsigned int)(blocks)), dim3(256), 0, s, __VA_ARGS__); \
        PCC_HIP(hipGetLastError());                                                          \
    } while (0)

// What the passes of one window share: the lattice of `window` over the m points (xy, z), their cells, the order by cell and
// (in SegmentScratch), xy and the cells in cell order, the cell starts.  Everything enqueued.  The tables hold cap + 1 words, cap the
// most cells a lattice over m points may have (ground_cell_cap: known to the host from m alone); the partition takes two 8-bit
// digits of the cell below 2^16 cells and three above.
struct GroundPass {
    const unsigned int* order = nullptr;
    const unsigned int* start = nullptr;  // uint32[cap + 1]; the last entry counts the finite points
    unsigned int cap = 0;
};
int ground_pass_setup(pcc_index* ix, const float2* xy, const float* z, size_t m, float window, GroundPass* P) {
    hipStream_t s = ix->stream;
    GroundScratch* g = scratch<GroundScratch>(ix);
    const unsigned int cap = (unsigned int)ground_cell_cap(m);
    P->cap = cap;
    PCC_TRY(g->cell.reserve(m * sizeof(int32_t)));
    PCC_TRY(g->sxy.reserve(m * sizeof(float2)));
    PCC_TRY(g->scell.reserve(m * sizeof(unsigned int)));
    PCC_TRY(g->skey.reserve(m * sizeof(unsigned int)));
    PCC_TRY(g->tab.reserve(((size_t)cap + 1) * sizeof(unsigned int)));
    PCC_TRY(g->start.reserve(((size_t)cap + 1) * sizeof(unsigned int)));
    PCC_TRY(g->state.reserve(sizeof(GroundState)));
    GroundState* st = g->state.as<GroundState>();
    PCC_HIP(hipMemsetAsync(st->bounds, 0xff, sizeof(st->bounds), s));
    const int nb = ground_blocks(m);
    GROUND_LAUNCH(k_ground_bounds, nb, xy, z, m, st);
    hipLaunchKernelGGL(k_ground_plan, dim3(1), dim3(64), 0, s, st, window, m);
    PCC_HIP(hipGetLastError());
    GROUND_LAUNCH(k_ground_bin, nb, xy, z, m, (const GroundState*)st, g->cell.as<int32_t>());
    PCC_TRY(extract_order(ix, g->cell.as<int32_t>(), m, (int32_t)cap, &P->order, nullptr));
    GROUND_LAUNCH(k_ground_sorted, nb, xy, (const int32_t*)g->cell.as<int32_t>(), P->order, m, cap, g->sxy.as<float2>(),
                  g->scell.as<unsigned int>());
    GROUND_LAUNCH(k_ground_starts, ground_blocks((size_t)cap + 1), (const unsigned int*)g->scell.as<unsigned int>(), m, cap,
                  g->start.as<unsigned int>());
    P->start = g->start.as<unsigned int>();
    return PCC_OK;
}
// out = min (maximum: max) of vals over every point's box
int ground_pass(pcc_index* ix, const GroundPass& P, const float* vals, size_t m, bool maximum, float* out) {
    hipStream_t s = ix->stream;
    GroundScratch* g = scratch<GroundScratch>(ix);
    const unsigned int flip = maximum ? 0xffffffffu : 0u;
    unsigned int* tab = g->tab.as<unsigned int>();
    PCC_HIP(hipMemsetAsync(tab, 0xff, ((size_t)P.cap + 1) * sizeof(unsigned int), s));
    const int nb = ground_blocks(m);
    GROUND_LAUNCH(k_ground_agg, nb, vals, P.order, (const unsigned int*)g->scell.as<unsigned int>(), P.start, m, P.cap, flip,
                  g->skey.as<unsigned int>(), tab);
    GROUND_LAUNCH(k_ground_box, nb, (const float2*)g->sxy.as<float2>(), (const unsigned int*)g->skey.as<unsigned int>(), P.order, P.start,
                  (const unsigned int*)tab, (const GroundState*)g->state.as<GroundState>(), vals, m, P.cap, flip, out);
    return PCC_OK;
}
// the operator `op` over (xy, z)[m] with the window's passes set up -> out[m]
int ground_operator(pcc_index* ix, const GroundPass& P, const float* z, size_t m, int op, float* out) {
    GroundScratch* g = scratch<GroundScratch>(ix);
    if (op == PCC_MORPH_ERODE || op == PCC_MORPH_DILATE) return ground_pass(ix, P, z, m, op == PCC_MORPH_DILATE, out);
    PCC_TRY(g->eroded.reserve(m * sizeof(float)));
    PCC_TRY(ground_pass(ix, P, z, m, op == PCC_MORPH_CLOSE, g->eroded.as<float>()));
    return ground_pass(ix, P, g->eroded.as<float>(), m, op == PCC_MORPH_OPEN, out);
}

// the cloud on the device: the caller's own array, or a host cloud's copy in q_raw (up to the last byte read)
int ground_stage(pcc_index* ix, const void* pts, size_t n, size_t stride, int mem, const void** src) {
    *src = pts;
    if (mem != PCC_MEM_HOST) return PCC_OK;
    PCC_TRY(ix->q_raw.reserve(n * stride));
    PCC_HIP(hipMemcpyAsync(ix->q_raw.p, pts, (n - 1) * stride + 12, hipMemcpyHostToDevice, ix->stream));
    *src = ix->q_raw.p;
    return PCC_OK;
}

int ground_load(pcc_index* ix, const void* dpts, size_t n, size_t stride) {
    hipStream_t s = ix->stream;
    GroundScratch* g = scratch<GroundScratch>(ix);
    PCC_TRY(g->xy[0].reserve(n * sizeof(float2)));
    PCC_TRY(g->z[0].reserve(n * sizeof(float)));
    PCC_TRY(g->idx[0].reserve(n * sizeof(int32_t)));
    GROUND_LAUNCH(k_ground_load, ground_blocks(n), static_cast<const char*>(dpts), stride, n, g->xy[0].as<float2>(), g->z[0].as<float>(),
                  g->idx[0].as<int32_t>());
    return PCC_OK;
}

// The second loop of ProgressiveMorphologicalFilter::extract over a cloud on the device (n > 0): *ground (device, in
// GroundScratch) are the original indices of the *n_ground points that remain, ascending.  One wait per window.
int pmf_run(pcc_index* ix, const void* dpts, size_t n, size_t stride, const float* windows, const float* thresholds, size_t n_windows,
            const int32_t** ground, size_t* n_ground, size_t* pass_sizes, size_t max_passes) {
    hipStream_t s = ix->stream;
    GroundScratch* g = scratch<GroundScratch>(ix);
    PCC_TRY(ground_load(ix, dpts, n, stride));
    PCC_TRY(g->xy[1].reserve(n * sizeof(float2)));
    PCC_TRY(g->z[1].reserve(n * sizeof(float)));
    PCC_TRY(g->idx[1].reserve(n * sizeof(int32_t)));
    PCC_TRY(g->keep.reserve(n * sizeof(int32_t)));
    PCC_TRY(g->opened.reserve(n * sizeof(float)));
    int cur = 0;
    size_t m = n;
    // without a window only the non-finite points leave
    const size_t rounds = n_windows ? n_windows : 1;
    for (size_t it = 0; it < rounds; ++it) {
        if (m) {
            const float2* xy = g->xy[cur].as<float2>();
            const float* z = g->z[cur].as<float>();
            const float* opened = nullptr;
            if (n_windows) {
                GroundPass P;
                PCC_TRY(ground_pass_setup(ix, xy, z, m, windows[it], &P));
                PCC_TRY(ground_operator(ix, P, z, m, PCC_MORPH_OPEN, g->opened.as<float>()));
                opened = g->opened.as<float>();
            }
            GROUND_LAUNCH(k_ground_keep, ground_blocks(m), xy, z, opened, m, n_windows ? thresholds[it] : 0.f, g->keep.as<int32_t>());
            // the survivors in front, in their order: the stable partition with one cluster
            const unsigned int *order = nullptr, *d_offsets = nullptr;
            PCC_TRY(extract_order(ix, g->keep.as<int32_t>(), m, 1, &order, &d_offsets));
            PCC_TRY(offsets_to_host(ix, d_offsets, 1));
            PCC_HIP(hipStreamSynchronize(s));  // the window's one wait
            size_t off[2] = {0, 0};
            PCC_TRY(offsets_arrived(ix, 1, off));
            const size_t cnt = off[1];
            if (cnt && cnt < m)
                GROUND_LAUNCH(k_ground_compact, ground_blocks(cnt), order, cnt, xy, z, (const int32_t*)g->idx[cur].as<int32_t>(),
                              g->xy[cur ^ 1].as<float2>(), g->z[cur ^ 1].as<float>(), g->idx[cur ^ 1].as<int32_t>());
            if (cnt < m) cur ^= 1;  // (nobody left: the other side's m = 0 entries)
            m = cnt;
        }
        if (n_windows && pass_sizes && it < max_passes) pass_sizes[it] = m;
    }
    *ground = g->idx[cur].as<int32_t>();
    *n_ground = m;
    return PCC_OK;
}

int check_pmf(const PmfParams& p, float* windows, float* thresholds, size_t* n_windows) {
    if (const char* why = pmf_refusal(p)) { set_error("%s", why); return PCC_ERR_INVALID; }
    if (pmf_windows(p, PMF_MAX_WINDOWS, windows, thresholds, n_windows) != GROUND_PLAN_OK) {
        set_error("more than %d windows", PMF_MAX_WINDOWS);
        return PCC_ERR_OVERFLOW;
    }
    return PCC_OK;
}

}  // namespace
}  // namespace pcc

using namespace pcc;
extern "C" {
int pcc_pmf_windows(int max_window_size, float slope, float initial_distance, float max_distance, float cell_size, float base,
                    int exponential, size_t capacity, float* out_windows, float* out_thresholds, size_t* n_windows) {
    if (!n_windows || (capacity && (!out_windows || !out_thresholds))) { set_error("null output"); return PCC_ERR_INVALID; }
    const PmfParams p{max_window_size, slope, initial_distance, max_distance, cell_size, base, exponential};
    if (const char* why = pmf_refusal(p)) { set_error("%s", why); return PCC_ERR_INVALID; }
    if (pmf_windows(p, capacity, out_windows, out_thresholds, n_windows) != GROUND_PLAN_OK) {
        set_error("the window table is longer than the capacity %zu or than %d windows", capacity, PMF_MAX_WINDOWS);
        return PCC_ERR_OVERFLOW;
    }
    return PCC_OK;
}

int pcc_morphological_operator(pcc_index* ix, const void* pts, size_t n, size_t stride, int mem, float window, int op, float* out_z) {
    PCC_TRY(check_points(pts, n, stride, mem));
    if (n && !out_z) { set_error("null output"); return PCC_ERR_INVALID; }
    if (op != PCC_MORPH_DILATE && op != PCC_MORPH_ERODE && op != PCC_MORPH_OPEN && op != PCC_MORPH_CLOSE) {
        set_error("bad morphological operator %d", op);
        return PCC_ERR_INVALID;
    }
    if (!std::isfinite(window) || !(window > 0.f)) { set_error("window must be finite and positive"); return PCC_ERR_INVALID; }
    PCC_ENTER(ix);
    if (n == 0) { PCC_NOTHING_ENQUEUED(ix); return PCC_OK; }
    ev_next(ix);
    ev_mark(ix, EV_CALL0);
    GroundScratch* g = scratch<GroundScratch>(ix);
    const void* src = nullptr;
    PCC_TRY(ground_stage(ix, pts, n, stride, mem, &src));
    PCC_TRY(ground_load(ix, src, n, stride));
    Out<float> oz;
    PCC_TRY(oz.stage(out_z, n, mem, g->out_z));
    GroundPass P;
    PCC_TRY(ground_pass_setup(ix, g->xy[0].as<float2>(), g->z[0].as<float>(), n, window, &P));
    PCC_TRY(ground_operator(ix, P, g->z[0].as<float>(), n, op, oz.dev));
    ev_mark(ix, EV_CALL1);
    return finish(ix, mem, oz);
}

int pcc_progressive_morphological_filter(pcc_index* ix, const void* pts, size_t n, size_t stride, int mem, int max_window_size, float slope,
                                         float initial_distance, float max_distance, float cell_size, float base, int exponential,
                                         int32_t* out_ground, size_t* n_ground, size_t* out_pass_sizes, size_t max_passes) {
    PCC_TRY(check_points(pts, n, stride, mem));
    if ((n && !out_ground) || !n_ground) { set_error("null output"); return PCC_ERR_INVALID; }
    float windows[PMF_MAX_WINDOWS], thresholds[PMF_MAX_WINDOWS];
    size_t nw = 0;
    PCC_TRY(check_pmf(PmfParams{max_window_size, slope, initial_distance, max_distance, cell_size, base, exponential}, windows, thresholds,
                      &nw));
    PCC_ENTER(ix);
    *n_ground = 0;
    if (out_pass_sizes)
        for (size_t i = 0; i < std::min(nw, max_passes); ++i) out_pass_sizes[i] = 0;
    if (n == 0) { PCC_NOTHING_ENQUEUED(ix); return PCC_OK; }
    ev_next(ix);
    ev_mark(ix, EV_CALL0);
    const void* src = nullptr;
    PCC_TRY(ground_stage(ix, pts, n, stride, mem, &src));
    const int32_t* ground = nullptr;
    size_t ng = 0;
    PCC_TRY(pmf_run(ix, src, n, stride, windows, thresholds, nw, &ground, &ng, out_pass_sizes, max_passes));
    *n_ground = ng;
    ev_mark(ix, EV_CALL1);
    PCC_TRY(give(ix, mem, out_ground, ground, ng * sizeof(int32_t)));
    if (mem == PCC_MEM_HOST) PCC_HIP(hipStreamSynchronize(ix->stream));
    return PCC_OK;
}

int pcc_ground_segmentation(pcc_index* ix, const void* pts, size_t n, size_t stride, int mem, float leaf, int max_window_size, float slope,
                            float initial_distance, float max_distance, float cell_size, float base, int exponential, void* out_points,
                            size_t out_stride, size_t* n_filtered, int32_t* out_ground_index, size_t* n_ground, void* out_ground_points,
                            void* out_object_points) {
    // what pcc_voxel_grid refuses, with its messages
    PCC_TRY(check_points(pts, n, stride, mem));
    if (!out_points) { set_error("null output"); return PCC_ERR_INVALID; }
    if (out_stride < 12 || out_stride % 4) { set_error("bad output stride"); return PCC_ERR_INVALID; }
    if (!(leaf > 0.f)) { set_error("leaf size must be positive"); return PCC_ERR_INVALID; }
    if (!n_filtered || !n_ground) { set_error("null output"); return PCC_ERR_INVALID; }
    float windows[PMF_MAX_WINDOWS], thresholds[PMF_MAX_WINDOWS];
    size_t nw = 0;
    PCC_TRY(check_pmf(PmfParams{max_window_size, slope, initial_distance, max_distance, cell_size, base, exponential}, windows, thresholds,
                      &nw));
    PCC_ENTER(ix);
    *n_filtered = 0;
    *n_ground = 0;
    if (n == 0) { PCC_NOTHING_ENQUEUED(ix); return PCC_OK; }
    hipStream_t s = ix->stream;
    ev_next(ix);
    ev_mark(ix, EV_CALL0);
    GroundScratch* g = scratch<GroundScratch>(ix);

    // 1. the voxel grid into a zeroed buffer of this call's own (as pcc_region_growing_segmentation)
    const void* src = nullptr;
    PCC_TRY(ground_stage(ix, pts, n, stride, mem, &src));
    PCC_TRY(g->cloud.reserve(n * out_stride));
    PCC_HIP(hipMemsetAsync(g->cloud.p, 0, n * out_stride, s));
    size_t nv = 0;
    PCC_TRY(voxel_grid(ix, src, n, stride, PCC_MEM_DEVICE, leaf, 0, g->cloud.p, out_stride, &nv));
    *n_filtered = nv;
    if (nv == 0) return PCC_OK;  // (no finite point; voxel_grid has waited: nothing is in flight)

    // 2. the filter over the filtered cloud where it lies
    const int32_t* ground = nullptr;
    size_t ng = 0;
    PCC_TRY(pmf_run(ix, g->cloud.p, nv, out_stride, windows, thresholds, nw, &ground, &ng, nullptr, 0));
    *n_ground = ng;

    // 3. ExtractIndices, positive and negative: the stable partition by "object", ground in front, both ascending
    const unsigned int *order = nullptr, *d_offsets = nullptr;
    if (out_ground_points || out_object_points) {
        int32_t* label = g->keep.as<int32_t>();
        GROUND_LAUNCH(k_ground_mark, ground_blocks(nv), (const int32_t*)nullptr, nv, label);
        if (ng) GROUND_LAUNCH(k_ground_mark, ground_blocks(ng), ground, ng, label);
        PCC_TRY(extract_order(ix, label, nv, 2, &order, &d_offsets));
    }
    ev_mark(ix, EV_CALL1);
    PCC_TRY(give(ix, mem, out_points, g->cloud.p, nv * out_stride));
    PCC_TRY(give(ix, mem, out_ground_index, ground, ng * sizeof(int32_t)));
    if (order) {
        char* rec = nullptr;
        if (mem == PCC_MEM_HOST) {
            PCC_TRY(g->out_rec.reserve(nv * out_stride));
            rec = g->out_rec.as<char>();
        }
        void* dst_g = mem == PCC_MEM_HOST ? rec : out_ground_points;
        void* dst_o = mem == PCC_MEM_HOST ? rec + ng * out_stride : out_object_points;
        if (out_ground_points) PCC_TRY(launch_records(s, g->cloud.p, out_stride, order, ng, out_stride, dst_g, out_stride));
        if (out_object_points) PCC_TRY(launch_records(s, g->cloud.p, out_stride, order + ng, nv - ng, out_stride, dst_o, out_stride));
        if (mem == PCC_MEM_HOST) {
            PCC_TRY(give(ix, mem, out_ground_points, dst_g, ng * out_stride));
            PCC_TRY(give(ix, mem, out_object_points, dst_o, (nv - ng) * out_stride));
        }
    }
    if (mem == PCC_MEM_HOST) PCC_HIP(hipStreamSynchronize(s));
    return PCC_OK;
}
}  // extern "C"
