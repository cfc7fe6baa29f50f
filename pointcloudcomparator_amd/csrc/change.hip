// change.hip -- pcl::octree::OctreePointCloudChangeDetector on the GPU (gfx950): pcc_change_detection.
// replaces: spatial_change_detection (reference src/comparator.cpp:54-110, called from both verdict branches of main,
//   :1687-1698): add cloud A, switchBuffers(), add cloud B, getPointIndicesFromNewVoxels() -- the points of B in voxels
//   that hold no point of A.
//
// The lattice is change_plan.hpp's (fixed by the first finite point of A, else of B).  Passes, everything on the device:
//   k_chg_first   lowest index of a finite point of A and of B (block reduction, at most one atomicMin per block)
//   k_chg_anchor  the anchor a[3] from that point (one thread)
//   k_chg_bounds  min / max voxel coordinate per axis over both clouds as 64-bit integers (a thread converts the extremes of
//                 its points; wave, then block, then one atomic per block and bound); coordinates beyond 2^31 set the status word
//   k_chg_plan    the span verdict and the key origin (one thread)
//   k_chg_insert  A, then B, into an open-addressing table of 64-bit keys in HBM: atomicCAS claims a slot, a second word per
//                 slot holds "A is here" (bit 31) and the number of B points.  Lanes of a wave that hold the same key are
//                 merged first (a few rounds; what is left over inserts on its own), so a voxel of 20 000 points is not
//                 20 000 atomics on one word
//   k_chg_flags   every point of B finds its slot: flag = no A and enough B; launch_exclusive_scan; k_chg_compact moves the
//                 indices and, if asked for, whole records (4-byte words, 32 lanes per record)
// Every probe loop ends after `slots` steps at the latest and then sets CHG_PROBE (PCC_ERR_INTERNAL): no lane ever waits for
// another.  Which SLOT a key lands in depends on the order of arrival; membership, the A mark and the counts do not, and the
// output order comes from the scan -- so no result bit does.
#include <algorithm>
#include <cmath>

#include "entry.hpp"
#include "change_plan.hpp"

namespace pcc {

enum : unsigned int {
    CHG_RANGE = 1u,   // << axis: a voxel coordinate is not below 2^31 in magnitude
    CHG_SPAN = 8u,    // << axis: more than 2^21 voxels along the axis
    CHG_PROBE = 64u,  // a probe loop ran through the whole table
    CHG_NONE = 128u   // neither cloud has a finite point
};
constexpr unsigned int CHG_A_HERE = 0x80000000u;
constexpr int CHG_MERGE_ROUNDS = 8;

// the device words of one call; they travel to the host at its end (status and count; the bounds for a refusal's message)
struct ChangeDev {
    unsigned int status, count;
    unsigned int first[2];          // lowest index of a finite point of A, of B (~0u: none)
    unsigned long long lo[3], hi[3];  // min / max of (voxel coordinate + 2^31) over both clouds
    double a[3];                    // the anchor
    long long mn[3];                // lo - 2^31: the origin of the keys
};

struct ChangeScratch : Scratch {
    static constexpr ScratchSlot slot = SCRATCH_CHANGE;
    DevBuf a_raw, b_raw;            // the caller's clouds, staged (host memory)
    DevBuf keys, vals;              // the table: u64 key and u32 (A mark | B count) per slot
    DevBuf flags, scan_tmp;         // uint32[n_b + 1]: report flags, then their exclusive scan
    DevBuf out_index, out_records;  // results staged for a caller in host memory
    DevBuf dev;                     // ChangeDev
    HostBuf host;                   // its pinned copy
};

namespace {

__device__ __forceinline__ bool chg_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool chg_load(const char* __restrict__ pts, size_t stride, unsigned int i, float p[3]) {
    const float* f = reinterpret_cast<const float*>(pts + (size_t)i * stride);
    p[0] = f[0]; p[1] = f[1]; p[2] = f[2];
    return chg_finite(p[0]) && chg_finite(p[1]) && chg_finite(p[2]);
}

__global__ void k_chg_init(ChangeDev* __restrict__ d) {
    d->status = 0u; d->count = 0u;
    d->first[0] = d->first[1] = ~0u;
    for (int a = 0; a < 3; ++a) { d->lo[a] = ~0ull; d->hi[a] = 0ull; d->a[a] = 0.0; d->mn[a] = 0; }
}

// *first = the lowest index of a finite point.  A thread's indices ascend, so its first hit is its minimum; what the word
// already holds is a hint only (later workgroups find nothing below it and stop at once)
__global__ void __launch_bounds__(256)
k_chg_first(const char* __restrict__ pts, size_t stride, unsigned int n, unsigned int* __restrict__ first) {
    __shared__ unsigned int s_min[4];
    const unsigned int hint = __hip_atomic_load(first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned int best = ~0u;
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n && i < hint; i += gridDim.x * blockDim.x) {
        float p[3];
        if (chg_load(pts, stride, i, p)) { best = i; break; }
    }
    for (int m = 32; m >= 1; m >>= 1) best = min(best, (unsigned int)__shfl_xor((int)best, m, 64));
    if ((threadIdx.x & 63u) == 0u) s_min[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        best = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
        // (thousands of atomics on one word cost more than the reads: a workgroup that cannot lower the word any more stays away)
        if (best < __hip_atomic_load(first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(first, best);
    }
}

__global__ void k_chg_anchor(const char* __restrict__ a, size_t a_stride, const char* __restrict__ b, size_t b_stride, double res,
                             ChangeDev* __restrict__ d) {
    float p[3];
    if (d->first[0] != ~0u) (void)chg_load(a, a_stride, d->first[0], p);
    else if (d->first[1] != ~0u) (void)chg_load(b, b_stride, d->first[1], p);
    else { d->status = CHG_NONE; return; }
    for (int ax = 0; ax < 3; ++ax) d->a[ax] = change_anchor(p[ax], res);
}

// min / max voxel coordinate per axis.  floor(((double)x - a) / res) never decreases as x grows (IEEE subtraction and division by
// a positive number are monotone), so a thread keeps the float extremes of its points and converts those six values alone: the
// same integers as a conversion of every point, and the same range verdict (every quotient lies between the extremes')
__global__ void __launch_bounds__(256)
k_chg_bounds(const char* __restrict__ pts, size_t stride, unsigned int n, double res, ChangeDev* __restrict__ d) {
    __shared__ unsigned long long s_lo[4][3], s_hi[4][3];
    __shared__ unsigned int s_bad;
    if (d->status & CHG_NONE) return;
    if (threadIdx.x == 0) s_bad = 0u;
    float fl0 = INFINITY, fl1 = INFINITY, fl2 = INFINITY, fh0 = -INFINITY, fh1 = -INFINITY, fh2 = -INFINITY;
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float p[3];
        if (!chg_load(pts, stride, i, p)) continue;
        fl0 = fminf(fl0, p[0]); fh0 = fmaxf(fh0, p[0]);
        fl1 = fminf(fl1, p[1]); fh1 = fmaxf(fh1, p[1]);
        fl2 = fminf(fl2, p[2]); fh2 = fmaxf(fh2, p[2]);
    }
    unsigned long long lo0 = ~0ull, lo1 = ~0ull, lo2 = ~0ull, hi0 = 0ull, hi1 = 0ull, hi2 = 0ull;
    unsigned int bad = 0u;
    if (fl0 <= fh0) {  // (this thread has seen a finite point)
        const double a0 = d->a[0], a1 = d->a[1], a2 = d->a[2];
        int64_t k;
        if (change_coord(fl0, a0, res, &k)) lo0 = (unsigned long long)(k + 2147483648ll); else bad |= CHG_RANGE;
        if (change_coord(fh0, a0, res, &k)) hi0 = (unsigned long long)(k + 2147483648ll); else bad |= CHG_RANGE;
        if (change_coord(fl1, a1, res, &k)) lo1 = (unsigned long long)(k + 2147483648ll); else bad |= CHG_RANGE << 1;
        if (change_coord(fh1, a1, res, &k)) hi1 = (unsigned long long)(k + 2147483648ll); else bad |= CHG_RANGE << 1;
        if (change_coord(fl2, a2, res, &k)) lo2 = (unsigned long long)(k + 2147483648ll); else bad |= CHG_RANGE << 2;
        if (change_coord(fh2, a2, res, &k)) hi2 = (unsigned long long)(k + 2147483648ll); else bad |= CHG_RANGE << 2;
    }
    for (int m = 32; m >= 1; m >>= 1) {
        lo0 = min(lo0, (unsigned long long)__shfl_xor(lo0, m, 64)); hi0 = max(hi0, (unsigned long long)__shfl_xor(hi0, m, 64));
        lo1 = min(lo1, (unsigned long long)__shfl_xor(lo1, m, 64)); hi1 = max(hi1, (unsigned long long)__shfl_xor(hi1, m, 64));
        lo2 = min(lo2, (unsigned long long)__shfl_xor(lo2, m, 64)); hi2 = max(hi2, (unsigned long long)__shfl_xor(hi2, m, 64));
    }
    const unsigned int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) {
        s_lo[w][0] = lo0; s_lo[w][1] = lo1; s_lo[w][2] = lo2;
        s_hi[w][0] = hi0; s_hi[w][1] = hi1; s_hi[w][2] = hi2;
    }
    __syncthreads();
    if (bad) atomicOr(&s_bad, bad);
    __syncthreads();
    if (threadIdx.x < 3) {
        const unsigned int ax = threadIdx.x;
        const unsigned long long lo = min(min(s_lo[0][ax], s_lo[1][ax]), min(s_lo[2][ax], s_lo[3][ax]));
        const unsigned long long hi = max(max(s_hi[0][ax], s_hi[1][ax]), max(s_hi[2][ax], s_hi[3][ax]));
        if (lo <= hi) { atomicMin(&d->lo[ax], lo); atomicMax(&d->hi[ax], hi); }
    }
    if (threadIdx.x == 0 && s_bad) atomicOr(&d->status, s_bad);
}

__global__ void k_chg_plan(ChangeDev* __restrict__ d) {
    if (d->status & CHG_NONE) return;
    unsigned int st = 0u;
    for (int ax = 0; ax < 3; ++ax) {
        if (d->lo[ax] > d->hi[ax]) continue;  // (every point out of range along this axis: CHG_RANGE is set)
        const long long mn = (long long)d->lo[ax] - 2147483648ll, mx = (long long)d->hi[ax] - 2147483648ll;
        d->mn[ax] = mn;
        if (!change_span_ok(mn, mx)) st |= CHG_SPAN << ax;
    }
    if (st) d->status |= st;
}

// the key of a finite point of a call whose status is clean (every coordinate is in range then)
__device__ __forceinline__ unsigned long long chg_key(const float p[3], const double a[3], double res, const int64_t mn[3]) {
    int64_t k[3] = {0, 0, 0};
    (void)change_coord(p[0], a[0], res, &k[0]);
    (void)change_coord(p[1], a[1], res, &k[1]);
    (void)change_coord(p[2], a[2], res, &k[2]);
    return change_key(k, mn);
}

// cloud A (is_b == 0) marks its voxels, cloud B counts its points per voxel
__global__ void __launch_bounds__(256)
k_chg_insert(const char* __restrict__ pts, size_t stride, unsigned int n, double res, ChangeDev* __restrict__ d,
             unsigned long long* __restrict__ keys, unsigned int* __restrict__ vals, unsigned long long slots, int is_b) {
    if (d->status) return;
    const double a[3] = {d->a[0], d->a[1], d->a[2]};
    const int64_t mn[3] = {d->mn[0], d->mn[1], d->mn[2]};
    const unsigned int lane = threadIdx.x & 63u;
    // (the trip count is the workgroup's: every lane of a wave reaches the exchanges below)
    for (unsigned int base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {
        const unsigned int i = base + threadIdx.x;
        float p[3];
        const bool valid = i < n && chg_load(pts, stride, i, p);
        const unsigned long long key = valid ? chg_key(p, a, res, mn) : CHANGE_EMPTY_KEY;
        // lanes with one key: the lowest of them inserts for all.  Bounded: what CHG_MERGE_ROUNDS rounds leave inserts alone
        unsigned int add = valid ? 1u : 0u;
        unsigned long long todo = __ballot(valid);
        for (int r = 0; r < CHG_MERGE_ROUNDS && todo; ++r) {
            const int src = __ffsll((unsigned long long)todo) - 1;
            const unsigned long long k0 = __shfl(key, src, 64);
            const unsigned long long same = __ballot(valid && key == k0) & todo;
            if ((int)lane == src) add = (unsigned int)__popcll(same);
            else if ((same >> lane) & 1ull) add = 0u;
            todo &= ~same;
        }
        if (!add) continue;
        unsigned long long s = change_hash(key, slots);
        bool placed = false;
        for (unsigned long long t = 0; t < slots; ++t) {
            unsigned long long cur = keys[s];  // (a key, once written, stays: a plain read that shows it is final)
            if (cur != key) cur = cur == CHANGE_EMPTY_KEY ? atomicCAS(&keys[s], CHANGE_EMPTY_KEY, key) : cur;
            if (cur == key || cur == CHANGE_EMPTY_KEY) { placed = true; break; }
            s = (s + 1) & (slots - 1);
        }
        if (!placed) { atomicOr(&d->status, CHG_PROBE); continue; }
        if (is_b) atomicAdd(&vals[s], add);
        else if (!(vals[s] & CHG_A_HERE)) atomicOr(&vals[s], CHG_A_HERE);  // (the mark, once set, stays as well)
    }
}

// flags[i] = 1 for the points of B to report, flags[n] = 0 (after the exclusive scan: their number)
__global__ void __launch_bounds__(256)
k_chg_flags(const char* __restrict__ pts, size_t stride, unsigned int n, double res, ChangeDev* __restrict__ d,
            const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ vals, unsigned long long slots,
            unsigned int min_points, unsigned int* __restrict__ flags) {
    const bool clean = d->status == 0u;
    const double a[3] = {d->a[0], d->a[1], d->a[2]};
    const int64_t mn[3] = {d->mn[0], d->mn[1], d->mn[2]};
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += gridDim.x * blockDim.x) {
        unsigned int f = 0u;
        float p[3];
        if (clean && i < n && chg_load(pts, stride, i, p)) {
            const unsigned long long key = chg_key(p, a, res, mn);
            unsigned long long s = change_hash(key, slots);
            bool found = false;
            for (unsigned long long t = 0; t < slots; ++t) {
                const unsigned long long cur = keys[s];
                if (cur == key) { found = true; break; }
                if (cur == CHANGE_EMPTY_KEY) break;
                s = (s + 1) & (slots - 1);
            }
            if (!found) atomicOr(&d->status, CHG_PROBE);  // (every finite point of B was inserted)
            else {
                const unsigned int v = vals[s];
                f = (!(v & CHG_A_HERE) && (v & ~CHG_A_HERE) >= min_points) ? 1u : 0u;
            }
        }
        flags[i] = f;
    }
}

// pos = the exclusive scan of the flags (pos[n] = their number): index i of B goes to slot pos[i], its record with it.
// LANES lanes per point: 32 move a record's 4-byte words, 1 when only indices are asked for
template <int LANES>
__global__ void __launch_bounds__(256)
k_chg_compact(const char* __restrict__ pts, size_t stride, const unsigned int* __restrict__ pos, unsigned int n,
              int32_t* __restrict__ out_index, char* __restrict__ out_records, ChangeDev* __restrict__ d) {
    if (blockIdx.x == 0 && threadIdx.x == 0) d->count = pos[n];
    const unsigned int l = threadIdx.x % LANES;
    const unsigned int ngroups = (gridDim.x * blockDim.x) / LANES;
    const unsigned int words = (unsigned int)(stride / 4);
    for (unsigned int i = (blockIdx.x * blockDim.x + threadIdx.x) / LANES; i < n; i += ngroups) {
        const unsigned int at = pos[i];
        if (pos[i + 1] == at) continue;
        if (l == 0) out_index[at] = (int32_t)i;
        if (LANES > 1) {
            const unsigned int* src = reinterpret_cast<const unsigned int*>(pts + (size_t)i * stride);
            unsigned int* dst = reinterpret_cast<unsigned int*>(out_records + (size_t)at * stride);
            for (unsigned int w = l; w < words; w += LANES) dst[w] = src[w];
        }
    }
}

unsigned int chg_blocks(size_t n, size_t per_block, unsigned int cap) {
    return (unsigned int)std::max<size_t>(1, std::min<size_t>((n + per_block - 1) / per_block, cap));
}

}  // namespace

// behind the argument checks: n_a, n_b in [1, 2^31)
static int change_detection(pcc_index* ix, const void* a, size_t n_a, size_t a_stride, const void* b, size_t n_b, size_t b_stride, int mem,
                            double res, int min_points, int32_t* out_index, void* out_records, size_t* n_out) {
    hipStream_t s = ix->stream;
    ChangeScratch* c = scratch<ChangeScratch>(ix);
    // a strided host view may end with its last row's x, y, z; records travel whole
    const char *da = nullptr, *db = nullptr;
    PCC_TRY(stage_in(ix, static_cast<const char*>(a), (n_a - 1) * a_stride + 12, mem, c->a_raw, &da));
    PCC_TRY(stage_in(ix, static_cast<const char*>(b), out_records ? n_b * b_stride : (n_b - 1) * b_stride + 12, mem, c->b_raw, &db));
    Out<int32_t> oi;
    Out<char> orec;
    PCC_TRY(oi.stage(out_index, n_b, mem, c->out_index));
    PCC_TRY(orec.stage(static_cast<char*>(out_records), out_records ? n_b * b_stride : 0, mem, c->out_records));
    const unsigned long long slots = change_table_slots((uint64_t)n_a + n_b);
    PCC_TRY(c->keys.reserve(slots * sizeof(unsigned long long)));
    PCC_TRY(c->vals.reserve(slots * sizeof(unsigned int)));
    PCC_TRY(c->flags.reserve((n_b + 1) * sizeof(unsigned int)));
    PCC_TRY(c->dev.reserve(sizeof(ChangeDev)));
    PCC_TRY(c->host.reserve(sizeof(ChangeDev)));
    ChangeDev* d = c->dev.as<ChangeDev>();
    unsigned long long* keys = c->keys.as<unsigned long long>();
    unsigned int *vals = c->vals.as<unsigned int>(), *flags = c->flags.as<unsigned int>();
    const unsigned int ua = (unsigned int)n_a, ub = (unsigned int)n_b;
    const unsigned int ga = chg_blocks(n_a, 256, 4096), gb = chg_blocks(n_b, 256, 4096);
    // the table is cleared at the start of every call
    PCC_HIP(hipMemsetAsync(keys, 0xff, slots * sizeof(unsigned long long), s));
    PCC_HIP(hipMemsetAsync(vals, 0, slots * sizeof(unsigned int), s));
    hipLaunchKernelGGL(k_chg_init, dim3(1), dim3(1), 0, s, d);
    hipLaunchKernelGGL(k_chg_first, dim3(std::min(ga, 1024u)), dim3(256), 0, s, da, a_stride, ua, &d->first[0]);
    hipLaunchKernelGGL(k_chg_first, dim3(std::min(gb, 1024u)), dim3(256), 0, s, db, b_stride, ub, &d->first[1]);
    hipLaunchKernelGGL(k_chg_anchor, dim3(1), dim3(1), 0, s, da, a_stride, db, b_stride, res, d);
    hipLaunchKernelGGL(k_chg_bounds, dim3(ga), dim3(256), 0, s, da, a_stride, ua, res, d);
    hipLaunchKernelGGL(k_chg_bounds, dim3(gb), dim3(256), 0, s, db, b_stride, ub, res, d);
    hipLaunchKernelGGL(k_chg_plan, dim3(1), dim3(1), 0, s, d);
    hipLaunchKernelGGL(k_chg_insert, dim3(ga), dim3(256), 0, s, da, a_stride, ua, res, d, keys, vals, slots, 0);
    hipLaunchKernelGGL(k_chg_insert, dim3(gb), dim3(256), 0, s, db, b_stride, ub, res, d, keys, vals, slots, 1);
    hipLaunchKernelGGL(k_chg_flags, dim3(chg_blocks(n_b + 1, 256, 4096)), dim3(256), 0, s, db, b_stride, ub, res, d, keys, vals, slots,
                       (unsigned int)min_points, flags);
    PCC_HIP(hipGetLastError());
    PCC_TRY(launch_exclusive_scan(ix, s, flags, n_b + 1, c->scan_tmp));
    // (4096 workgroups: with 2^17 of them, a few points a group, the 10M pass took 268 instead of 239 us)
    if (out_records) hipLaunchKernelGGL(k_chg_compact<32>, dim3(chg_blocks(n_b, 8, 4096)), dim3(256), 0, s, db, b_stride, flags, ub, oi.dev, orec.dev, d);
    else hipLaunchKernelGGL(k_chg_compact<1>, dim3(gb), dim3(256), 0, s, db, b_stride, flags, ub, oi.dev, (char*)nullptr, d);
    PCC_HIP(hipGetLastError());
    // the call's one read-back: status word and count (the bounds travel with them for the refusal's message)
    PCC_HIP(hipMemcpyAsync(c->host.p, d, sizeof(ChangeDev), hipMemcpyDeviceToHost, s));
    PCC_HIP(hipStreamSynchronize(s));
    const ChangeDev h = *c->host.as<ChangeDev>();
    if (h.status & CHG_PROBE) { set_error("change detection: a probe ran through all %llu slots of the voxel table", slots); return PCC_ERR_INTERNAL; }
    for (int ax = 0; ax < 3; ++ax) {
        if (h.status & (CHG_RANGE << ax)) {
            set_error("resolution %g too small for these clouds: a voxel coordinate along %c is beyond 2^31, the span beyond the 2^21 voxels an axis may take",
                      res, "xyz"[ax]);
            return PCC_ERR_UNSUPPORTED;
        }
    }
    for (int ax = 0; ax < 3; ++ax) {
        if (h.status & (CHG_SPAN << ax)) {
            set_error("resolution %g too small for these clouds: they span %llu voxels along %c (limit 2^21 = %llu)", res,
                      (unsigned long long)(h.hi[ax] - h.lo[ax] + 1), "xyz"[ax], (unsigned long long)CHANGE_MAX_SPAN);
            return PCC_ERR_UNSUPPORTED;
        }
    }
    *n_out = h.count;  // (CHG_NONE: no finite point anywhere, nothing reported)
    oi.count = h.count;
    orec.count = (size_t)h.count * b_stride;
    return finish(ix, mem, oi, orec);
}

}  // namespace pcc

using namespace pcc;
extern "C" {
int pcc_change_detection(pcc_index* ix, const void* a, size_t n_a, size_t a_stride, const void* b, size_t n_b, size_t b_stride, int mem,
                         double resolution, int min_points_per_leaf, int32_t* out_index, void* out_records, size_t* n_out) {
    // the arguments first: host arithmetic, refused before any device is looked at
    if (!a || !b || !out_index || !n_out) { set_error("null argument"); return PCC_ERR_INVALID; }
    PCC_TRY(check_mem(mem));
    if (n_a == 0 || n_b == 0) { set_error("empty input cloud"); return PCC_ERR_EMPTY; }
    PCC_TRY(check_points(a, n_a, a_stride, mem));
    PCC_TRY(check_points(b, n_b, b_stride, mem));
    if (reinterpret_cast<uintptr_t>(a) % 4 || reinterpret_cast<uintptr_t>(b) % 4 || reinterpret_cast<uintptr_t>(out_index) % 4 ||
        reinterpret_cast<uintptr_t>(out_records) % 4) {
        set_error("points, indices and records must be 4-byte aligned");
        return PCC_ERR_INVALID;
    }
    if (!(resolution > 0) || !std::isfinite(resolution)) { set_error("resolution must be positive and finite"); return PCC_ERR_INVALID; }
    if (min_points_per_leaf < 0) { set_error("min_points_per_leaf must not be negative"); return PCC_ERR_INVALID; }
    PCC_ENTER(ix);
    *n_out = 0;
    return change_detection(ix, a, n_a, a_stride, b, n_b, b_stride, mem, resolution, min_points_per_leaf, out_index, out_records, n_out);
}
}  // extern "C"
