// pcc_internal.hpp -- shared declarations of libpcc_nn (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include "pcc_nn.h"
#include "flann_tree.hpp"
#include "cloud_batch.hpp"

// every PCC_SEED_STRIDE-th reference is a "seed": the exhaustive scan of the seeds bounds a far query's ball
#define PCC_SEED_SHIFT 6
#define PCC_SEED_STRIDE (1 << PCC_SEED_SHIFT)
// sharded device counters (pcc::DevWords): shard s owns words [s * PCC_OPEN_CTR_STRIDE ...], one 128-byte line each
#define PCC_OPEN_SHARDS 64
#define PCC_OPEN_CTR_STRIDE 32
#define PCC_TIE_SHARDS 16
#define FLANN_DEV_STACK_MAX 256  // deepest tree k_tie_walk takes (20 bytes of scratch per level and lane)

namespace pcc {

// ---- error plumbing --------------------------------------------------------
void set_error(const char* fmt, ...);
#define PCC_HIP(expr)                                                            \
    do {                                                                         \
        hipError_t _e = (expr);                                                  \
        if (_e != hipSuccess) {                                                  \
            pcc::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                           __FILE__, __LINE__);                                  \
            return PCC_ERR_DEVICE;                                               \
        }                                                                        \
    } while (0)
#define PCC_TRY(expr)                 \
    do {                              \
        int _s = (expr);              \
        if (_s != PCC_OK) return _s;  \
    } while (0)

// ---- device buffer that only grows ------------------------------------------
// DevBuf and HostBuf OWN their memory: the destructor frees, a move hands the block over and leaves the source
// empty, nothing copies.  Whatever holds one -- the handle, a feature's scratch -- needs no cleanup code of its own.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    int reserve(size_t bytes);  // returns pcc_status
    // room for `want` bytes with the first `keep` bytes kept (reserve() keeps nothing): grows to max(want, 2 * cap), copies on `s`
    // and waits for it.  A failure on the way frees the new block and leaves this one as it was.
    int grow_keep(hipStream_t s, size_t keep, size_t want);
    void release();
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// grow-only pinned host buffer (read-backs that the host then walks: SOR mean distances, ...); owns its memory as DevBuf does
struct HostBuf {
    void* p = nullptr;
    size_t cap = 0;
    HostBuf() = default;
    HostBuf(const HostBuf&) = delete;
    HostBuf& operator=(const HostBuf&) = delete;
    HostBuf(HostBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    HostBuf& operator=(HostBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~HostBuf() { release(); }
    int reserve(size_t bytes);
    void release();
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};
static_assert(!std::is_copy_constructible<DevBuf>::value && std::is_nothrow_move_constructible<DevBuf>::value, "DevBuf owns its memory");
static_assert(!std::is_copy_constructible<HostBuf>::value && std::is_nothrow_move_constructible<HostBuf>::value, "HostBuf owns its memory");

// selects `dev` for the scope and restores the caller's device at its end; ok = false when the device could not be selected
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; }
        if (prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
    }
    ~DeviceGuard() {
        int cur;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// Uniform-grid parameters (device + host copy).  Cell of a point along GRID axis a (0: the cells of a row, fastest in the
// linear id (c2 * dim1 + c1) * dim0 + c0; 1: the rows of a layer; 2: the layers):
//   c_a = clamp(int((p[ax_a] - org_a) * inv_h), 0, dim_a - 1)
// The same expression (same rounding) is used at build and query time.  ax[] names the coordinate of the cloud (0 x, 1 y, 2 z)
// each grid axis follows: k_grid_params puts the cloud's SHORTEST extent on axis 1 and the longest on axis 2, so that the rows
// above / below and the layers before / behind a query's row lie as close to it in memory as the cloud allows.
struct GridParams {
    float org[3];  // grid axes
    float h;
    float inv_h;
    int dim[3];    // grid axes
    int ncells;
    int ax[3];     // grid axis -> coordinate of the cloud
};


// The rule behind GridParams::ax (one place: k_grid_params on the device, the clustering grid on the host): the coordinate
// with the second shortest extent runs along the rows, the shortest over the rows of a layer, the longest over the layers;
// ties keep x, y, z order.  forced 0..5 = xyz, xzy, yxz, yzx, zxy, zyx (PCC_OPT_GRID_AXES), anything else: by extent.
// GRID_AXES_MIN_POINTS: clouds below it would keep x, y, z.  Measured on ONE handle (same memory for every setting, tools/exp_ab.py,
// exp_knn_ab.py): for k = 1 the layout by extent costs 3-5 % of a step at 1M-1.4M points (C2 0.2263 -> 0.2327 ms, room scan 0.3601 ->
// 0.3787), gains 1.4-3 % at 4M and is time-neutral at 10M (1.3333 / 1.3334 ms), where it takes a sixth of the search's fabric traffic away;
// for k-NN at 1M it is worth 7 % at K = 51 and 17 % at K = 100 on the corridor scene (1.229 -> 1.143, 2.196 -> 1.814 ms: the ball boxes of the
// bound path span rows of several layers) and nothing on the room scan.  A cloud of the reference's sizes spends 5-20x longer in its k-NN
// consumers (SOR, normals, region growing) than in a k = 1 step: 0 -- by extent at every size.
constexpr unsigned int GRID_AXES_MIN_POINTS = 0u;
__host__ __device__ inline void grid_axes_for(const float ext[3], int forced, int ax[3]) {
    // (no array is indexed by a variable: on the device that would put it in scratch memory)
    const float e0 = ext[0], e1 = ext[1], e2 = ext[2];
    // rank of each coordinate by ascending extent, ties in x, y, z order (a stable sort of three)
    const int r0 = (e1 < e0 ? 1 : 0) + (e2 < e0 ? 1 : 0);
    const int r1 = (e0 <= e1 ? 1 : 0) + (e2 < e1 ? 1 : 0);
    const int r2 = (e0 <= e2 ? 1 : 0) + (e1 <= e2 ? 1 : 0);
    const int shortest = r0 == 0 ? 0 : (r1 == 0 ? 1 : 2), second = r0 == 1 ? 0 : (r1 == 1 ? 1 : 2), longest = r0 == 2 ? 0 : (r1 == 2 ? 1 : 2);
    (void)r2;
    ax[0] = second; ax[1] = shortest; ax[2] = longest;
    if (forced >= 0 && forced < 6) {
        ax[0] = forced >> 1;                          // 0 0 1 1 2 2
        const int o0 = ax[0] == 0 ? 1 : 0, o1 = ax[0] == 2 ? 1 : 2;  // the other two, ascending
        ax[1] = (forced & 1) ? o1 : o0;
        ax[2] = (forced & 1) ? o0 : o1;
    }
}
// element `i` of a three-vector without indexing memory by a variable
template <class T>
__host__ __device__ inline T pick3(const T v[3], int i) { return i == 0 ? v[0] : (i == 1 ? v[1] : v[2]); }

// Device-resident description of the grid, written by k_grid_params from the pack kernel's
// per-workgroup statistics.  The host never waits for it on the build path: launches are sized
// from upper bounds it knows (n, nc_cap) and kernels read the actual values from here.
struct GridDev {
    GridParams g;
    float slack;            // absolute slack of the outside-of-cube bound (cell-boundary rounding)
    unsigned int n_valid;   // finite points (PCL total_nr_points_)
    unsigned int n_invalid;
    float lo[3], hi[3];     // bounding box of the valid points (x, y, z: what the handle reports)
    float glo[3], ghi[3];   // the same box along the grid's axes (ball_box, k_grid_far)
    unsigned int voxel;     // 1: cells are PCL VoxelGrid voxels -- id from floor(v*inv_h) - org (org = float(min_b))
};

// Tuning knobs of one handle (pcc_index_set_option).  The PCC_* environment variables only supply the defaults a new
// handle starts with; nothing in the library reads the environment after that.
struct Options {
    double grid_ppc = 0.75;         // PCC_OPT_GRID_PPC: mean references per cell the grid aims for (0.5 was the optimum of the lane-per-query
                                    // kernel; with the flat kernels 0.7-1.0 is a plateau for volumetric scenes, surface scans of 10M points
                                    // prefer 0.25-0.5, those of the reference's sizes 1.0: DESIGN.md 5)
    int grid_trim = 3;              // PCC_OPT_GRID_TRIM: k of the trimmed bounding box (0: plain bounding box)
    int far_mode = -1;              // PCC_OPT_FAR_MODE: -1 auto, 0 exhaustive fallback only, 1 always seed scan + ball walk
    int icp_sorted = 1;             // PCC_OPT_ICP_SORTED: pcc_icp_align keeps its source cloud in the target grid's cell order (one gather, then
                                    // every pass reads queries and writes keys front to back); 0 = caller's order, gathered / scattered per pass
    int icp_warm = 1;               // PCC_OPT_ICP_WARM: ICP passes start from the previous pass's neighbours
    int icp_device_loop = 1;        // PCC_OPT_ICP_DEVICE_LOOP: 0 = the host-driven loop (same bits)
    int ec_cells = 3;               // PCC_OPT_EC_CELLS: clustering on the clique-cell grid: 3 union-find over CELLS (round 5), 1 / 2 over points
                                    // (lanes over neighbour cells / over points); 0: per-point ball scan on the search grid
    double sort_mp_min = 1.8e6;     // PCC_OPT_SORT_MP_MIN: references from which the three-level sort is used (round 5, build us two-level /
                                    // three-level: 1M 89 / 124, 1.5M 122 / 135, 2M 155 / 149)
    double sort_mp_min_q = 2.5e6;   // PCC_OPT_SORT_MP_MIN_Q: the same for query clouds (5M until round 5: with the cells from the pack kernel and the
                                    // larger level-3 stage the three-level form wins from ~2.5M on -- 3M 117 -> 88 us, 4M 131 -> 98 us, 2M 75 = 77)
    int nn1_kernel = 1;             // PCC_OPT_NN1_KERNEL: 0 one lane per query; 1 rows drained flat, lanes over candidates (2 / 3: open lanes listed / in place)
    int knn_cache_k = 0;            // PCC_OPT_KNN_CACHE_K: self k-NN rows searched with at least this K and kept (0: off)
    int knn_kernel = 1;             // PCC_OPT_KNN_KERNEL: 1 selection kernel for k <= 128, 0 merge network only
    int nn1_dense_min = 4;          // PCC_OPT_NN1_DENSE_MIN: references per own cell from which a wave starts with the own cell alone
    int sort_stage1 = 1;            // PCC_OPT_SORT_STAGE1: level 1 of the three-level sort writes bucket-sorted LDS tiles (1: reference points; 2: query pairs too; 0: one store per point)
    int nn1_open_flat = 1;          // PCC_OPT_NN1_OPEN_FLAT: the listed open lanes drained flat (k_nn1_open_flat); 0 = one lane per query
    int flann_split = 0;            // PCC_OPT_FLANN_SPLIT: 0 middleSplit_, 1 middleSplit (which rule FLANN's divideTree is replayed with)
    int grid_axes = -1;             // PCC_OPT_GRID_AXES: which coordinate the grid's axes (row, rows of a layer, layers) follow: -1 by extent (second
                                    // shortest, shortest, longest; clouds below GRID_AXES_MIN_POINTS -- 0 -- would keep xyz); -2 by extent whatever that says;
                                    // 0 xyz (the layout of rounds 1-5), 1 xzy, 2 yxz, 3 yzx, 4 zxy, 5 zyx
    int knn_run = 16;               // PCC_OPT_KNN_RUN: k-NN selection kernel: consecutive cell-sorted queries a wave takes in a row, every one after the
                                    // first starting from its predecessor's K-th distance + their separation (knn.hip); 1 = every query on its own.
                                    // One handle, 1M self query, runs of 4 / 8 / 16 / 32, ms: corridor K = 51 1.167 / 1.146 / 1.119 / 1.215, K = 100
                                    // 1.910 / 1.816 / 1.775 / 2.013; room scan K = 51 0.976 / 0.971 / 0.946 / 0.991, K = 100 1.210 / 1.179 / 1.148 / 1.212
    int scan_chained = 1;           // PCC_OPT_SCAN_CHAINED: exclusive scans of up to 512 x 2048 counters in ONE launch (workgroups pass their totals on as
                                    // tagged 64-bit atomics and wait for the workgroups in front of them: relies on in-order dispatch); 0 = the two-launch
                                    // form (block totals, then apply), which waits for nothing
    int rift_layout = 1;            // PCC_OPT_RIFT_LAYOUT: RIFT histogram kernel, 1 = 32 lanes per row (votes by all lanes, bins by owner lanes), 0 = one lane per row
    int fpfh_layout = 1;            // PCC_OPT_FPFH_LAYOUT: FPFH kernels (SPFH and weighting), 1 = a wave per row (pair features by all lanes, bins by owner
                                    // lanes), 0 = one lane per row
    int sift_layout = 1;            // PCC_OPT_SIFT_LAYOUT: SIFT scale-space kernel, 1 = a wave per point (weights by all lanes, sums by one owner lane per
                                    // scale), 0 = one lane per (point, scale)
    int host_pipe = 1;              // PCC_OPT_HOST_PIPE: clouds / results of 8 MB and more in pageable HOST memory cross PCIe through the library's own pinned
                                    // chunk buffers, staged by a few host threads (x, y, z only when the stride is 24 bytes or more); 0 = one
                                    // hipMemcpyAsync of the raw array (rounds 1-5)
    int fuse_params = 0;            // PCC_OPT_FUSE_PARAMS (bits): 1 = the grid parameters come out of the build's pack kernel (its last workgroup to finish)
                                    // instead of k_grid_params -- built in round 6 and a LOSS: the hand-over needs an agent-scope release fence in every
                                    // workgroup, which on this chip writes the XCD's L2 back, in a kernel that has just dirtied 160 MB of it: build
                                    // 0.437 -> 0.497 ms at C3, 0.089 -> 0.112 at C2 (EXPERIMENTS.md); 2 = a pass of pcc_icp_align is solved by the last
                                    // workgroup of k_icp_sums (a kernel that writes 65 KB) instead of k_icp_solve
    int xcd_run = 256;              // PCC_OPT_XCD_RUN: consecutive workgroups of the k = 1 search steered to the same XCD (its L2).  32 until round 5;
                                    // with the layers of the grid a few rows apart (grid_axes) a run should hold several LAYERS, so that the rows of
                                    // the layer behind are re-read from the same L2: C3 fabric traffic of the search 2.95 -> 2.42 GB per call.  Time,
                                    // on one handle: C3 step 1.3517 (by extent, 32) -> 1.3334 (by extent, 256); x / y / z layout 1.3333 / 1.3316
    int rift_batch_brute_max = 8192;   // PCC_OPT_RIFT_BATCH_BRUTE_MAX: clouds of a pcc_rift_descriptors_batch call up to this many points get their radius
                                    // rows from the exhaustive builder over the whole batch (rift_batch.hip); larger ones take the single path, one by
                                    // one, on a work handle.  Measured (EXPERIMENTS.md, "Batched RIFT descriptors"): a cloud alone is cheaper there from ~4500 points, beside others from ~11 000
    int sift_batch_brute_max = 8192;   // PCC_OPT_SIFT_BATCH_BRUTE_MAX: clouds of a pcc_sift_keypoints_batch call up to this many points go through the
                                    // batch kernels (sift_batch.hip: segmented voxel grid, exhaustive rows and 25-NN over the whole batch); larger
                                    // ones take the single path, one by one, on a work handle.  Measured (EXPERIMENTS.md, "Batched SIFT keypoints"): a
                                    // cloud alone is cheaper there from ~3000 points, beside others not before the 8000 measured
    int rgb_batch_brute_max = 8192;    // PCC_OPT_RGB_BATCH_BRUTE_MAX: clouds of a pcc_region_growing_rgb_batch call up to this many points get their
                                    // k-NN rows from the exhaustive segmented kernel over the whole batch (region_rgb_batch.hip); larger ones take
                                    // the single path, one by one, on a work handle.  Measured (EXPERIMENTS.md, "Batched colour region growing"):
                                    // beside others the batch kernels win at every size measured (up to 8000 points); a cloud alone ties from 8192 on
    int fpfh_batch_brute_max = 8192;   // PCC_OPT_FPFH_BATCH_BRUTE_MAX: clusters of a pcc_fpfh_descriptors_batch call up to this many points get their
                                    // radius rows from the exhaustive builder over the whole batch (fpfh_batch.hip); larger ones take the single
                                    // path, one by one, on a work handle.  Measured (EXPERIMENTS.md, "Batched FPFH descriptors"; device memory):
                                    // 60 clusters of 20 ... 5000 points take 4.02 / 2.24 / 1.49 / 1.49 ms at 2048 / 4096 / 8192 / 16 384; a cluster alone is cheaper on the work
                                    // handle somewhere between 8192 points (0.46 against 0.48 ms) and 16 384 (0.85 against 0.69 ms): only 2048,
                                    // 4096, 8192 and 16 384 were measured
    int vfh_batch_brute_max = 8192;    // PCC_OPT_VFH_BATCH_BRUTE_MAX: clusters of a pcc_vfh_descriptors_batch call of 2 .. this many points go through
                                    // the batch kernels (vfh_batch.hip: exhaustive rows, one chain wave per cluster, votes and bins over the whole
                                    // batch); larger ones take the single call, one by one, on a work handle.  Measured (EXPERIMENTS.md,
                                    // "Batched VFH descriptors"; device memory): 60 clusters of 20 ... 5000 points take 2.12 / 0.98 / 0.45 / 0.45 ms at
                                    // 2048 / 4096 / 8192 / 16 384; a cluster alone is cheaper on the work handle from 8192 points (0.30 against 0.33 ms)
    int overlap_prep = 1;           // PCC_OPT_OVERLAP_PREP: a k = 1 search that follows setInputCloud directly packs and sorts its queries on a
                                    // second stream while the build's cell sort is still running (they share nothing but the grid parameters);
                                    // from 2M queries on, 2 = at every size
    void from_env();
};

// SOR statistics on the device (pack.hip): exact == 0 -> the tree sums may differ from PCL's in-order sums
struct SorStats {
    double sum, sq, thr;
    unsigned long long kept;
    unsigned int exact, pad;
};

// The handle's device words (pcc_index::words(), zeroed at creation).  Kernels are handed addresses inside it, so every offset
// is fixed (asserted below); pad* are free words.
struct DevWords {
    unsigned int pad0[32];
    unsigned int fb_count;            // k = 1 search: queries on the fallback list (grid.hip)
    unsigned int far_count;           // ... on the far list: directly behind fb_count, the two are cleared together
    unsigned int pad1[6];
    unsigned int op[4];               // scalars of one operation: cluster count (cluster.hip), region growing's four words (region.hip)
    unsigned long long radius_total;  // CSR total of pcc_normals_radius
    unsigned int pad2[2];
    unsigned int icp_nsorted;         // valid points of the cell-ordered ICP source
    unsigned int pad3[3];
    unsigned int grid_ticket;         // ticket of the grid derivation fused into the build's pack kernel (grid_params_fused)
    unsigned int icp_ticket;          // ticket of the pass solve fused into k_icp_sums
    unsigned int pad4[10];
    SorStats sor;                     // pcc_sor's statistics
    unsigned int pad5[1024 - 64 - sizeof(SorStats) / 4];
    // open lanes of a listed k = 1 search, count of shard s in open[s][0] (a single word takes ~88 atomics per microsecond)
    unsigned int open[PCC_OPEN_SHARDS][PCC_OPEN_CTR_STRIDE];
    // PCC_TIES_FLANN, per slice s of the tie list: tie[s][0] queries listed as tied, [1] indices changed, [2] walks too deep
    unsigned int tie[PCC_TIE_SHARDS][PCC_OPEN_CTR_STRIDE];
};
static_assert(offsetof(DevWords, fb_count) == 4 * 32, "DevWords layout");
static_assert(offsetof(DevWords, far_count) == offsetof(DevWords, fb_count) + 4, "far_count directly behind fb_count");
static_assert(offsetof(DevWords, op) == 4 * 40, "DevWords layout");
static_assert(offsetof(DevWords, radius_total) == 4 * 44, "DevWords layout");
static_assert(offsetof(DevWords, icp_nsorted) == 4 * 48, "DevWords layout");
static_assert(offsetof(DevWords, grid_ticket) == 4 * 52, "DevWords layout");
static_assert(offsetof(DevWords, icp_ticket) == 4 * 53, "DevWords layout");
static_assert(offsetof(DevWords, sor) == 4 * 64, "DevWords layout");
static_assert(offsetof(DevWords, open) == 4 * 1024, "DevWords layout");
static_assert(offsetof(DevWords, tie) == 4 * 3072, "DevWords layout");
static_assert(sizeof(DevWords) == 14336, "DevWords layout");

// Clear the counters a k = 1 search starts from (fb_count, far_count, the open-lane shards) in the kernel in front of it, which
// saves the search its memset nodes; lanes 0..63 of one workgroup take part.  fb_count: &DevWords::fb_count of the handle.
__device__ __forceinline__ void clear_search_counters(unsigned int* __restrict__ fb_count) {
    constexpr unsigned int open0 = (offsetof(DevWords, open) - offsetof(DevWords, fb_count)) / 4;
    if (threadIdx.x < 64) {
        if (threadIdx.x < 2) fb_count[threadIdx.x] = 0u;
        fb_count[open0 + threadIdx.x * PCC_OPEN_CTR_STRIDE] = 0u;
    }
}

constexpr int PACK_MAX_BLOCKS = 1024;  // rows of per-workgroup statistics launch_pack writes at most

// The handle's pinned host words (pcc_index::pinned()).  fb_mirror and vox_count are written behind the host's back (by a kernel,
// by a copy nobody waits for) and read later, so they share no byte with anything else.
struct PinnedWords {
    alignas(8) unsigned int readback[4];  // read_back()
    unsigned int fb_mirror;               // fb_count of the last GRID k = 1 search, copied by k_unpack / k_icp_sums (grid_nn1 reads it
                                          // without a wait, pcc_index_stats after one)
    unsigned int vox_count;               // voxel_grid: the voxel count, copied without a wait and read after a later one
    float vox_rows[PACK_MAX_BLOCKS * 8];  // voxel_grid: the pack kernel's per-workgroup rows
};
static_assert(offsetof(PinnedWords, fb_mirror) >= sizeof(PinnedWords::readback) &&
                  offsetof(PinnedWords, vox_count) >= offsetof(PinnedWords, fb_mirror) + 4 &&
                  offsetof(PinnedWords, vox_rows) >= offsetof(PinnedWords, vox_count) + 4,
              "PinnedWords: the asynchronously written words overlap");

// ---- what a feature keeps on a handle between its stages and calls ------------------------------------------
// One slot per feature, filled at the feature's first call on the handle (scratch<T>() below) and destroyed with the handle.  A
// scratch type lives in its feature's file, names its slot, and holds owning members only: none has a destructor body.
struct Scratch { virtual ~Scratch() = default; };
enum ScratchSlot {
    SCRATCH_RIFT, SCRATCH_FPFH, SCRATCH_SIFT, SCRATCH_RIFT_BATCH, SCRATCH_SIFT_BATCH, SCRATCH_RGB_BATCH, SCRATCH_MATCH_COLOUR,
    SCRATCH_CLUSTER_DESC, SCRATCH_SEGMENT, SCRATCH_GROUND, SCRATCH_CHANGE, SCRATCH_MATCH_BATCH, SCRATCH_FPFH_BATCH,
    SCRATCH_VFH, SCRATCH_VFH_BATCH, SCRATCH_SHOT, SCRATCH_SLOTS
};
// A work handle: a second handle a feature indexes clouds of its own on (the caller's stream for the length of a call:
// entry.hpp, WorkLease).  Made at the first lease, destroyed with its owner.
struct WorkHandle {
    pcc_index* ix = nullptr;
    WorkHandle() = default;
    WorkHandle(const WorkHandle&) = delete;
    WorkHandle& operator=(const WorkHandle&) = delete;
    ~WorkHandle() { (void)pcc_index_destroy(ix); }
};

// rift.hip: what pcc_rift_descriptors keeps between its stages.  Buffers of their own: the radius searches in between use the
// handle's shared scratch.
struct RiftScratch : Scratch {
    static constexpr ScratchSlot slot = SCRATCH_RIFT;
    DevBuf rgb;                  // the caller's colour words, staged (host memory)
    DevBuf normals, inten;       // float4[n] plane fit; float[n] intensity, NaN outside cloud2
    DevBuf grad;                 // float4[n]: intensity gradient, w = 1 for the points of cloud2
    DevBuf hist, keep, scan_tmp; // float[n][32] before the last compaction; its flags / positions
    DevBuf out_hist, out_index;  // results staged for a caller in host memory
};
// sift.hip: what pcc_sift_keypoints keeps between its octaves and calls
struct SiftScratch : Scratch {
    static constexpr ScratchSlot slot = SCRATCH_SIFT;
    WorkHandle work;             // the handle the octave clouds are indexed on (scratch of its own)
    DevBuf pts, rgb;             // the caller's points / colour words, staged (host memory)
    DevBuf cloud[2];             // octave clouds, 32-byte records: the voxel grid reads one and writes the other
    DevBuf inten, resp;          // float[n] intensity; float[n][scales] Gaussian responses
    DevBuf nbr, nbr_d2;          // the k-NN rows of the extremum test
    DevBuf mask, count, scan_tmp;  // keypoint columns per point (bits), their number / positions
    DevBuf octaves;              // SiftOctave per octave
    DevBuf kp;                   // float4 keypoints of the call, every octave's in turn
};
// What every batch call keeps of its OWN between calls: the work handle the clouds off the batch route are
// indexed on, pinned staging going up and coming down, what `up` holds on the device.
struct BatchStaging : Scratch {
    WorkHandle work;
    HostBuf up, down;
    DevBuf dev;
};
struct RiftBatchItem;      // rift_batch_plan.hpp: a work item of the exhaustive row builder
// the staging and result buffers of pcc_match_knn_batch (match_batch.hip), pcc_match_knn_batch_dims (match_dims.hip),
// pcc_match_fpfh_batch (match_fpfh.hip) and pcc_cluster_matching (cluster_match.hip)
struct MatchBatchScratch : Scratch {
    static constexpr ScratchSlot slot = SCRATCH_MATCH_BATCH;
    HostBuf up, down, tree_up, tree_down;  // pinned: table + records going up, best + second coming down; trees + walk items, found
    DevBuf dev, res, tree_dev, tree_res;
};
struct HostPipe;           // host_pipe.hpp (api.hip): pipelined transfers between pageable host memory and the device
}  // namespace pcc
#define PCC_EV_SLOTS 64
#define PCC_EV_KINDS 10
// The opaque handle of the C-ABI.
struct pcc_index {
    std::mutex mu;                     // every entry point holds it: calls on ONE handle from several threads are serialised
    pcc::Options opt;                  // pcc_index_set_option
    int device = 0;
    hipStream_t stream = nullptr;      // stream in use
    hipStream_t own_stream = nullptr;  // library-owned stream
    hipEvent_t edge_ev = nullptr;      // pcc_index_wait_stream / pcc_stream_wait_index
    // Query staging beside the build (PCC_OPT_OVERLAP_PREP, api.hip: PrepOverlap).  params_ev is recorded behind k_grid_params of
    // every build; a search that is the NEXT call on the handle (build_fresh) sends its pack + query sort to side_stream behind
    // that event -- not behind the build's sort -- and the main stream picks the result up through side_ev.  The sort's scratch is
    // swapped for the `side` set meanwhile, so the two sorts share no buffer.
    hipStream_t side_stream = nullptr;
    hipEvent_t params_ev = nullptr, side_ev = nullptr;
    bool params_ev_set = false;        // params_ev was recorded by the build the handle currently holds, on the stream in use
    bool build_fresh = false;          // nothing has been enqueued on the handle since that build
    bool after_build = false;          // build_fresh as the entry point in progress found it
    bool edge_fresh = false;           // one pcc_index_wait_stream came between the build and now: side_stream waits for edge_ev too
    struct SideScratch {
        pcc::DevBuf a, b, c, e, mp_a, mp_b, mp_c, scan_flags;
        unsigned int scan_epoch = 0;
    } side;
    size_t n_orig = 0;                 // points handed to pcc_index_create / set_input
    size_t n_valid = 0;                // finite points (PCL total_nr_points_); valid after sync_info()
    unsigned int nc_cap = 0;           // upper bound of the grid's cell count the host sizes launches with
    pcc::DevBuf d_grid;                // GridDev on the device
    pcc::HostBuf h_grid_buf;           // pinned host mirror, filled asynchronously
    pcc::GridDev* h_grid() const { return h_grid_buf.as<pcc::GridDev>(); }
    bool stats_pending = false;        // fallback counter of the last GRID search in flight to pinned->fb_mirror
    size_t last_nq = 0;
    bool info_pending = false;         // h_grid copy in flight: sync before reading n_valid / grid / bbox
    int engine = PCC_ENGINE_BRUTE;     // resolved engine
    int engine_requested = PCC_ENGINE_AUTO;
    float bbox_lo[3] = {0, 0, 0}, bbox_hi[3] = {0, 0, 0};  // of the valid points
    // references in ORIGINAL order: (x, y, z, bits(index)), n_orig entries; non-finite points stay
    // in place flagged w = -1 (every kernel skips them), so position == original index
    pcc::DevBuf refs;
    // GRID engine: references permuted into cell order + CSR cell starts
    bool has_grid = false;
    pcc::GridParams grid{};
    pcc::DevBuf cell_refs;   // float4[n_valid], cell-sorted, .w = orig index
    pcc::DevBuf cell_start;  // uint32[ncells + 1]
    pcc::DevBuf seeds;       // float4[ceil(n / PCC_SEED_STRIDE)]: every 64th reference (w = its position; strides 32 / 128 / 256 measured 38.3 / 40.0 / 44.2 ms vs 38.0 on the ICP config) -- upper bounds for far queries
    unsigned int last_fallback_seen = 0;  // fallback count of an earlier search (heuristic only, may be stale)
    // scratch (grow-only, reused across calls on the index's stream)
    pcc::DevBuf q_raw, q_packed, out_packed, out_idx, out_d2, scratch_a, scratch_b,
        scratch_c, scratch_d, scratch_e, scratch_f, scratch_g, blk_stats, icp_src, icp_state, vox_a, vox_b, vox_c,
        mp_a, mp_b, mp_c,  // cellsort_mp.hip: two intermediate point buffers, bucket counters
        q_cells,     // grid cell of every staged query (k_pack), read by level 1 of the three-level sort instead of the points
        scan_flags,  // k_scan_chained: one tagged total per workgroup (pack.hip); nothing else ever writes here
        rows_idx, rows_d2;  // pcc_radius_fill_max: the k-NN rows it cuts at the radius (no scratch the query sort touches)
    // PCC_TIES_FLANN (flann_tree.hpp): kd-tree of FLANN's shape, built on the host at the first search after every
    // set_input, walked on the device (flann_order.hip)
    int tie_mode = PCC_TIES_LOWEST_INDEX;
    pcc::FlannTree flann;
    bool flann_valid = false;
    size_t small_raw_n = 0, small_raw_stride = 0;  // the indexed cloud's raw records are in the pinned small-call buffer (slot 0): n, stride; 0 = not
    int self_rows_k = 0;      // self_rows holds the self k-NN rows of the indexed cloud with this many neighbours (0: nothing kept)
    pcc::DevBuf self_rows;
    bool occ_valid = false;   // occ (device word): number of non-empty cells of the current grid, counted at the first radius count
    pcc::DevBuf occ;
    pcc::DevBuf tie_buf, flann_nodes, flann_leaf;
    pcc::DevBuf knn_fb;  // a list of up to n indices + its count, one user at a time: queries the k-NN selection kernel hands back,
                         // rows a fused radius fill leaves to k_sort_rows, region growing's points with a cross edge
    size_t q_cells_n = 0;                         // q_cells describes q_packed[0 .. q_cells_n) as staged (0: stale -- consumed, or q_packed has moved since)
    unsigned int scan_epoch = 0;                  // tag of the last chained scan on this handle
    bool sor_exact_last = true;                   // the last pcc_sor took its sums on the device (no addition of PCL's order rounds)
    bool open_pending = false;                    // the open-lane counters of the last listed k = 1 search are still on the device
    bool ties_pending = false;                    // the tie counters of the last search are still on the device
    uint64_t ties_flagged = 0, ties_changed = 0;  // of the last search in FLANN mode
    pcc::DevBuf words_buf;                                                   // pcc::DevWords, zeroed at creation
    pcc::DevWords* words() const { return words_buf.as<pcc::DevWords>(); }  // (a device pointer)
    pcc::HostBuf pinned_buf;                                                    // pcc::PinnedWords, zeroed at creation
    pcc::PinnedWords* pinned() const { return pinned_buf.as<pcc::PinnedWords>(); }
    pcc::HostBuf host_a, host_b;  // large pinned read-back buffers
    pcc::HostBuf host_c;          // pinned staging of the FLANN tree a small call builds (flann_order.hip)
    std::unique_ptr<pcc::HostPipe> pipe;  // two pinned chunk buffers + events, made at the first large host transfer (api.hip)
    std::unique_ptr<pcc::Scratch> scratch[pcc::SCRATCH_SLOTS];  // what the features keep here, made at their first call (pcc::scratch<T>())
    uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // HIP-event instrumentation (pcc_index_enable_timing): event pairs on the index's stream
    // ring of PCC_EV_SLOTS calls so a timed region of many steps is covered without syncing
    int timing = 0;  // 0 off, 1 main kernel only (2 events per call), 2 full breakdown
    hipEvent_t ev[PCC_EV_SLOTS][PCC_EV_KINDS] = {};
    bool ev_rec[PCC_EV_SLOTS][PCC_EV_KINDS] = {};
    unsigned int ev_slot = 0;  // slot of the call in flight
    ~pcc_index();  // api.hip: scratches, then streams and events, then the buffers -- under pcc_index_destroy's device guard
};

namespace pcc {

// A search key is (d2 bits << 32 | position); ~0 means "nothing found".  FLANN starts every result set with a worst
// distance of FLT_MAX and rejects dist >= worst (KNNSimpleResultSet), so a candidate whose squared distance
// overflowed -- coordinates around 1e19 -- is no neighbour either: every consumer of a key treats d2 >= FLT_MAX like ~0.
// (The searches themselves keep such candidates: they only matter when nothing finite exists.)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline bool key_none(unsigned long long key) { return (unsigned int)(key >> 32) >= 0x7f7fffffu; }

// the grid of a grid-stride kernel of 256 lanes a workgroup over n elements: a workgroup each, 2048 at the most
inline unsigned int blocks_for(size_t n) { return (unsigned int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048); }

// the scratch of feature T on a handle, made at the first use
template <class T>
T* scratch(pcc_index* ix) {
    std::unique_ptr<Scratch>& s = ix->scratch[T::slot];
    if (!s) s = std::make_unique<T>();
    return static_cast<T*>(s.get());
}

enum { EV_MAIN0 = 0, EV_MAIN1, EV_FB0, EV_FB1, EV_CALL0, EV_CALL1, EV_BUILD0, EV_BUILD1, EV_SORT0, EV_SORT1 };
// every entry point that may enqueue work passes here once it holds the handle's mutex
inline void entered(pcc_index* ix) {
    ix->after_build = ix->build_fresh;
    ix->build_fresh = false;
}
inline void ev_mark(pcc_index* ix, int id) {
    if (!ix->timing || (ix->timing == 1 && id > EV_MAIN1)) return;
    unsigned int s = ix->ev_slot % PCC_EV_SLOTS;
    if (ix->ev[s][id]) { (void)hipEventRecord(ix->ev[s][id], ix->stream); ix->ev_rec[s][id] = true; }
}
// a new instrumented call begins: advance the ring and forget what the slot held
inline void ev_next(pcc_index* ix) {
    if (!ix->timing) return;
    ++ix->ev_slot;
    unsigned int s = ix->ev_slot % PCC_EV_SLOTS;
    for (int k = 0; k < PCC_EV_KINDS; ++k) ix->ev_rec[s][k] = false;
}

// N device values read back synchronously: copied into the handle's pinned read-back words, the handle's stream waited for
template <int N = 1, class T>
int read_back(pcc_index* ix, const T* dev, T* out) {
    static_assert(N * sizeof(T) <= sizeof(PinnedWords::readback) && alignof(T) <= alignof(PinnedWords), "read_back: too large");
    PCC_HIP(hipMemcpyAsync(ix->pinned()->readback, dev, N * sizeof(T), hipMemcpyDeviceToHost, ix->stream));
    PCC_HIP(hipStreamSynchronize(ix->stream));
    memcpy(out, ix->pinned()->readback, N * sizeof(T));
    return PCC_OK;
}

// ---- kernels / launchers (pack.hip) -------------------------------------------
// AoS (stride bytes, 3 floats at offset 0) -> float4(x,y,z,bits(i)); non-finite points are
// written with w = -1.
// PackGrid (index builds): the pack kernel's last workgroup also derives the index's grid (what k_grid_params does in
// a launch of its own): ticket = a zeroed device word, the rest are k_grid_params' arguments
struct PackGrid {
    unsigned int* ticket;
    float ppc;
    unsigned int nc_cap;
    int trim_k, axes;
    GridDev* out;
    GridDev* host_mirror;
};
// What a pack launch writes besides the packed points; what is left empty is not written.
struct PackExtras {
    float* blk_stats = nullptr;  // 8 floats per workgroup: [0] bits(invalid count), [1..3] min xyz, [4..6] max xyz of its valid points
    int* n_blocks = nullptr;     // host word: the number of workgroups launched (rows of blk_stats)
    unsigned int* zero_word = nullptr;           // &DevWords::fb_count: clears the counters of a k = 1 search (clear_search_counters)
    float4* seeds = nullptr;                     // (with blk_stats) every PCC_SEED_STRIDE-th point
    unsigned long long* invalid_keys = nullptr;  // result key of every non-finite point preset to "nothing found"
    unsigned int* cells = nullptr;               // (without blk_stats) the cell of every point in the grid *gd describes
    const GridDev* gd = nullptr;
    PackGrid grid{};             // (with blk_stats) used when grid.out is set
    bool indexed_cloud = false;  // read by stage_points alone: a small cloud goes to pinned slot 0 and its raw records stay (small_tie_replay)
};
int launch_pack(hipStream_t s, const void* aos, size_t n, size_t stride, float4* out, const PackExtras& x);
// exclusive scan of uint32 data[n] in place; data[n] receives the total when
// write_total.  tmp is grown as needed.
int launch_exclusive_scan(pcc_index* ix, hipStream_t s, unsigned int* data, size_t n, DevBuf& tmp);
// packed u64 keys (d2 bits << 32 | packed position) -> original idx, d2; n keys; q (nullable,
// one per key) flags invalid queries (w < 0) which get -1/+inf, as do empty keys (~0)
// mirror (nullable): device word copied to *mirror_host (pinned) by the kernel -- fallback counter for stats
int launch_unpack(hipStream_t s, const unsigned long long* packed, const float4* q, size_t n,
                  int32_t* idx, float* d2, const unsigned int* mirror_dev = nullptr, unsigned int* mirror_host = nullptr);
int launch_transform(hipStream_t s, const float* T16_dev_or_null, const float T[16],
                     const void* src, size_t n, size_t sstride, void* dst, size_t dstride, unsigned int* zero_word = nullptr);
// packed points whose w flags them invalid get NaN coordinates again (in place): what a raw cloud looked like
int launch_nanify(hipStream_t s, float4* pts, size_t n);
// dst[i].w = src[i].w (validity flags of packed points)
int launch_gather_sorted(hipStream_t s, const float4* q, const unsigned int* order, const unsigned int* n_sorted, size_t n, float4* dst,
                         unsigned int* ns_word);
int launch_copy_w(hipStream_t s, const float4* src, float4* dst, size_t n);
// SOR: mean_dist[orig(i)] = float(sum_{j=1..K-1} sqrt(double(d2_j)) / (K-1)) from the K-NN keys of
// the self query; rows with fewer than K neighbours keep 0
int launch_sor_mean(hipStream_t s, const unsigned long long* keys, const float4* refs, size_t n, int K,
                    float* mean_dist, const float* d2_rows = nullptr);
// SOR: sum / sq_sum / threshold / inlier mask of the mean distances on the device (pack.hip) into *stats_dev
int launch_sor_stats(hipStream_t s, const float* m, size_t n, const GridDev* gd, int K, double stddev_mult, double* scratch,
                     SorStats* stats_dev, uint8_t* inlier_dev);
int launch_sor_partial(hipStream_t s, const float* m, size_t n, double* scratch, double* out4_dev);
int launch_sor_threshold_mask(hipStream_t s, const float* m, size_t n, const GridDev* gd, int K, double stddev_mult,
                              const double* in4_dev, SorStats* stats_dev, uint8_t* inlier_dev);
void sor_threshold_host(const double in4[4], double n_valid, int K, double stddev_mult, double* thr, int* exact);
// ---- sor.hip: what pcc_sor, pcc_sor_partial and pcc_sor_sharded (comm.hip) share, over the points [start, start + count) ----
constexpr size_t SOR_STATS_OUT4 = 3 * 1024;  // scratch of launch_sor_stats / _partial: 3 x 1024 partial doubles, then the four results
constexpr size_t SOR_STATS_SCRATCH_BYTES = (SOR_STATS_OUT4 + 4) * sizeof(double) + 64;
int sor_begin(pcc_index* ix, size_t start, size_t count, int mean_k);  // the arguments, and the grid the search needs
// the mean stage: self K-NN of those points (K = mean_k + 1) and their mean distances, *dmean (ix->out_d2, `count` floats)
int sor_means(pcc_index* ix, size_t start, size_t count, int K, float** dmean);
// the in-order fallback: PCL's sums over ALL `no` mean distances (host memory) in index order -> threshold, kept count over the
// whole cloud, and the inlier mask of those points in mask[0 .. count)
void sor_in_order(const float* hm, size_t no, size_t n_valid, int K, double stddev_mult, size_t start, size_t count, double* thr,
                  size_t* kept, uint8_t* mask);
int launch_clamp_counts(hipStream_t s, int32_t* counts, size_t n, int32_t cap);
int launch_knn_rows_to_csr(hipStream_t s, const unsigned long long* keys, const int32_t* ridx, const float* rd2, int K, float r2,
                           const int64_t* offsets, size_t nq, int32_t* idx_out, float* d2_out);
int launch_copy_row_prefix(hipStream_t s, const unsigned long long* src, int k_src, unsigned long long* dst, int k_dst, size_t n);

// ---- exhaustive engine (nn1_brute.hip) -------------------------------------------
// For every query q[i] (float4, w<0 = invalid) min over refs[0..m) of the unfused
// squared distance, lowest original index on ties, merged into out[i] with a 64-bit
// atomicMin (out must be pre-set to ~0).  If qlist != nullptr only the queries
// qlist[0..*qcount) are processed (GRID fallback list; count read on device).
// idx_from_w (list mode only): report refs[p].w as the index instead of p (seed subset, see grid.hip)
int launch_nn1_brute(hipStream_t s, const float4* refs, size_t m, const float4* q,
                     size_t n, unsigned long long* out, const unsigned int* qlist,
                     const unsigned int* qcount_dev, size_t qcount_max, bool idx_from_w = false);

// ---- small-call form (small.hip): the query side of a k = 1 call in one launch -- raw host-pinned queries in, (idx, d2) out into
// pinned host memory, q_packed / out_packed written as the separate launches would
int launch_small_nn1(hipStream_t s, const void* raw_q, size_t nq, size_t stride, const float4* refs, size_t n, float4* q_packed,
                     unsigned long long* out_packed, int32_t* idx, float* d2, unsigned int* tie_blocks, unsigned char* tie_q);  // PCC_TIES_FLANN: tied queries per 64 (pinned) and a flag per query (device)
constexpr size_t SMALL_FUSED_REFS = 4096;    // indexed clouds up to here take it (PCC_ENGINE_AUTO's exhaustive range)
constexpr size_t SMALL_FUSED_POINTS = 8192;  // indexed clouds up to here: the grid parameters come from the pack kernel's last workgroup

// ---- grid.hip --------------------------------------------------------------------------
int grid_params(pcc_index* ix, const float* blk_stats_dev, int n_blocks);  // async: d_grid + pinned mirror
int grid_params_fused(pcc_index* ix, PackGrid* pg);                        // the same from inside the pack kernel: fills *pg for launch_pack
int grid_build(pcc_index* ix);                                             // async: cell sort of the references
int sync_info(pcc_index* ix);                                              // wait for the pinned mirror, refresh host fields
unsigned int grid_nc_cap(size_t n, double ppc);
// What ONE k = 1 search is told by its caller, on the caller's stack (nn1_packed -> grid_nn1; the exhaustive engine needs none of
// it).  Default-constructed: a plain search that sorts its queries itself.
struct Nn1Call {
    // order_given: the lane order is given for order_nq queries (order == nullptr: the identity).  An ICP pass (icp_pass) that sorts
    // leaves its order here as given: the loop keeps one struct, a rigid motion keeps neighbouring points neighbours, and any
    // permutation of the valid queries is correct, so its later passes skip the sort.  No other search's order is reused
    bool order_given = false;
    unsigned int *order = nullptr, *n_sorted = nullptr;  // (n_sorted: device word, the number of valid queries)
    size_t order_nq = 0;
    bool counters_cleared = false;  // the pack / transform / solve kernel in front has cleared fb_count, far_count and the open-lane
                                    // shards (clear_search_counters); the search uses them up
    bool icp_pass = false;          // a pass of pcc_icp_align: plain box instead of the ball walk, far route in auto mode
    bool warm = false;              // (ICP passes) out[] holds the previous pass's keys of the same queries: the search starts from them
    const float* pre_transform = nullptr;  // cell-ordered ICP loop: the 3 x 4 matrix (device memory) the search applies to its queries, and writes
                                           // back, before it looks -- the pass's k_transform; needs grid_nn1_takes_transform, identity order
};
int grid_nn1(pcc_index* ix, const float4* q, size_t nq, unsigned long long* out, Nn1Call& call);
bool grid_nn1_takes_transform(const pcc_index* ix);
// sort queries by reference-grid cell: order[0..*n_sorted) (device) lists the valid queries
int grid_sort_queries(pcc_index* ix, const float4* q, size_t nq, unsigned int** order_dev,
                      unsigned int** n_sorted_dev);
float grid_slack(const GridParams& g);
// ---- cellsort.hip: LDS-based two-level counting sort by cell ---------------------------------------
int cell_sort(pcc_index* ix, const float4* pts, size_t n, bool refs, float4* out_pts, unsigned int* out_order,
              unsigned int* cell_start, unsigned int** n_sorted_dev, const GridDev* gd_override = nullptr,
              unsigned int nc_cap_override = 0);
// ---- cellsort_mp.hip: the same contract in three coalesced levels (large clouds); out_pts may also be given for queries
int cell_sort_mp(pcc_index* ix, const float4* pts, size_t n, bool refs, float4* out_pts, unsigned int* out_order,
                 unsigned int* cell_start, unsigned int** n_sorted_dev, const GridDev* gd_override = nullptr,
                 unsigned int nc_cap_override = 0);
// ---- voxel.hip: pcl::VoxelGrid (leaf-lattice centroids) ---------------------------------------------
int voxel_grid(pcc_index* ctx, const void* pts, size_t n, size_t stride, int mem, float leaf, int has_rgb,
               void* out, size_t out_stride, size_t* out_n);
// ---- knn.hip: k-NN, radius search (GRID engine) ----------------------------------------
// keys[nq][K] (pre-set to ~0) receive the K smallest (d2, position) keys ascending
int grid_knn(pcc_index* ix, const float4* q, size_t nq, int K, unsigned long long* keys, int32_t* idx_out = nullptr,
             float* d2_out = nullptr);
bool grid_knn_delivers(int K);
// the self k-NN rows (keys) of the indexed cloud with k neighbours, kept between calls under PCC_OPT_KNN_CACHE_K
int self_knn_keys(pcc_index* ix, int k, const unsigned long long** keys);
// counts[i] = #refs with d2 < r2; with fill != 0 also writes keys at offsets[i]..
// idx_out / d2_out / delivered (fill only): when given, a fill that takes the wave-per-query route writes the caller's
// arrays itself (sorted in registers) and sets *delivered
// a fill whose rows hold this many neighbours and more on average takes the wave-per-query route (api.hip radius_fill_impl
// decides the memset by it, knn.hip grid_radius the kernel: the two must agree)
constexpr unsigned int RAD_WAVE_MEAN = 24;
int grid_radius(pcc_index* ix, const float4* q, size_t nq, float r, float r2, int32_t* counts,
                const int64_t* offsets, unsigned long long* keys, int sorted, size_t total = 0, int32_t* idx_out = nullptr,
                float* d2_out = nullptr, bool* delivered = nullptr);
constexpr int PCC_ERR_RETRY_HOST = -1000;  // sac_plane without a host array met a degenerate sample: repeat with one (internal)
// sac.hip: the loop of pcc_plane_removal over a cloud's records (arguments checked, n > 0).  It stages the cloud in q_packed and
// ping-pongs it with vox_a, the original indices between vox_b and vox_c; waits only where sac_plane() waits.  PCC_ERR_OVERFLOW
// (more than max_planes planes) leaves the counts of the planes found.
struct PlaneLoop {
    const void* pts = nullptr;  // records in space `mem`; a host array is read on turn 0 (single points)
    size_t n = 0, stride = 0;
    int mem = 0;
    double stop_fraction = 0, threshold = 0, probability = 0;
    int max_iterations = 0, optimize = 0;
    size_t max_planes = 0;
    float* out_coefficients = nullptr;     // host tables, as pcc_plane_removal's
    uint32_t* out_plane_sizes = nullptr;
    int* out_iterations = nullptr;         // nullable
    int* ended_without_model = nullptr;    // nullable
    int32_t* plane_of_point = nullptr;     // device, nullable
    // results
    size_t planes = 0, remaining = 0;
    uint64_t host_copies = 0;              // turns that took a host copy of the current cloud (a degenerate sample)
    const int32_t* remaining_index = nullptr;  // device: the original indices of the points that remain, ascending (vox_b or vox_c)
};
int plane_loop(pcc_index* ix, PlaneLoop& L);
int check_plane_loop(double stop_fraction, int max_iterations, double threshold, double probability, size_t max_planes,
                     const float* out_coefficients, const uint32_t* out_plane_sizes, const void* n_planes, const void* n_remaining);
// out record j = the first record_bytes of input record idx[j] (k_planes_records), both on the device
int launch_plane_records(hipStream_t s, const void* in, size_t stride, const int32_t* idx, size_t m, size_t record_bytes, void* out,
                         size_t out_stride);
// cluster.hip: pcl::EuclideanClusterExtraction over the indexed cloud, labels_dev[n_orig].  device_rank: up to EC_RANK_MAX clusters
// are numbered by k_ec_rank instead of the host sort (one wait, for the count)
constexpr unsigned int EC_RANK_MAX = 2048;
int grid_clusters(pcc_index* ix, float r, float r2, uint32_t min_size, uint32_t max_size, int32_t* labels_dev, int32_t* n_clusters,
                  int32_t* sizes, int max_sizes, bool device_rank = false);
// the two halves of pcc_normals_radius (normals.hip): the sorted self radius rows of the indexed cloud as a CSR (keys: d2 bits << 32 | point
// index; offsets[n + 1]; both stay valid until the next radius search on the handle), and the plane fit over such rows
int radius_csr(pcc_index* ix, double radius, const unsigned long long** keys, const unsigned int** offsets);
int launch_normals_csr(pcc_index* ix, const unsigned long long* keys, const unsigned int* offsets, const float vp[3], float4* out);
// the plane fit over the rows of any packed cloud: refs[n], `order` a cell_refs-shaped array whose first gd->n_valid entries name
// the points to take (their w)
int launch_normals_csr(hipStream_t s, const float4* refs, const float4* order, const GridDev* gd, size_t n, const unsigned long long* keys,
                       const unsigned int* offsets, const float vp[3], float4* out);
// the middle of a CSR build (normals.hip): counts off32[n] (off32[n] = 0) -> exclusive offsets in place (off32[n] = the total) and
// widened into off64[n + 1]; *total on the host (the build's one wait); 2^32 entries and more are PCC_ERR_OVERFLOW
int csr_offsets(pcc_index* ix, unsigned int* off32, int64_t* off64, size_t n, unsigned long long* total);
// knn.hip: every row of a CSR somebody else filled, sorted ascending in place (k_sort_rows)
int sort_csr_rows(hipStream_t s, const int64_t* offsets, size_t n, unsigned long long* keys);
// rift.hip: the RIFT descriptor pipeline on device arrays; *n_out on the host
int rift_descriptors(pcc_index* ix, const unsigned char* rgb, size_t rgb_stride, double normal_radius, double gradient_radius,
                     double rift_radius, float* out_hist, int32_t* out_index, size_t* n_out);
// the radius and bin checks of pcc_rift_descriptors and its batch form (rift.hip)
int check_rift_params(double normal_radius, double gradient_radius, double rift_radius, int nr_distance_bins, int nr_gradient_bins);
// the same stages over any packed cloud (rift_batch.hip: the concatenation of a batch): see rift.hip
typedef std::function<int(double radius, const unsigned long long** keys, const unsigned int** offsets)> RiftRows;
int rift_stages(pcc_index* ix, const float4* refs, const float4* order, const GridDev* gd, size_t n, const RiftRows& rows,
                const unsigned char* rgb, size_t rgb_stride, double normal_radius, double gradient_radius, double rift_radius,
                float* out_hist, int32_t* out_index);
// rift_batch.hip: pcc_rift_descriptors_batch behind its argument checks
int rift_descriptors_batch(pcc_index* ix, const CloudBatch& batch, double normal_radius, double gradient_radius, double rift_radius,
                           float* out_hist, int32_t* out_index, size_t* out_offsets);
// rift_batch.hip: the sorted radius rows (d2 < r2, ascending (d2, index)) of a concatenation of clouds as one CSR, from the exhaustive
// builder: d_items (device) are query blocks of one cloud each, d_pts the concatenation with w = bits(concatenated index).  offs / keys:
// the caller's buffers for uint32 offsets[total + 1] (+ the same as int64) and the entries.  One wait: the CSR's total
int batch_radius_rows(pcc_index* ix, const RiftBatchItem* d_items, unsigned int n_items, const float4* d_pts, size_t total, float r2,
                      DevBuf& offs, DevBuf& keys, const unsigned long long** keys_out, const unsigned int** offsets_out);
// rift_batch.hip: after the stages over a concatenation of n points (pos = the exclusive scan of the kept points' flags, pos[n] = the
// rows written): slice[c] .. slice[c + 1] are the rows of cloud c, and every point index in out_index loses its cloud's base
int launch_batch_finish(hipStream_t s, const unsigned int* pos, const unsigned int* bases, size_t n_clouds, size_t n, unsigned int* slice,
                        int32_t* out_index);
// fpfh.hip: the radius and bin checks of pcc_fpfh_descriptors and its batch form
int check_fpfh_params(double normal_radius, double fpfh_radius, int nr_bins_f1, int nr_bins_f2, int nr_bins_f3);
// fpfh.hip: the stages of pcc_fpfh_descriptors over any packed cloud (fpfh_batch.hip: the concatenation of a batch), arguments as
// rift_stages'.  normals (nullable): the caller's own plane fit -- it fills normals[n] and hands over the CSR at fpfh_radius, and
// `rows` is not asked.  *pos: uint32[n + 1] on the device, where every point of cloud2 lies in the output, pos[n] = the rows written
// vfh.hip: the null-argument and radius checks of pcc_vfh_descriptor
int check_vfh_params(double normal_radius, const float* out_hist, const size_t* n_out);
typedef std::function<int(float4* normals, const unsigned long long** keys, const unsigned int** offsets)> FpfhNormals;
int fpfh_stages(pcc_index* ix, const float4* refs, const float4* order, const GridDev* gd, size_t n, const RiftRows& rows,
                double normal_radius, double fpfh_radius, const FpfhNormals* normals, float* out_hist, int32_t* out_index,
                const unsigned int** pos);
// sift.hip: the detector on device arrays: the keypoints are left in SiftScratch::kp, *n_out of them
int sift_keypoints(pcc_index* ix, const unsigned char* pts, size_t n, size_t stride, const unsigned char* rgb, size_t rgb_stride,
                   float min_scale, int nr_octaves, int nr_scales_per_octave, float min_contrast, size_t* n_out);
// The partition machinery the segmentation calls share (segment.hip).  extract_order: labels[n]
// on the device, n > 0, n_clusters > 0 -> *order (uint32[n]: the kept points key by key, ascending inside a key, then the points
// left out (label -1)) and *offsets (uint32[n_clusters + 1]; offsets_out may be null: not computed), both in SegmentScratch; everything
// enqueued, nothing waited for.
// offsets_to_host / offsets_arrived: the offsets and the bad-label flag on their way to the host, and read after the caller's wait.
// launch_records: out record j = the first record_bytes of input record order[j].  give: a result in a buffer of the library's into
// the caller's array in either space (host: through deliver; the caller waits).
int extract_order(pcc_index* ix, const int32_t* labels, size_t n, int32_t n_clusters, const unsigned int** order_out,
                  const unsigned int** offsets_out);
int offsets_to_host(pcc_index* ix, const unsigned int* d_offsets, int32_t n_clusters);
int offsets_arrived(pcc_index* ix, int32_t n_clusters, size_t* out_offsets);
int launch_records(hipStream_t s, const void* in, size_t stride, const unsigned int* order, size_t m, size_t record_bytes, void* out,
                   size_t out_stride);
int give(pcc_index* ix, int mem, void* user, const void* dev, size_t bytes);
// normals.hip: the plane fit over the self k-NN rows `keys` (n x K) of a packed cloud
int launch_normals(hipStream_t s, const unsigned long long* keys, const float4* refs, const float4* cell_refs, const GridDev* gd, size_t n,
                   int K, const float vp[3], float4* out);
// region.hip: pcl::RegionGrowing over the self k-NN rows of the index; *sweeps (nullable) = the sweeps it took to settle
int grid_region_growing(pcc_index* ix, const unsigned long long* keys, const float4* normals, int K, float smoothness,
                        float curvature_threshold, uint32_t min_size, uint32_t max_size, int32_t* labels_dev, int32_t* n_clusters,
                        unsigned int* sweeps = nullptr);
int grid_first_within(pcc_index* ix, const float4* q, size_t nq, double radius, int32_t* idx_dev);
// ---- flann_order.hip: flags[i] = 1 when another reference shares query i's minimum distance; the tied queries walked
// through FLANN's tree on the device
int resolve_ties_flann(pcc_index* ix, const float4* q, unsigned long long* keys, size_t nq, bool may_wait = false);
// The small-call form of the replay (small.hip has flagged the tied queries, tie_q[i] != 0, and the indexed cloud's raw records are
// still in the pinned buffer): tree built from those records, uploaded without a wait, ONE launch walks the flagged queries and
// writes the changed indices into idx_host (pinned) and their number per 64 queries into changed_blocks (pinned).  *done = false:
// the tree is deeper than the device walk takes, nothing was enqueued (the caller takes resolve_ties_flann).
int small_tie_replay(pcc_index* ix, const void* raw_refs, size_t nq, const unsigned char* tie_q, int32_t* idx_host,
                     unsigned int* changed_blocks, bool* done);
// ---- icp.hip -----------------------------------------------------------------------------
// per-workgroup partial sums (17 doubles each) of the matched pairs; returns #blocks written
struct IcpState;
// fuse (device-resident loop on one GPU): the last workgroup of k_icp_sums to finish also solves the pass (k_icp_solve's work);
// ticket = a zeroed device word; center_dev must be given
struct IcpFuse {
    unsigned int* ticket;
    IcpState* st;
    int max_iter, fixed;
    unsigned int* zero_word;
};
int launch_icp_sums(hipStream_t s, const float4* src, size_t n, const unsigned long long* keys,
                    const float4* refs, double* partials, int* n_blocks, const unsigned int* mirror_dev = nullptr,
                    unsigned int* mirror_host = nullptr, const double* center_dev = nullptr,  // sums of p - center, q - center (device pointer)
                    const IcpFuse* fuse = nullptr);
constexpr int ICP_MAX_BLOCKS = 480;  // (480 rows of 17 doubles fit the 64 KB of LDS k_icp_solve stages them in)
// state of the device-resident ICP loop (pcc_icp_align): no host round trip per pass
struct IcpState {
    float Ti[16];     // transform of the pass just solved (identity once the loop has stopped)
    float T[16];      // running product T_i * ... * T_1
    double prev_mse;  // mean squared distance of the previous pass (convergence test)
    int it;           // iterations completed
    int stopped;      // the loop has ended (criteria met, iteration cap, or too few correspondences): later passes are no-ops
    int converged;    // pcl::DefaultConvergenceCriteria's verdict at the stop
};
int launch_icp_solve(hipStream_t s, const double* partials, int n_blocks, IcpState* state, int max_iter, int fixed,
                     const double* center_dev, unsigned int* zero_word = nullptr);
// collectives of the sharded ICP loop, supplied by comm.hip (RCCL on the handle's stream); icp.hip knows no RCCL type
struct IcpHooks {
    void* ctx;
    int (*allreduce_sum_f64)(void* ctx, double* dev, int count, hipStream_t s);
    int (*bcast_f64)(void* ctx, double* dev, int count, int root, hipStream_t s);
    int (*agree)(void* ctx, int local_status);  // the worst status over the ranks (one all-reduce): same return everywhere
};
int icp_align_impl(pcc_index* ix, const IcpHooks* hooks, const void* src, size_t n, size_t stride, int mem, int max_iter, int fixed,
                   float T[16], double* fitness, int* iterations, int* converged);
// ---- api.hip internals the other files build on ----------------------------------------------------------------------
// match_dims.hip: the search of pcc_match_knn_batch_dims for dim != 3 (arguments checked by the entry point in match_batch.hip)
int match_knn_batch_dims(pcc_index* ix, size_t n_pairs, const void* const* des1, const size_t* n1, const void* const* des2,
                         const size_t* n2, size_t stride, int dim, float threshold, int32_t* out, float* out_d2, size_t* out_offsets);
// match_fpfh.hip: the search of pcc_match_fpfh_batch (arguments checked by the entry point in match_batch.hip)
int match_fpfh_batch(pcc_index* ix, size_t n_pairs, const void* const* des1, const size_t* n1, const void* const* des2,
                     const size_t* n2, size_t stride, int mem, float threshold, int32_t* out, float* out_d2, size_t* out_offsets);
int check_mem(int mem);  // PCC_MEM_HOST or PCC_MEM_DEVICE
int check_points(const void* pts, size_t n, size_t stride, int mem);
int stage_queries(pcc_index* ix, const void* q, size_t nq, size_t stride, int mem, Nn1Call* search = nullptr);
int nn1_packed(pcc_index* ix, size_t nq, Nn1Call& call);
int set_input(pcc_index* ix, const void* pts, size_t n, size_t stride, int mem);
int make_handle(int device, int engine, pcc_index** out);  // an empty handle on `device`

}  // namespace pcc
