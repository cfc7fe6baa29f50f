// api.hip -- the handle of libpcc_nn's C-ABI (include/pcc_nn.h) -- lifecycle, options, streams, staging of clouds -- and the point
// searches on it; every other operation's entry points live beside its kernels.
// Host-side glue only: argument checks, H2D/D2H staging, launch order.  There is
// no CPU compute fallback: without a HIP device every entry point fails with
// PCC_ERR_DEVICE.
#include "entry.hpp"
#include <atomic>
#include "host_pipe.hpp"
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>
#include <algorithm>
#include <thread>

namespace pcc {

#ifdef PCC_COUNT_PAIRS
unsigned long long pairs_take_grid();
unsigned long long pairs_take_knn();
unsigned long long pairs_take_cluster();
unsigned long long pairs_take_flann();
unsigned long long pairs_take_rift_batch();
unsigned long long pairs_take_rgb_batch();
#endif

static thread_local std::string g_err;
void set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}

// Every option of a handle, once: its id, the PCC_* environment variable that supplies a new handle's default, the member of
// Options it lives in (an int or a double) and the values it takes, whoever sets it (pcc_index_set_option or the environment).
// An int option takes any value inside its range and keeps its truncation.
struct OptionRow {
    enum Kind { CLOSED, ABOVE_LO, FLAG };  // lo <= v <= hi; lo < v <= hi; exactly 0 or 1
    int id;
    const char* env;
    int Options::*i;
    double Options::*d;
    double lo, hi;  // (hi = HUGE_VAL: no upper bound)
    Kind kind;
    bool takes(double v) const { return std::isfinite(v) && (kind == FLAG ? v == 0 || v == 1 : (kind == ABOVE_LO ? v > lo : v >= lo) && v <= hi); }
};
static const OptionRow g_options[] = {
    {PCC_OPT_GRID_PPC, "PCC_GRID_PPC", nullptr, &Options::grid_ppc, 0, 1024, OptionRow::ABOVE_LO},
    {PCC_OPT_GRID_TRIM, "PCC_GRID_TRIM", &Options::grid_trim, nullptr, 0, 8, OptionRow::CLOSED},
    {PCC_OPT_FAR_MODE, "PCC_GRID_FAR", &Options::far_mode, nullptr, -1, 1, OptionRow::CLOSED},
    {PCC_OPT_ICP_WARM, "PCC_ICP_WARM", &Options::icp_warm, nullptr, 0, 1, OptionRow::FLAG},
    {PCC_OPT_ICP_DEVICE_LOOP, "PCC_ICP_DEVICE_LOOP", &Options::icp_device_loop, nullptr, 0, 1, OptionRow::FLAG},
    {PCC_OPT_EC_CELLS, "PCC_EC_CELLS", &Options::ec_cells, nullptr, 0, 4, OptionRow::CLOSED},
    {PCC_OPT_SORT_MP_MIN, "PCC_SORT_MP_MIN", nullptr, &Options::sort_mp_min, 0, HUGE_VAL, OptionRow::CLOSED},
    {PCC_OPT_SORT_MP_MIN_Q, "PCC_SORT_MP_MIN_Q", nullptr, &Options::sort_mp_min_q, 0, HUGE_VAL, OptionRow::CLOSED},
    {PCC_OPT_NN1_KERNEL, "PCC_NN1_KERNEL", &Options::nn1_kernel, nullptr, 0, 3, OptionRow::CLOSED},
    {PCC_OPT_FLANN_SPLIT, "PCC_FLANN_SPLIT", &Options::flann_split, nullptr, 0, 2, OptionRow::CLOSED},
    {PCC_OPT_NN1_DENSE_MIN, "PCC_NN1_DENSE_MIN", &Options::nn1_dense_min, nullptr, 1, 1000000, OptionRow::CLOSED},
    {PCC_OPT_KNN_KERNEL, "PCC_KNN_KERNEL", &Options::knn_kernel, nullptr, 0, 1, OptionRow::FLAG},
    {PCC_OPT_KNN_CACHE_K, "PCC_KNN_CACHE_K", &Options::knn_cache_k, nullptr, 0, 512, OptionRow::CLOSED},
    {PCC_OPT_NN1_OPEN_FLAT, "PCC_NN1_OPEN_FLAT", &Options::nn1_open_flat, nullptr, 0, 1, OptionRow::FLAG},
    {PCC_OPT_SORT_STAGE1, "PCC_SORT_STAGE1", &Options::sort_stage1, nullptr, 0, 2, OptionRow::CLOSED},
    {PCC_OPT_ICP_SORTED, "PCC_ICP_SORTED", &Options::icp_sorted, nullptr, 0, 1, OptionRow::FLAG},
    {PCC_OPT_OVERLAP_PREP, "PCC_OVERLAP_PREP", &Options::overlap_prep, nullptr, 0, 2, OptionRow::CLOSED},
    {PCC_OPT_GRID_AXES, "PCC_GRID_AXES", &Options::grid_axes, nullptr, -2, 5, OptionRow::CLOSED},
    {PCC_OPT_XCD_RUN, "PCC_XCD_RUN", &Options::xcd_run, nullptr, 1, 4096, OptionRow::CLOSED},
    {PCC_OPT_FUSE_PARAMS, "PCC_FUSE_PARAMS", &Options::fuse_params, nullptr, 0, 3, OptionRow::CLOSED},
    {PCC_OPT_HOST_PIPE, "PCC_HOST_PIPE", &Options::host_pipe, nullptr, 0, 1, OptionRow::FLAG},
    {PCC_OPT_SCAN_CHAINED, "PCC_SCAN_CHAINED", &Options::scan_chained, nullptr, 0, 1, OptionRow::FLAG},
    {PCC_OPT_KNN_RUN, "PCC_KNN_RUN", &Options::knn_run, nullptr, 1, 64, OptionRow::CLOSED},
    {PCC_OPT_RIFT_LAYOUT, "PCC_RIFT_LAYOUT", &Options::rift_layout, nullptr, 0, 1, OptionRow::FLAG},
    {PCC_OPT_SIFT_LAYOUT, "PCC_SIFT_LAYOUT", &Options::sift_layout, nullptr, 0, 1, OptionRow::FLAG},
    {PCC_OPT_RIFT_BATCH_BRUTE_MAX, "PCC_RIFT_BATCH_BRUTE_MAX", &Options::rift_batch_brute_max, nullptr, 0, 1073741824, OptionRow::CLOSED},
    {PCC_OPT_SIFT_BATCH_BRUTE_MAX, "PCC_SIFT_BATCH_BRUTE_MAX", &Options::sift_batch_brute_max, nullptr, 0, 1073741824, OptionRow::CLOSED},
    {PCC_OPT_RGB_BATCH_BRUTE_MAX, "PCC_RGB_BATCH_BRUTE_MAX", &Options::rgb_batch_brute_max, nullptr, 0, 1073741824, OptionRow::CLOSED},
    {PCC_OPT_FPFH_LAYOUT, "PCC_FPFH_LAYOUT", &Options::fpfh_layout, nullptr, 0, 1, OptionRow::FLAG},
    {PCC_OPT_FPFH_BATCH_BRUTE_MAX, "PCC_FPFH_BATCH_BRUTE_MAX", &Options::fpfh_batch_brute_max, nullptr, 0, 1073741824, OptionRow::CLOSED},
    {PCC_OPT_VFH_BATCH_BRUTE_MAX, "PCC_VFH_BATCH_BRUTE_MAX", &Options::vfh_batch_brute_max, nullptr, 0, 1073741824, OptionRow::CLOSED},
};
static const OptionRow* option_row(int option) {
    for (const OptionRow& r : g_options)
        if (r.id == option) return &r;
    return nullptr;
}

// PCC_* environment variables give a new handle its defaults; a value outside the option's range is ignored (the
// built-in default stays), exactly what pcc_index_set_option would have refused
void Options::from_env() {
    for (const OptionRow& r : g_options) {
        const char* txt = getenv(r.env);
        if (!txt || !*txt) continue;
        char* end = nullptr;
        const double value = strtod(txt, &end);
        if (end == txt || !r.takes(r.i ? std::trunc(value) : value)) continue;
        if (r.d) this->*r.d = value; else this->*r.i = (int)value;
    }
}

// test hook (pcc_debug_fail_alloc): the n-th device allocation from now on fails as an exhausted hipMalloc would
static std::atomic<int> g_fail_alloc{0};
// test hook (pcc_debug_live_buffers): the blocks DevBuf / HostBuf hold at this moment, process-wide.  Counted where a block is
// really taken or given back, nowhere else: the early return of reserve() -- all a hot call sees -- does not touch them.
static std::atomic<uint64_t> g_live_dev{0}, g_live_pinned{0};

int DevBuf::reserve(size_t bytes) {
    if (bytes <= cap && p) return PCC_OK;
    // (one compare-exchange per armed growth: two threads can never both take the count through zero)
    int armed = g_fail_alloc.load(std::memory_order_relaxed);
    while (armed > 0 && !g_fail_alloc.compare_exchange_weak(armed, armed - 1)) {}
    if (armed == 1) {
        set_error("hipMalloc(%zu) failed: injected by pcc_debug_fail_alloc", bytes);
        return PCC_ERR_NOMEM;  // (the buffer keeps what it had: exactly what a refused growth leaves behind)
    }
    if (bytes == 0) bytes = 256;
    size_t want = bytes + bytes / 8;  // slack so slowly growing batches do not realloc each call
    want = (want + 255) & ~(size_t)255;
    release();
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
        p = nullptr;
        set_error("hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        return PCC_ERR_NOMEM;
    }
    g_live_dev.fetch_add(1, std::memory_order_relaxed);
    cap = want;
    return PCC_OK;
}
void DevBuf::release() {
    if (p) {
        (void)hipFree(p);
        g_live_dev.fetch_sub(1, std::memory_order_relaxed);
    }
    p = nullptr;
    cap = 0;
}
int DevBuf::grow_keep(hipStream_t s, size_t keep, size_t want) {
    if (p && want <= cap) return PCC_OK;
    DevBuf grown;  // (freed by its destructor on every return in front of the move)
    PCC_TRY(grown.reserve(std::max(want, 2 * cap)));
    if (keep && p) {
        PCC_HIP(hipMemcpyAsync(grown.p, p, keep, hipMemcpyDeviceToDevice, s));
        PCC_HIP(hipStreamSynchronize(s));
    }
    *this = std::move(grown);
    return PCC_OK;
}

int HostBuf::reserve(size_t bytes) {
    if (bytes <= cap && p) return PCC_OK;
    if (bytes == 0) bytes = 256;
    size_t want = bytes + bytes / 8;
    want = (want + 4095) & ~(size_t)4095;
    release();
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e != hipSuccess) {
        p = nullptr;
        set_error("hipHostMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        return PCC_ERR_NOMEM;
    }
    g_live_pinned.fetch_add(1, std::memory_order_relaxed);
    cap = want;
    return PCC_OK;
}
void HostBuf::release() {
    if (p) {
        (void)hipHostFree(p);
        g_live_pinned.fetch_sub(1, std::memory_order_relaxed);
    }
    p = nullptr;
    cap = 0;
}

// the handle's pipe, made at the first transfer that needs it
static HostPipe* host_pipe(pcc_index* ix) {
    if (!ix->pipe) ix->pipe = std::make_unique<HostPipe>();
    return ix->pipe.get();
}

// Stage a caller cloud (host or device AoS) as packed float4 on the device.
// host: the raw array (or, for large pageable clouds, its x / y / z alone: host_pipe.hpp) to the device, then the pack kernel.
static int stage_points(pcc_index* ix, const void* pts, size_t n, size_t stride, int mem,
                        DevBuf& raw, float4* packed, const PackExtras& px) {
    const void* src = pts;
    if (mem == PCC_MEM_HOST && n > 0) {
        const size_t bytes = (n - 1) * stride + 12;
        if (ix->opt.host_pipe && bytes >= PIPE_MIN_BYTES && !host_pointer_is_pinned(pts)) {
            // (everything enqueued so far may still be reading `raw`: the chunks are enqueued on the same stream, in order behind it)
            const size_t dst_stride = stride >= 24 ? 12 : stride;
            PCC_TRY(raw.reserve(n * dst_stride + 16));
            ix->small_raw_n = 0;  // (the chunk buffers are the small-call buffers: an indexed cloud's raw records do not survive this)
            PCC_TRY(host_pipe(ix)->upload(ix->stream, static_cast<const char*>(pts), n, stride, raw.as<char>(), dst_stride));
            stride = dst_stride;
        } else if (ix->opt.host_pipe && bytes <= SMALL_DIRECT_BYTES) {
            // SMALL clouds -- the reference's descriptor clouds, 4 ... 18 381 records of 128 bytes, up to 300 calls per comparison
            // (src/comparator.cpp:560-588): a hipMemcpyAsync from pageable memory makes the host wait for a staged copy (~15 us a
            // piece).  Up to SMALL_DIRECT_BYTES the cloud is copied into the handle's pinned buffer instead (slot 0: indexed clouds,
            // 1: query clouds) and the pack kernel reads it from there across the link -- no copy command at all.  (Between 1 and
            // 8 MB the runtime's own staging is as good: 18 381 descriptors 244 us a call against 277 through the pinned buffer.)
            PCC_TRY(host_pipe(ix)->init());
            const int slot = px.indexed_cloud ? 0 : 1;
            PCC_HIP(hipEventSynchronize(ix->pipe->ev[slot]));  // (whoever read this buffer last has finished: nearly always true already)
            memcpy(ix->pipe->buf[slot].p, pts, bytes);
            src = ix->pipe->buf[slot].p;
            if (slot == 0) { ix->small_raw_n = n; ix->small_raw_stride = stride; }  // (the indexed cloud's records stay there: small_tie_replay)
            PCC_TRY(launch_pack(ix->stream, src, n, stride, packed, px));
            PCC_HIP(hipEventRecord(ix->pipe->ev[slot], ix->stream));
            return PCC_OK;
        } else {
            PCC_TRY(raw.reserve(n * stride));
            PCC_HIP(hipMemcpyAsync(raw.p, pts, bytes, hipMemcpyHostToDevice, ix->stream));
        }
        src = raw.p;
    }
    return launch_pack(ix->stream, src, n, stride, packed, px);
}

int check_mem(int mem) {
    if (mem != PCC_MEM_HOST && mem != PCC_MEM_DEVICE) { set_error("bad mem space %d", mem); return PCC_ERR_INVALID; }
    return PCC_OK;
}

int check_points(const void* pts, size_t n, size_t stride, int mem) {
    PCC_TRY(check_mem(mem));
    if (n && !pts) { set_error("null point pointer"); return PCC_ERR_INVALID; }
    if (stride < 12 || stride % 4) { set_error("stride %zu must be a multiple of 4 and >= 12", stride); return PCC_ERR_INVALID; }
    if (n >= (1ull << 31)) { set_error("more than 2^31 points"); return PCC_ERR_UNSUPPORTED; }
    return PCC_OK;
}

// queries -> ix->q_packed (float4, w < 0 marks a non-finite query).  search: the k = 1 search the caller runs next, if it does
int stage_queries(pcc_index* ix, const void* q, size_t nq, size_t stride, int mem, Nn1Call* search) {
    PCC_TRY(ix->q_packed.reserve(nq * sizeof(float4)));
    PCC_TRY(ix->out_packed.reserve(nq * sizeof(unsigned long long)));
    // the pack kernel also zeroes the GRID engine's search counters (clear_search_counters) and presets the result key of
    // every non-finite query to "nothing found"
    PackExtras px;
    px.zero_word = &ix->words()->fb_count;
    px.invalid_keys = ix->out_packed.as<unsigned long long>();
    // clouds that will take the three-level sort: the pack kernel also writes every query's grid cell (4 B), which level 1 of
    // the sort then reads instead of the points (pcc_index::q_cells; valid until the sort has used it)
    ix->q_cells_n = 0;
    if (ix->engine == PCC_ENGINE_GRID && ix->has_grid && nq >= (size_t)ix->opt.sort_mp_min_q) {
        PCC_TRY(ix->q_cells.reserve(nq * sizeof(unsigned int) + 64));
        px.cells = ix->q_cells.as<unsigned int>();
        px.gd = ix->d_grid.as<GridDev>();
        ix->q_cells_n = nq;
    }
    PCC_TRY(stage_points(ix, q, nq, stride, mem, ix->q_raw, ix->q_packed.as<float4>(), px));
    if (search && nq > 0) search->counters_cleared = true;  // (px.zero_word; callers that run no k = 1 search pass none)
    return PCC_OK;
}

// one result into the caller's host array (entry.hpp: finish): large pageable arrays through the host pipe (host_pipe.hpp), else one copy
int deliver(pcc_index* ix, const void* dev, void* user, size_t bytes) {
    if (!user || bytes == 0) return PCC_OK;
    if (ix->opt.host_pipe && bytes >= PIPE_MIN_BYTES && !host_pointer_is_pinned(user)) {
        ix->small_raw_n = 0;  // (as in stage_points)
        return host_pipe(ix)->download(ix->stream, static_cast<const char*>(dev), static_cast<char*>(user), bytes);
    }
    PCC_HIP(hipMemcpyAsync(user, dev, bytes, hipMemcpyDeviceToHost, ix->stream));
    return PCC_OK;
}

// k = 1 search of ix->q_packed[0..nq) into ix->out_packed (u64 per query)
// The small-call form (small.hip): host queries against a small exhaustively searched cloud -- the reference's descriptor
// matching.  PCC_OPT_HOST_PIPE = 0 keeps the separate launches (pack, preset, search, unpack).
static bool small_call(const pcc_index* ix, size_t nq, size_t stride, int mem) {
    return mem == PCC_MEM_HOST && ix->opt.host_pipe && ix->engine == PCC_ENGINE_BRUTE && ix->n_orig <= SMALL_FUSED_REFS && nq > 0 &&
           (nq - 1) * stride + 12 <= SMALL_DIRECT_BYTES && nq * sizeof(float) <= SMALL_RESULT_BYTES;
}
// queries to the pinned buffer, one launch, one wait; the results are in host_a (indices) and host_b (squared distances).
// PCC_TIES_FLANN: the kernel also counts the queries whose minimum is shared by a second reference; only if there are any does the
// tie replay (a kd-tree of FLANN's shape over the indexed cloud, flann_order.hip) run, on the q_packed / out_packed the kernel left
static int small_nn1(pcc_index* ix, const void* q, size_t nq, size_t stride, bool want_idx, bool want_d2) {
    const bool flann = ix->tie_mode == PCC_TIES_FLANN;
    const size_t nblk = (nq + 63) / 64;
    PCC_TRY(ix->q_packed.reserve(nq * sizeof(float4)));
    PCC_TRY(ix->out_packed.reserve(nq * sizeof(unsigned long long)));
    PCC_TRY(ix->host_a.reserve((nq + 2 * nblk) * sizeof(int32_t)));  // (+ per workgroup: tied queries, indices the replay changed)
    PCC_TRY(ix->host_b.reserve(nq * sizeof(float)));
    if (flann) PCC_TRY(ix->tie_buf.reserve(nq + 64));  // (a tie flag per query)
    PCC_TRY(host_pipe(ix)->init());
    PCC_HIP(hipEventSynchronize(ix->pipe->ev[1]));  // (whoever read the query buffer last has finished)
    memcpy(ix->pipe->buf[1].p, q, (nq - 1) * stride + 12);
    ix->q_cells_n = 0;
    ix->stats[0] = 0;
    ix->stats[1] = nq;
    ix->stats_pending = false;
    int32_t* hidx = ix->host_a.as<int32_t>();
    unsigned int* tie_blocks = flann ? reinterpret_cast<unsigned int*>(hidx + nq) : nullptr;
    unsigned char* tie_q = flann ? ix->tie_buf.as<unsigned char>() : nullptr;
    ev_mark(ix, EV_MAIN0);
    PCC_TRY(launch_small_nn1(ix->stream, ix->pipe->buf[1].p, nq, stride, ix->refs.as<float4>(), ix->n_orig, ix->q_packed.as<float4>(),
                             ix->out_packed.as<unsigned long long>(), want_idx || flann ? hidx : nullptr,
                             want_d2 ? ix->host_b.as<float>() : nullptr, tie_blocks, tie_q));
    ev_mark(ix, EV_MAIN1);
    ev_mark(ix, EV_CALL1);
    // (the wait below is also what lets the next call overwrite the pinned query buffer: no event is recorded for it)
    PCC_HIP(hipStreamSynchronize(ix->stream));
    ix->ties_pending = false;  // (whatever the tie order: pcc_index_stats reports THIS search, not a FLANN-order one before it)
    ix->ties_flagged = ix->ties_changed = 0;
    if (!flann) return PCC_OK;
    unsigned int tied = 0;
    for (size_t b = 0; b < nblk; ++b) tied += tie_blocks[b];
    ix->ties_flagged = tied;
    if (tied == 0) return PCC_OK;
    if (ix->small_raw_n == ix->n_orig) {
        unsigned int* changed_blocks = tie_blocks + nblk;
        bool done = false;
        PCC_TRY(small_tie_replay(ix, ix->pipe->buf[0].p, nq, tie_q, hidx, changed_blocks, &done));
        if (done) {
            PCC_HIP(hipStreamSynchronize(ix->stream));
            for (size_t b = 0; b < nblk; ++b) ix->ties_changed += changed_blocks[b];
            return PCC_OK;
        }
    }
    // (the separate launches' replay: its tree build downloads the packed cloud into host_a, which may move -- the indices are
    // unpacked again, all of them, into wherever it is afterwards; the distances in host_b stand)
    PCC_TRY(resolve_ties_flann(ix, ix->q_packed.as<float4>(), ix->out_packed.as<unsigned long long>(), nq));
    PCC_TRY(ix->host_a.reserve((nq + 2 * nblk) * sizeof(int32_t)));
    PCC_TRY(launch_unpack(ix->stream, ix->out_packed.as<unsigned long long>(), nullptr, nq, ix->host_a.as<int32_t>(), nullptr));
    PCC_HIP(hipStreamSynchronize(ix->stream));
    return PCC_OK;
}

// Small host results of a k = 1 search in out_packed: the unpack kernel writes them into pinned memory itself (host_a: indices,
// host_b: squared distances, where small_nn1 leaves them too), no copy command; EV_CALL1, then one wait.  fb_mirror: it also
// mirrors the GRID search's fallback count into the pinned words (pcc_index_stats).
static int unpack_pinned(pcc_index* ix, size_t nq, bool want_idx, bool want_d2, bool fb_mirror) {
    PCC_TRY(ix->host_a.reserve(nq * sizeof(int32_t)));
    PCC_TRY(ix->host_b.reserve(nq * sizeof(float)));
    PCC_TRY(launch_unpack(ix->stream, ix->out_packed.as<unsigned long long>(), nullptr, nq, want_idx ? ix->host_a.as<int32_t>() : nullptr,
                          want_d2 ? ix->host_b.as<float>() : nullptr, fb_mirror ? &ix->words()->fb_count : nullptr,
                          fb_mirror ? &ix->pinned()->fb_mirror : nullptr));
    ev_mark(ix, EV_CALL1);
    PCC_HIP(hipStreamSynchronize(ix->stream));
    return PCC_OK;
}

int nn1_packed(pcc_index* ix, size_t nq, Nn1Call& call) {
    PCC_TRY(ix->out_packed.reserve(nq * sizeof(unsigned long long)));
    auto* out = ix->out_packed.as<unsigned long long>();
    // GRID: every valid query's key is written by the search kernel itself (no 8 MB memset)
    if (ix->engine == PCC_ENGINE_GRID) return grid_nn1(ix, ix->q_packed.as<float4>(), nq, out, call);
    PCC_HIP(hipMemsetAsync(out, 0xff, nq * sizeof(unsigned long long), ix->stream));
    ix->stats[0] = 0;
    ix->stats[1] = nq;
    ix->stats_pending = false;
    ev_mark(ix, EV_MAIN0);
    int st = launch_nn1_brute(ix->stream, ix->refs.as<float4>(), ix->n_orig, ix->q_packed.as<float4>(), nq,
                              out, nullptr, nullptr, 0);
    ev_mark(ix, EV_MAIN1);
    return st;
}

static int resolve_engine(int requested, size_t n) {
    // the grid build costs a few passes over the cloud; below ~4k points one exhaustive
    // sweep is cheaper than building it
    if (requested == PCC_ENGINE_AUTO) return n >= 4096 ? PCC_ENGINE_GRID : PCC_ENGINE_BRUTE;
    return requested;
}

// (re)build the index over a new cloud, fully asynchronous on the index's stream:
// pack (+ per-workgroup bbox / non-finite counts) -> grid sizing ON THE DEVICE -> cell sort.
// Non-finite points stay in place flagged w = -1 (no compaction: position == original index).
// Host-visible facts (n_valid, bbox, grid) arrive through a pinned mirror; sync_info() waits.
static int set_input_impl(pcc_index* ix, const void* pts, size_t n, size_t stride, int mem) {
    ev_next(ix);
    ev_mark(ix, EV_BUILD0);
    PCC_TRY(ix->refs.reserve(n * sizeof(float4)));
    int nblk = 0;
    PCC_TRY(ix->seeds.reserve(((n + PCC_SEED_STRIDE - 1) / PCC_SEED_STRIDE) * sizeof(float4)));  // the pack kernel also emits the seed subset
    PackExtras px;  // the indexed cloud: statistics for the grid, the seed subset
    px.indexed_cloud = true;
    px.blk_stats = ix->blk_stats.as<float>();
    px.n_blocks = &nblk;
    px.seeds = ix->seeds.as<float4>();
    // (small clouds: a launch is what a call costs there, and the fence the fused form pays is nothing over a handful of rows)
    const bool fused = (ix->opt.fuse_params & 1) != 0 || (ix->opt.host_pipe && n <= SMALL_FUSED_POINTS);
    if (fused) PCC_TRY(grid_params_fused(ix, &px.grid));
    PCC_TRY(stage_points(ix, pts, n, stride, mem, ix->q_raw, ix->refs.as<float4>(), px));
    if (!fused) PCC_TRY(grid_params(ix, ix->blk_stats.as<float>(), nblk));
    ix->engine = resolve_engine(ix->engine_requested, n);
    // everything a query needs to be packed and sorted exists from here on (PrepOverlap below)
    if (ix->engine == PCC_ENGINE_GRID && ix->opt.overlap_prep) {
        if (!ix->params_ev) PCC_HIP(hipEventCreateWithFlags(&ix->params_ev, hipEventDisableTiming));
        PCC_HIP(hipEventRecord(ix->params_ev, ix->stream));
        ix->params_ev_set = true;
    }
    if (ix->engine == PCC_ENGINE_GRID) PCC_TRY(grid_build(ix));
    ev_mark(ix, EV_BUILD1);
    return PCC_OK;
}
// on any failure the index is left EMPTY (n_orig = 0: every search then answers PCC_ERR_EMPTY instead of
// launching over buffers a failed reserve() has freed)
int set_input(pcc_index* ix, const void* pts, size_t n, size_t stride, int mem) {
    ix->n_valid = 0;
    ix->has_grid = false;
    ix->flann_valid = false;
    ix->small_raw_n = 0;
    ix->occ_valid = false;
    ix->q_cells_n = 0;  // (cells staged against the grid that is about to be replaced)
    ix->self_rows_k = 0;
    ix->n_orig = n;  // the build steps size their launches from it
    ix->params_ev_set = false;
    ix->edge_fresh = false;
    const int st = set_input_impl(ix, pts, n, stride, mem);
    if (st != PCC_OK) { ix->n_orig = 0; ix->has_grid = false; }
    ix->build_fresh = st == PCC_OK && ix->params_ev_set;  // (until the next entry point: pcc::entered)
    return st;
}

// ---- query staging beside the build (PCC_OPT_OVERLAP_PREP) -----------------------------------------------------------------
// The reference builds its tree and asks at once (src/comparator.cpp:564-577).  Here the build is pack -> grid parameters ->
// three sort levels, and a query needs only the grid parameters to be packed (with its cell) and sorted: two thirds of the
// build and the whole query staging are independent streaming passes.  While an object of this type lives, the handle's
// launches go to side_stream -- which waits for the build's k_grid_params, i.e. for everything enqueued before it as well, but
// not for the build's sort -- and the sort's scratch buffers are swapped for a set of their own; its end joins the side
// stream back into the main one, error or not.  Buffers the staging writes besides (q_packed, q_cells, out_packed, the
// order in scratch_g, the counters in `small`) are touched by no build kernel, and their last readers were enqueued before
// the build.
struct PrepOverlap {
    pcc_index* ix;
    hipStream_t main_stream = nullptr;
    bool on = false;
    // (below ~2M queries the staging is a few launches of 10-20 us each and the second stream's events cost what they hide:
    // 1M x 1M 0.221 / 0.222 / 0.226 ms without, 0.225 with; 10M x 10M 1.331 / 1.334 / 1.319 -> 1.308 / 1.303 / 1.301)
    static constexpr size_t min_queries = 2000000;
    // Only on the library's OWN stream: a caller that has handed its stream over (pcc_index_set_stream) may have enqueued the
    // kernel that produces the queries on it between the build and this search -- "enqueued on the index's stream" is the
    // ordering pcc_nn.h promises -- and the side stream, which waits for the build's k_grid_params only, would read them early.
    static bool wanted(const pcc_index* ix, size_t nq) {
        return ix->opt.overlap_prep && ix->stream == ix->own_stream && ix->after_build && ix->params_ev_set && ix->engine == PCC_ENGINE_GRID && ix->has_grid &&
               (nq >= min_queries || ix->opt.overlap_prep == 2);  // (2: whatever the size -- tests, fuzz)
    }
    explicit PrepOverlap(pcc_index* i) : ix(i) {}
    void swap_scratch() {  // (std::swap moves: the two owners exchange their blocks, nothing is copied or freed)
        std::swap(ix->scratch_a, ix->side.a);
        std::swap(ix->scratch_b, ix->side.b);
        std::swap(ix->scratch_c, ix->side.c);
        std::swap(ix->scratch_e, ix->side.e);
        std::swap(ix->mp_a, ix->side.mp_a);
        std::swap(ix->mp_b, ix->side.mp_b);
        std::swap(ix->mp_c, ix->side.mp_c);
        std::swap(ix->scan_flags, ix->side.scan_flags);
        std::swap(ix->scan_epoch, ix->side.scan_epoch);
    }
    int begin() {
        if (!ix->side_stream) PCC_HIP(hipStreamCreateWithFlags(&ix->side_stream, hipStreamNonBlocking));
        if (!ix->side_ev) PCC_HIP(hipEventCreateWithFlags(&ix->side_ev, hipEventDisableTiming));
        PCC_HIP(hipStreamWaitEvent(ix->side_stream, ix->params_ev, 0));
        if (ix->edge_fresh) PCC_HIP(hipStreamWaitEvent(ix->side_stream, ix->edge_ev, 0));  // (the caller's producer stream)
        main_stream = ix->stream;
        ix->stream = ix->side_stream;
        swap_scratch();
        on = true;
        return PCC_OK;
    }
    int end() {
        if (!on) return PCC_OK;
        on = false;
        swap_scratch();
        ix->stream = main_stream;
        PCC_HIP(hipEventRecord(ix->side_ev, ix->side_stream));
        PCC_HIP(hipStreamWaitEvent(main_stream, ix->side_ev, 0));
        return PCC_OK;
    }
    ~PrepOverlap() { (void)end(); }
};

int ensure_grid(pcc_index* ix) {
    if (ix->n_orig == 0) { set_error("index is empty"); return PCC_ERR_EMPTY; }
    if (!ix->has_grid) PCC_TRY(grid_build(ix));
    return PCC_OK;
}

// shared by pcc_index_create and pcc_index_clone_to_device: an empty handle on `device`
int make_handle(int device, int engine, pcc_index** out) {
    pcc_index* ix = new pcc_index();
    ix->device = device;
    ix->opt.from_env();
    DeviceGuard g(device);
    int st = PCC_OK;
    auto fail = [&](int s) { pcc_index_destroy(ix); return s; };
    if (!g.ok) { set_error("hipSetDevice(%d) failed", device); return fail(PCC_ERR_DEVICE); }
    if (hipStreamCreateWithFlags(&ix->own_stream, hipStreamNonBlocking) != hipSuccess) { set_error("hipStreamCreate failed"); return fail(PCC_ERR_DEVICE); }
    ix->stream = ix->own_stream;
    if (ix->pinned_buf.reserve(sizeof(PinnedWords)) != PCC_OK) { set_error("hipHostMalloc failed"); return fail(PCC_ERR_DEVICE); }
    if ((st = ix->words_buf.reserve(sizeof(DevWords))) != PCC_OK) return fail(st);
    if (hipMemset(ix->words_buf.p, 0, sizeof(DevWords)) != hipSuccess) { set_error("hipMemset failed"); return fail(PCC_ERR_DEVICE); }  // (the ticket words start at 0)
    if ((st = ix->blk_stats.reserve(PACK_MAX_BLOCKS * 8 * sizeof(float))) != PCC_OK) return fail(st);
    ix->engine_requested = engine;
    ix->engine = engine;
    memset(ix->pinned(), 0, sizeof(PinnedWords));
    if (ix->h_grid_buf.reserve(sizeof(GridDev)) != PCC_OK) { set_error("hipHostMalloc failed"); return fail(PCC_ERR_DEVICE); }
    memset(ix->h_grid(), 0, sizeof(GridDev));
    *out = ix;
    return PCC_OK;
}

}  // namespace pcc

// The order of a handle's end (pcc_index_destroy has selected its device and waited for its stream):
pcc_index::~pcc_index() {
    // 1. what the features keep: their work handles wait on their own streams, and go before this handle's streams and events
    for (auto& s : scratch) s.reset();
    pipe.reset();
    // 2. the streams and events
    for (int sl = 0; sl < PCC_EV_SLOTS; ++sl)
        for (int k = 0; k < PCC_EV_KINDS; ++k)
            if (ev[sl][k]) (void)hipEventDestroy(ev[sl][k]);
    if (edge_ev) (void)hipEventDestroy(edge_ev);
    if (params_ev) (void)hipEventDestroy(params_ev);
    if (side_ev) (void)hipEventDestroy(side_ev);
    if (side_stream) { (void)hipStreamSynchronize(side_stream); (void)hipStreamDestroy(side_stream); }
    if (own_stream) (void)hipStreamDestroy(own_stream);
    // 3. the handle's own buffers: every DevBuf and HostBuf member frees itself behind this body
}

using namespace pcc;
extern "C" {
int pcc_version(void) { return PCC_VERSION; }
const char* pcc_last_error(void) { return g_err.c_str(); }

int pcc_device_count(int* count) {
    if (!count) { set_error("null count"); return PCC_ERR_INVALID; }
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *count = 0; set_error("hipGetDeviceCount: %s", hipGetErrorString(e)); return PCC_ERR_DEVICE; }
    *count = c;
    return PCC_OK;
}

int pcc_index_destroy(pcc_index* ix) {
    if (!ix) return PCC_OK;
    DeviceGuard g(ix->device);
    if (ix->stream) (void)hipStreamSynchronize(ix->stream);
    delete ix;
    return PCC_OK;
}

int pcc_index_create(const void* pts, size_t n, size_t stride, int dim, int mem, int device, int engine,
                     pcc_index** out) {
    if (!out) { set_error("null out"); return PCC_ERR_INVALID; }
    *out = nullptr;
    if (dim != 3) { set_error("dim %d unsupported: every hot call site of the reference searches 3 floats", dim); return PCC_ERR_UNSUPPORTED; }
    if (engine < PCC_ENGINE_AUTO || engine > PCC_ENGINE_GRID) { set_error("bad engine %d", engine); return PCC_ERR_INVALID; }
    PCC_TRY(check_points(pts, n, stride, mem));
    if (n == 0) { set_error("Cannot create a KDTree with an empty input cloud"); return PCC_ERR_EMPTY; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available (libpcc_nn has no CPU path)"); return PCC_ERR_DEVICE; }
    if (device < 0 || device >= ndev) { set_error("device %d out of range (%d present)", device, ndev); return PCC_ERR_INVALID; }
    pcc_index* ix = nullptr;
    PCC_TRY(make_handle(device, engine, &ix));
    DeviceGuard g(device);
    int st = PCC_OK;
    auto fail = [&](int s) { pcc_index_destroy(ix); return s; };
    if ((st = set_input(ix, pts, n, stride, mem)) != PCC_OK) return fail(st);
    if ((st = sync_info(ix)) != PCC_OK) return fail(st);
    if (hipStreamSynchronize(ix->stream) != hipSuccess) { set_error("index build failed: %s", hipGetErrorString(hipGetLastError())); return fail(PCC_ERR_DEVICE); }
    if (ix->n_valid == 0) { set_error("Cannot create a KDTree with an empty input cloud (all %zu points non-finite)", n); return fail(PCC_ERR_EMPTY); }
    *out = ix;
    return PCC_OK;
}

int pcc_index_clone_to_device(pcc_index* src, int device, pcc_index** out) {
    return pcc_index_clone_to_devices(src, &device, 1, out);
}

int pcc_index_clone_to_devices(pcc_index* src, const int* devices, int count, pcc_index** out) {
    if (!out || !devices || count < 0) { set_error("null argument"); return PCC_ERR_INVALID; }
    for (int k = 0; k < count; ++k) out[k] = nullptr;
    if (!src) { set_error("null index"); return PCC_ERR_INVALID; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available (libpcc_nn has no CPU path)"); return PCC_ERR_DEVICE; }
    for (int k = 0; k < count; ++k)
        if (devices[k] < 0 || devices[k] >= ndev) { set_error("device %d out of range (%d present)", devices[k], ndev); return PCC_ERR_INVALID; }
    if (count == 0) return PCC_OK;
    // `src` stays locked until every peer copy has landed: a concurrent pcc_index_set_input on it may free or rewrite
    // the packed cloud the copies read
    HandleLock lock(src->mu);  // (no call ON src: it keeps its "the build was the last thing enqueued")
    {
        DeviceGuard g(src->device);
        if (!g.ok) { set_error("hipSetDevice(%d) failed", src->device); return PCC_ERR_DEVICE; }
        if (src->n_orig == 0) { set_error("index is empty"); return PCC_ERR_EMPTY; }
        PCC_HIP(hipStreamSynchronize(src->stream));  // the packed cloud is complete
    }
    const size_t n = src->n_orig;
    // One host thread per clone: handle creation (stream, pinned blocks, device allocations: ~3 ms of driver calls
    // each -- more than the copy itself), the peer copy on the clone's own stream over its own xGMI link, the build
    // behind it, the join.  Nothing of one clone waits for another: the copies to the other GPUs of a node and their
    // builds all overlap (one after the other: 7 x (3 ms + 160 MB + build) at 10M points).
    std::vector<int> status((size_t)count, PCC_OK);
    std::vector<std::string> errors((size_t)count);
    auto one = [&](int k) {
        auto run = [&]() -> int {
            pcc_index* ix = nullptr;
            PCC_TRY(make_handle(devices[k], src->engine_requested, &ix));
            out[k] = ix;
            ix->opt = src->opt;
            ix->tie_mode = src->tie_mode;
            DeviceGuard g(devices[k]);
            PCC_TRY(ix->icp_src.reserve(n * sizeof(float4)));
            if (hipMemcpyPeerAsync(ix->icp_src.p, devices[k], src->refs.p, src->device, n * sizeof(float4), ix->stream) != hipSuccess) {
                set_error("hipMemcpyPeerAsync %d -> %d failed: %s", src->device, devices[k], hipGetErrorString(hipGetLastError()));
                return PCC_ERR_DEVICE;
            }
            // (non-finite points get their NaN back so that the build sees what the original upload saw)
            PCC_TRY(launch_nanify(ix->stream, ix->icp_src.as<float4>(), n));
            PCC_TRY(set_input(ix, ix->icp_src.p, n, sizeof(float4), PCC_MEM_DEVICE));
            PCC_TRY(sync_info(ix));
            if (hipStreamSynchronize(ix->stream) != hipSuccess) { set_error("index build failed: %s", hipGetErrorString(hipGetLastError())); return PCC_ERR_DEVICE; }
            return PCC_OK;
        };
        status[(size_t)k] = run();
        if (status[(size_t)k] != PCC_OK) errors[(size_t)k] = g_err;  // (the message is thread-local)
    };
    if (count == 1) {
        one(0);
    } else {
        std::vector<std::thread> th;
        for (int k = 0; k < count; ++k) th.emplace_back(one, k);
        for (std::thread& t : th) t.join();
    }
    for (int k = 0; k < count; ++k)
        if (status[(size_t)k] != PCC_OK) {
            const int bad = status[(size_t)k];
            const std::string msg = errors[(size_t)k];
            for (int j = 0; j < count; ++j) { if (out[j]) pcc_index_destroy(out[j]); out[j] = nullptr; }
            set_error("%s", msg.c_str());
            return bad;
        }
    return PCC_OK;
}

int pcc_index_set_input(pcc_index* ix, const void* pts, size_t n, size_t stride, int dim, int mem) {
    PCC_ENTER(ix);
    if (dim != 3) { set_error("dim %d unsupported", dim); return PCC_ERR_UNSUPPORTED; }
    PCC_TRY(check_points(pts, n, stride, mem));
    if (n == 0) { ix->n_valid = 0; ix->n_orig = 0; set_error("Cannot create a KDTree with an empty input cloud"); return PCC_ERR_EMPTY; }
    // asynchronous: a cloud without any finite point is reported by pcc_index_size (0) and by
    // searches returning idx = -1, not by this call
    return set_input(ix, pts, n, stride, mem);
}

int pcc_index_enable_timing(pcc_index* ix, int on) {
    PCC_ENTER(ix);
    PCC_NOTHING_ENQUEUED(ix);
    PCC_HIP(hipStreamSynchronize(ix->stream));
    if (on) {
        for (int sl = 0; sl < PCC_EV_SLOTS; ++sl)
            for (int k = 0; k < PCC_EV_KINDS; ++k)
                if (!ix->ev[sl][k]) PCC_HIP(hipEventCreate(&ix->ev[sl][k]));
    }
    for (int sl = 0; sl < PCC_EV_SLOTS; ++sl)
        for (int k = 0; k < PCC_EV_KINDS; ++k) ix->ev_rec[sl][k] = false;
    ix->ev_slot = 0;
    ix->timing = on < 0 ? 0 : (on > 2 ? 2 : on);
    return PCC_OK;
}

int pcc_index_timing(pcc_index* ix, float ms[8]) {
    PCC_ENTER(ix);
    PCC_NOTHING_ENQUEUED(ix);
    if (!ms) { set_error("null ms"); return PCC_ERR_INVALID; }
    PCC_HIP(hipStreamSynchronize(ix->stream));
    const int pairs[5][2] = {{EV_MAIN0, EV_MAIN1}, {EV_FB0, EV_FB1}, {EV_CALL0, EV_CALL1}, {EV_BUILD0, EV_BUILD1}, {EV_SORT0, EV_SORT1}};
    for (int i = 0; i < 8; ++i) ms[i] = 0.f;
    for (int i = 0; i < 5; ++i) {
        double sum = 0;
        int cnt = 0;
        for (int sl = 0; sl < PCC_EV_SLOTS; ++sl) {
            int a = pairs[i][0], b = pairs[i][1];
            if (ix->ev[sl][a] && ix->ev[sl][b] && ix->ev_rec[sl][a] && ix->ev_rec[sl][b]) {
                float t = 0.f;
                if (hipEventElapsedTime(&t, ix->ev[sl][a], ix->ev[sl][b]) == hipSuccess) { sum += t; ++cnt; }
            }
        }
        if (cnt) ms[i] = (float)(sum / cnt);
        if (i == 0) ms[7] = (float)cnt;
    }
    return PCC_OK;
}

int pcc_index_size(const pcc_index* cix, size_t* n_valid) {
    if (!cix || !n_valid) { set_error("null argument"); return PCC_ERR_INVALID; }
    pcc_index* ix = const_cast<pcc_index*>(cix);  // may have to wait for the asynchronous build
    PCC_ENTER(ix);
    PCC_NOTHING_ENQUEUED(ix);
    PCC_TRY(sync_info(ix));
    *n_valid = ix->n_valid;
    return PCC_OK;
}
int pcc_index_set_stream(pcc_index* ix, void* s) {
    PCC_ENTER(ix);
    PCC_HIP(hipStreamSynchronize(ix->stream));
    ix->stream = s ? static_cast<hipStream_t>(s) : ix->own_stream;
    return PCC_OK;
}
// order the index's stream against another stream of the same device without blocking the host
static int stream_edge(pcc_index* ix, hipStream_t from, hipStream_t to) {
    if (from == to) return PCC_OK;
    if (!ix->edge_ev) PCC_HIP(hipEventCreateWithFlags(&ix->edge_ev, hipEventDisableTiming));
    PCC_HIP(hipEventRecord(ix->edge_ev, from));
    PCC_HIP(hipStreamWaitEvent(to, ix->edge_ev, 0));
    return PCC_OK;
}
int pcc_index_wait_stream(pcc_index* ix, void* producer) {
    PCC_ENTER(ix);
    PCC_TRY(stream_edge(ix, static_cast<hipStream_t>(producer), ix->stream));
    // (a search staged beside the build -- PrepOverlap -- must honour this edge on its side stream as well; edge_ev is the
    // producer's mark until the next edge, and one such edge is remembered)
    if (ix->after_build && !ix->edge_fresh && static_cast<hipStream_t>(producer) != ix->stream) {
        ix->build_fresh = true;
        ix->edge_fresh = true;
    }
    return PCC_OK;
}
int pcc_stream_wait_index(pcc_index* ix, void* consumer) {
    PCC_ENTER(ix);
    PCC_NOTHING_ENQUEUED(ix);
    return stream_edge(ix, ix->stream, static_cast<hipStream_t>(consumer));
}
int pcc_index_sync(pcc_index* ix) {
    PCC_ENTER(ix);
    PCC_NOTHING_ENQUEUED(ix);
    PCC_HIP(hipStreamSynchronize(ix->stream));
    return PCC_OK;
}
int pcc_index_engine(const pcc_index* ix, int* engine) {
    if (!ix || !engine) { set_error("null argument"); return PCC_ERR_INVALID; }
    *engine = ix->engine;
    return PCC_OK;
}
int pcc_index_set_engine(pcc_index* ix, int engine) {
    PCC_ENTER(ix);
    if (engine < PCC_ENGINE_AUTO || engine > PCC_ENGINE_GRID) { set_error("bad engine %d", engine); return PCC_ERR_INVALID; }
    ix->engine_requested = engine;
    engine = resolve_engine(engine, ix->n_orig);
    if (engine == PCC_ENGINE_GRID && !ix->has_grid && ix->n_orig) PCC_TRY(grid_build(ix));
    ix->engine = engine;
    return PCC_OK;
}
int pcc_index_set_tie_order(pcc_index* ix, int ties) {
    PCC_ENTER(ix);
    PCC_NOTHING_ENQUEUED(ix);
    if (ties != PCC_TIES_LOWEST_INDEX && ties != PCC_TIES_FLANN) { set_error("bad tie order %d", ties); return PCC_ERR_INVALID; }
    ix->tie_mode = ties;
    return PCC_OK;
}
int pcc_index_set_option(pcc_index* ix, int option, double value) {
    PCC_ENTER(ix);
    PCC_NOTHING_ENQUEUED(ix);
    const OptionRow* r = option_row(option);
    if (!r) { set_error("unknown option %d", option); return PCC_ERR_INVALID; }
    if (!std::isfinite(value)) { set_error("option %d: non-finite value", option); return PCC_ERR_INVALID; }
    if (!r->takes(value)) { set_error("option %d: value %g out of range", option, value); return PCC_ERR_INVALID; }
    if (r->d) ix->opt.*r->d = value; else ix->opt.*r->i = (int)value;
    if (option == PCC_OPT_FLANN_SPLIT) ix->flann_valid = false;  // the replayed tree has to be rebuilt with the other rule
    return PCC_OK;
}
int pcc_index_get_option(pcc_index* ix, int option, double* value) {
    PCC_ENTER(ix);
    PCC_NOTHING_ENQUEUED(ix);
    if (!value) { set_error("null value"); return PCC_ERR_INVALID; }
    const OptionRow* r = option_row(option);
    if (!r) { set_error("unknown option %d", option); return PCC_ERR_INVALID; }
    *value = r->d ? ix->opt.*r->d : (double)(ix->opt.*r->i);
    return PCC_OK;
}
int pcc_debug_fail_alloc(int nth) {
    g_fail_alloc.store(nth > 0 ? nth : 0);
    return PCC_OK;
}
int pcc_debug_live_buffers(uint64_t live[2]) {
    if (!live) { set_error("null argument"); return PCC_ERR_INVALID; }
    live[0] = g_live_dev.load(std::memory_order_relaxed);
    live[1] = g_live_pinned.load(std::memory_order_relaxed);
    return PCC_OK;
}
int pcc_counts_pairs(void) {
#ifdef PCC_COUNT_PAIRS
    return 1;
#else
    return 0;
#endif
}
int pcc_index_stats(const pcc_index* cix, uint64_t stats[8]) {
    if (!cix || !stats) { set_error("null argument"); return PCC_ERR_INVALID; }
    pcc_index* ix = const_cast<pcc_index*>(cix);
    PCC_ENTER(ix);
    PCC_TRY(sync_info(ix));
#ifdef PCC_COUNT_PAIRS
    // profiling build: distances evaluated by the pruned kernels (process-wide, every handle) since the previous call
    PCC_HIP(hipStreamSynchronize(ix->stream));
    ix->stats[4] = pairs_take_grid() + pairs_take_knn() + pairs_take_cluster() + pairs_take_flann() + pairs_take_rift_batch() + pairs_take_rgb_batch();
#endif
    if (ix->stats_pending) {
        PCC_HIP(hipStreamSynchronize(ix->stream));
        ix->stats_pending = false;
        ix->stats[1] = ix->pinned()->fb_mirror;
        ix->stats[0] = ix->last_nq - ix->stats[1];
    }
    if (ix->ties_pending) {  // the sharded counters of the last search in FLANN mode
        unsigned int h[PCC_TIE_SHARDS * PCC_OPEN_CTR_STRIDE];
        PCC_HIP(hipMemcpyAsync(h, ix->words()->tie, sizeof(h), hipMemcpyDeviceToHost, ix->stream));
        PCC_HIP(hipStreamSynchronize(ix->stream));
        ix->ties_flagged = ix->ties_changed = 0;
        for (int sh = 0; sh < PCC_TIE_SHARDS; ++sh) {
            ix->ties_flagged += h[sh * PCC_OPEN_CTR_STRIDE];
            ix->ties_changed += h[sh * PCC_OPEN_CTR_STRIDE + 1];
        }
        ix->ties_pending = false;
    }
    if (ix->open_pending) {  // lanes the 3x3x3 cube left open in the last listed k = 1 search (sharded counters)
        unsigned int h[PCC_OPEN_SHARDS * PCC_OPEN_CTR_STRIDE];
        PCC_HIP(hipMemcpyAsync(h, ix->words()->open, sizeof(h), hipMemcpyDeviceToHost, ix->stream));
        PCC_HIP(hipStreamSynchronize(ix->stream));
        ix->stats[7] = 0;
        for (int sh = 0; sh < PCC_OPEN_SHARDS; ++sh) ix->stats[7] += h[sh * PCC_OPEN_CTR_STRIDE];
        ix->open_pending = false;
    }
    ix->stats[5] = ix->ties_flagged;
    ix->stats[6] = ix->ties_changed;
    memcpy(stats, ix->stats, sizeof(ix->stats));
    return PCC_OK;
}

int pcc_nn1(pcc_index* ix, const void* q, size_t nq, size_t stride, int mem, int32_t* idx, float* d2) {
    PCC_ENTER(ix);
    PCC_TRY(check_points(q, nq, stride, mem));
    if (nq == 0) return PCC_OK;
    if (ix->n_orig == 0) { set_error("index is empty"); return PCC_ERR_EMPTY; }
    ev_next(ix);
    ev_mark(ix, EV_CALL0);
    if (small_call(ix, nq, stride, mem)) {
        PCC_TRY(small_nn1(ix, q, nq, stride, idx != nullptr, d2 != nullptr));
    } else {
        Nn1Call call;
        {
            PrepOverlap beside(ix);
            if (PrepOverlap::wanted(ix, nq)) PCC_TRY(beside.begin());
            PCC_TRY(stage_queries(ix, q, nq, stride, mem, &call));
            if (beside.on) {  // (the search is given the order sorted here, beside the build)
                PCC_TRY(grid_sort_queries(ix, ix->q_packed.as<float4>(), nq, &call.order, &call.n_sorted));
                call.order_given = true; call.order_nq = nq;
                PCC_TRY(beside.end());
            }
        }
        PCC_TRY(nn1_packed(ix, nq, call));
        if (ix->tie_mode == PCC_TIES_FLANN)
            PCC_TRY(resolve_ties_flann(ix, ix->q_packed.as<float4>(), ix->out_packed.as<unsigned long long>(), nq, mem == PCC_MEM_HOST));
        // small host results: straight into pinned memory (unpack_pinned)
        const bool direct = mem == PCC_MEM_HOST && ix->opt.host_pipe && nq * sizeof(float) <= SMALL_RESULT_BYTES;
        if (!direct) {
            Out<int32_t> ri;
            Out<float> rd;
            PCC_TRY(ri.stage(idx, nq, mem, ix->out_idx));
            PCC_TRY(rd.stage(d2, nq, mem, ix->out_d2));
            PCC_TRY(launch_unpack(ix->stream, ix->out_packed.as<unsigned long long>(), nullptr, nq, ri.dev, rd.dev,
                                  &ix->words()->fb_count, &ix->pinned()->fb_mirror));
            ev_mark(ix, EV_CALL1);
            return finish(ix, mem, ri, rd);
        }
        PCC_TRY(unpack_pinned(ix, nq, idx != nullptr, d2 != nullptr, true));
    }
    // (small_nn1 and unpack_pinned leave the results in host_a / host_b)
    if (idx) memcpy(idx, ix->host_a.p, nq * sizeof(int32_t));
    if (d2) memcpy(d2, ix->host_b.p, nq * sizeof(float));
    return PCC_OK;
}

int pcc_knn(pcc_index* ix, const void* q, size_t nq, size_t stride, int mem, int k, int32_t* idx, float* d2) {
    PCC_ENTER(ix);
    PCC_TRY(check_points(q, nq, stride, mem));
    if (k < 1 || k > PCC_KNN_MAX_K) { set_error("k=%d outside [1, %d]", k, PCC_KNN_MAX_K); return PCC_ERR_UNSUPPORTED; }
    if (nq == 0) return PCC_OK;
    PCC_TRY(ensure_grid(ix));
    ev_next(ix);
    ev_mark(ix, EV_CALL0);
    PCC_TRY(stage_queries(ix, q, nq, stride, mem));
    Out<int32_t> ri;
    Out<float> rd;
    PCC_TRY(ri.stage(idx, nq * (size_t)k, mem, ix->out_idx));
    PCC_TRY(rd.stage(d2, nq * (size_t)k, mem, ix->out_d2));
    if (grid_knn_delivers(k)) {
        // the search writes indices and distances itself (no key array, no unpack pass)
        PCC_TRY(grid_knn(ix, ix->q_packed.as<float4>(), nq, k, nullptr, ri.dev, rd.dev));
    } else {
        PCC_TRY(ix->out_packed.reserve(nq * (size_t)k * sizeof(unsigned long long)));
        auto* keys = ix->out_packed.as<unsigned long long>();
        PCC_TRY(grid_knn(ix, ix->q_packed.as<float4>(), nq, k, keys));
        // rows of invalid queries were never touched (all ~0) and unpack to -1 / +inf
        PCC_TRY(launch_unpack(ix->stream, keys, nullptr, nq * (size_t)k, ri.dev, rd.dev));
    }
    ev_mark(ix, EV_CALL1);
    return finish(ix, mem, ri, rd);
}

int pcc_radius_count(pcc_index* ix, const void* q, size_t nq, size_t stride, int mem, double radius, int32_t* counts) {
    return pcc_radius_count_max(ix, q, nq, stride, mem, radius, 0u, counts);
}
// radiusSearch's max_nn, decided under the handle's lock for count and fill alike: "all" when it is 0 or reaches the number of
// FINITE indexed points (PCL's total_nr_points_); beyond PCC_KNN_MAX_K both calls refuse (the rows come from the k-NN kernels)
static int radius_max_mode(pcc_index* ix, unsigned int max_nn, bool* all) {
    PCC_TRY(sync_info(ix));
    *all = max_nn == 0 || (size_t)max_nn >= ix->n_valid;
    if (!*all && max_nn > (unsigned int)PCC_KNN_MAX_K) { set_error("max_nn=%u beyond %d", max_nn, PCC_KNN_MAX_K); return PCC_ERR_UNSUPPORTED; }
    return PCC_OK;
}
static int radius_fill_impl(pcc_index* ix, const void* q, size_t nq, size_t stride, int mem, double radius, int sorted,
                            const int64_t* offsets, int32_t* idx, float* d2);

int pcc_radius_count_max(pcc_index* ix, const void* q, size_t nq, size_t stride, int mem, double radius, unsigned int max_nn,
                         int32_t* counts) {
    PCC_ENTER(ix);
    PCC_TRY(check_points(q, nq, stride, mem));
    if (!counts) { set_error("null counts"); return PCC_ERR_INVALID; }
    if (!(radius >= 0)) { set_error("bad radius"); return PCC_ERR_INVALID; }
    if (nq == 0) return PCC_OK;
    PCC_TRY(ensure_grid(ix));
    bool max_nn_is_all = true;
    PCC_TRY(radius_max_mode(ix, max_nn, &max_nn_is_all));  // (the same decision, and the same refusal, as the fill's)
    ev_next(ix);
    ev_mark(ix, EV_CALL0);
    PCC_TRY(stage_queries(ix, q, nq, stride, mem));
    Out<int32_t> rc;
    PCC_TRY(rc.stage(counts, nq, mem, ix->out_idx));
    PCC_HIP(hipMemsetAsync(rc.dev, 0, nq * sizeof(int32_t), ix->stream));
    PCC_TRY(grid_radius(ix, ix->q_packed.as<float4>(), nq, (float)radius, radius2(radius), rc.dev, nullptr, nullptr, 0));
    // KdTreeFLANN::radiusSearch(..., max_nn): 0 or anything from the cloud's size on means "all" -- the size PCL compares
    // with is total_nr_points_, the FINITE points --; else FLANN keeps the max_nn nearest within the radius
    if (!max_nn_is_all) PCC_TRY(launch_clamp_counts(ix->stream, rc.dev, nq, (int32_t)max_nn));
    ev_mark(ix, EV_CALL1);
    return finish(ix, mem, rc);
}

int pcc_radius_fill_max(pcc_index* ix, const void* q, size_t nq, size_t stride, int mem, double radius, int sorted, unsigned int max_nn,
                        const int64_t* offsets, int32_t* idx, float* d2) {
    // the max_nn NEAREST within the radius, ascending (FLANN's KNNRadiusResultSet, whatever `sorted` says): the k-NN rows
    // with k = max_nn, cut at the radius.  Unused by the reference's own call sites (src/segmentation.cpp:125-131 passes 0):
    // correctness first, no kernel of its own
    PCC_ENTER(ix);
    PCC_TRY(check_points(q, nq, stride, mem));
    if (!offsets) { set_error("null offsets"); return PCC_ERR_INVALID; }
    if (!(radius >= 0)) { set_error("bad radius"); return PCC_ERR_INVALID; }
    if (nq == 0) return PCC_OK;
    PCC_TRY(ensure_grid(ix));
    bool max_nn_is_all = true;
    PCC_TRY(radius_max_mode(ix, max_nn, &max_nn_is_all));
    if (max_nn_is_all) return radius_fill_impl(ix, q, nq, stride, mem, radius, sorted, offsets, idx, d2);
    PCC_TRY(stage_queries(ix, q, nq, stride, mem));
    const int K = (int)max_nn;
    int64_t total = 0;
    const int64_t* doff = nullptr;
    PCC_TRY(stage_offsets(ix, offsets, nq, mem, &doff, &total));
    if (total == 0) return PCC_OK;
    const bool rows = grid_knn_delivers(K);
    unsigned long long* keys = nullptr;
    int32_t* ridx = nullptr;
    float* rd2 = nullptr;
    if (rows) {
        // (buffers of their own: the query sort inside grid_knn re-reserves scratch_e as its pair buffer, and a reserve
        // that grows FREES the old block -- with the rows in scratch_e a fresh handle, nq = 1 or max_nn = 1 left the k-NN
        // kernels writing into freed memory)
        PCC_TRY(ix->rows_idx.reserve(nq * (size_t)K * sizeof(int32_t)));
        PCC_TRY(ix->rows_d2.reserve(nq * (size_t)K * sizeof(float)));
        ridx = ix->rows_idx.as<int32_t>();
        rd2 = ix->rows_d2.as<float>();
        PCC_TRY(grid_knn(ix, ix->q_packed.as<float4>(), nq, K, nullptr, ridx, rd2));
    } else {
        PCC_TRY(ix->out_packed.reserve(nq * (size_t)K * sizeof(unsigned long long)));
        keys = ix->out_packed.as<unsigned long long>();
        PCC_TRY(grid_knn(ix, ix->q_packed.as<float4>(), nq, K, keys));
    }
    Out<int32_t> ri;
    Out<float> rd;
    PCC_TRY(ri.stage(idx, (size_t)total, mem, ix->out_idx));
    PCC_TRY(rd.stage(d2, (size_t)total, mem, ix->out_d2));
    PCC_TRY(launch_knn_rows_to_csr(ix->stream, keys, ridx, rd2, K, radius2(radius), doff, nq, ri.dev, rd.dev));
    return finish(ix, mem, ri, rd);
}

int pcc_radius_fill(pcc_index* ix, const void* q, size_t nq, size_t stride, int mem, double radius, int sorted,
                    const int64_t* offsets, int32_t* idx, float* d2) {
    PCC_ENTER(ix);
    return radius_fill_impl(ix, q, nq, stride, mem, radius, sorted, offsets, idx, d2);
}
// (the caller holds the handle's lock)
static int radius_fill_impl(pcc_index* ix, const void* q, size_t nq, size_t stride, int mem, double radius, int sorted,
                            const int64_t* offsets, int32_t* idx, float* d2) {
    PCC_TRY(check_points(q, nq, stride, mem));
    if (!offsets) { set_error("null offsets"); return PCC_ERR_INVALID; }
    if (nq == 0) return PCC_OK;
    PCC_TRY(ensure_grid(ix));
    ev_next(ix);
    ev_mark(ix, EV_CALL0);
    PCC_TRY(stage_queries(ix, q, nq, stride, mem));
    int64_t total = 0;
    const int64_t* doff = nullptr;
    PCC_TRY(stage_offsets(ix, offsets, nq, mem, &doff, &total));
    if (total == 0) return PCC_OK;
    PCC_TRY(ix->out_packed.reserve((size_t)total * sizeof(unsigned long long)));
    auto* keys = ix->out_packed.as<unsigned long long>();
    Out<int32_t> ri;
    Out<float> rd;
    PCC_TRY(ri.stage(idx, (size_t)total, mem, ix->out_idx));
    PCC_TRY(rd.stage(d2, (size_t)total, mem, ix->out_d2));
    // rows of 24 neighbours and more on average: the fill delivers index and distance itself (sorted in registers, no
    // key array in between); otherwise keys -> sort -> unpack.  (Slots a fill does not reach read "nothing found".)
    const bool wave_fill = (size_t)total >= RAD_WAVE_MEAN * nq && (ri.dev || rd.dev);
    if (!wave_fill) PCC_HIP(hipMemsetAsync(keys, 0xff, (size_t)total * sizeof(unsigned long long), ix->stream));
    bool delivered = false;
    PCC_TRY(grid_radius(ix, ix->q_packed.as<float4>(), nq, (float)radius, radius2(radius), nullptr, doff, keys, sorted, (size_t)total,
                        ri.dev, rd.dev, &delivered));
    if (!delivered) PCC_TRY(launch_unpack(ix->stream, keys, nullptr, (size_t)total, ri.dev, rd.dev));
    ev_mark(ix, EV_CALL1);
    return finish(ix, mem, ri, rd);
}

int pcc_first_within(pcc_index* ix, const void* q, size_t nq, size_t stride, int mem, double radius, int32_t* idx) {
    PCC_ENTER(ix);
    PCC_TRY(check_points(q, nq, stride, mem));
    if (!idx) { set_error("null idx"); return PCC_ERR_INVALID; }
    if (!(radius >= 0)) { set_error("bad radius"); return PCC_ERR_INVALID; }
    if (nq == 0) return PCC_OK;
    PCC_TRY(ensure_grid(ix));
    ev_next(ix);
    ev_mark(ix, EV_CALL0);
    PCC_TRY(stage_queries(ix, q, nq, stride, mem));
    Out<int32_t> ri;
    PCC_TRY(ri.stage(idx, nq, mem, ix->out_idx));
    PCC_TRY(grid_first_within(ix, ix->q_packed.as<float4>(), nq, radius, ri.dev));
    ev_mark(ix, EV_CALL1);
    return finish(ix, mem, ri);
}

int pcc_match_knn(pcc_index* ix, const void* des2, size_t n2, size_t stride, int mem, float threshold,
                  int32_t* out, int32_t* out_size) {
    PCC_ENTER(ix);
    PCC_TRY(check_points(des2, n2, stride, mem));
    if (!out || !out_size) { set_error("null output"); return PCC_ERR_INVALID; }
    out[0] = 0;  // std::vector<int> correspondence(1) -- reference src/comparator.cpp:568
    *out_size = 1;
    if (n2 == 0) return PCC_OK;
    if (ix->n_orig == 0) { set_error("index is empty"); return PCC_ERR_EMPTY; }
    ev_next(ix);
    ev_mark(ix, EV_CALL0);
    if (small_call(ix, n2, stride, mem)) {
        PCC_TRY(small_nn1(ix, des2, n2, stride, true, true));
    } else {
        Nn1Call call;
        PCC_TRY(stage_queries(ix, des2, n2, stride, mem, &call));
        PCC_TRY(nn1_packed(ix, n2, call));
        if (ix->tie_mode == PCC_TIES_FLANN) PCC_TRY(resolve_ties_flann(ix, ix->q_packed.as<float4>(), ix->out_packed.as<unsigned long long>(), n2, true));
        PCC_TRY(unpack_pinned(ix, n2, true, true, false));
    }
    const int32_t* hi = ix->host_a.as<int32_t>();
    const float* hd = ix->host_b.as<float>();
    int32_t c = 1;
    for (size_t i = 0; i < n2; ++i)  // neighborCount == 1 && squaredDistances[0] < threshold (:579)
        if (hi[i] >= 0 && hd[i] < threshold) out[c++] = hi[i];
    *out_size = c;
    return PCC_OK;
}
}  // extern "C"
