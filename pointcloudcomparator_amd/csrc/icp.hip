// icp.hip -- the reduction ICP needs after every correspondence pass (gfx950).
//
// Replaces the host loop of pcl::registration::TransformationEstimationSVD::
// estimateRigidTransformation (reached from the reference's icp.align(),
// src/comparator.cpp:1096): PCL copies the matched pairs into two 3xN float matrices and
// calls Eigen's umeyama(); all umeyama needs from them are sum p, sum q and sum q p^T.
// The sums are accumulated in double (PCL/Eigen use float; compared with a tolerance,
// SURVEY hard part 6) as one partial row per workgroup, reduced on the host in a fixed
// order -> bitwise reproducible run to run (no float atomics).
#include "entry.hpp"
#include "rigid_solve.hpp"
#include <vector>

namespace pcc {

// The device-resident loop's solver and judge: one workgroup.  Lanes 0..16 add the per-workgroup partial sums in
// workgroup order (the order the host loop uses, so the sums have the same bits), lane 0 then runs Horn's closed form
// (rigid_solve.hpp), composes the running transform and applies the loop's criteria exactly as the host loop does
// (SURVEY 9.5): fewer than 3 correspondences -> stop, not converged; iteration cap -> stop, converged; |mse - previous|
// < 1e-12 (unless `fixed`) -> stop, converged.  Once stopped the state is frozen and every later pass that was already
// enqueued applies the identity.
// One body, two homes: k_icp_solve (a launch of its own: the sharded loop, whose sums pass through an all-reduce first) and the
// LAST workgroup of k_icp_sums to finish (round 6: a pass of the one-GPU loop is search -> sums, one launch less).  AGENT: the
// rows were written by other workgroups of the same launch and are read past the caches.
template <bool AGENT>
__device__ __forceinline__ void icp_solve_block(const double* __restrict__ partials, int n_blocks, IcpState* __restrict__ st, int max_iter,
                                                int fixed, const double* __restrict__ center_dev, unsigned int* __restrict__ zero_word,
                                                double* __restrict__ part /* LDS, n_blocks * 17 doubles */) {
    // (as k_pack / k_transform do: when the next pass's search applies the transform itself there is no k_transform in between)
    if (zero_word) clear_search_counters(zero_word);
    __shared__ double sums[17];
    // all partial rows, staged with coalesced loads, 8 per thread in flight (the rows come from other XCDs' write-backs: read
    // one by one in a dependent loop they cost 120 us)
    const int total = n_blocks * 17;
    for (int base = 0; base < total; base += 8 * (int)blockDim.x) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = base + (int)threadIdx.x + u * (int)blockDim.x;
            v[u] = 0.0;
            if (i < total) {
                if (AGENT) v[u] = __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(partials) + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                else v[u] = partials[i];
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = base + (int)threadIdx.x + u * (int)blockDim.x;
            if (i < total) part[i] = v[u];
        }
    }
    __syncthreads();
    if (threadIdx.x < 17) {
        double a = 0;
        int b = 0;
        for (; b + 16 <= n_blocks; b += 16) {  // 16 LDS reads in flight, added in workgroup order
            double v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = part[(b + u) * 17 + threadIdx.x];
#pragma unroll
            for (int u = 0; u < 16; ++u) a += v[u];
        }
        for (; b < n_blocks; ++b) a += part[b * 17 + threadIdx.x];
        sums[threadIdx.x] = a;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float Ti[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (!st->stopped) {
        double sm[17];
        for (int k = 0; k < 17; ++k) sm[k] = sums[k];
        float Tn[16];
        const double center[3] = {center_dev[0], center_dev[1], center_dev[2]};
        if (rigid_from_sums(sm, Tn, center) != 0) {
            st->stopped = 1;  // min_number_correspondences_: not converged
            st->converged = 0;
        } else {
            for (int k = 0; k < 16; ++k) Ti[k] = Tn[k];
            float Tt[16];
            for (int k = 0; k < 16; ++k) Tt[k] = st->T[k];
            mat4_mul_f(Ti, Tt, Tt);  // final = T_i * final
            for (int k = 0; k < 16; ++k) st->T[k] = Tt[k];
            const double mse = sm[15] / sm[16];
            const int it = st->it + 1;
            st->it = it;
            if (it >= max_iter || (!fixed && fabs(mse - st->prev_mse) < 1e-12)) {
                st->stopped = 1;  // DefaultConvergenceCriteria: the iteration cap counts as converged
                st->converged = 1;
            }
            st->prev_mse = mse;
        }
    }
    for (int k = 0; k < 16; ++k) st->Ti[k] = Ti[k];
}

__global__ void __launch_bounds__(1024)
k_icp_solve(const double* __restrict__ partials, int n_blocks, IcpState* __restrict__ st, int max_iter, int fixed,
            const double* __restrict__ center_dev, unsigned int* __restrict__ zero_word) {
    extern __shared__ double part[];
    icp_solve_block<false>(partials, n_blocks, st, max_iter, fixed, center_dev, zero_word, part);
}

__global__ void __launch_bounds__(256)
k_icp_sums(const float4* __restrict__ src, unsigned int n, const unsigned long long* __restrict__ keys,
           const float4* __restrict__ refs, double* __restrict__ partials, const unsigned int* __restrict__ mirror_dev,
           unsigned int* __restrict__ mirror_host, const double* __restrict__ center, IcpFuse fuse) {
    const double cx = center ? center[0] : 0.0, cy = center ? center[1] : 0.0, cz = center ? center[2] : 0.0;
    if (mirror_dev && blockIdx.x == 0 && threadIdx.x == 0) *mirror_host = *mirror_dev;  // fallback count for the far-query heuristic
    double acc[17];
#pragma unroll
    for (int k = 0; k < 17; ++k) acc[k] = 0.0;
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const unsigned long long key = keys[i];
        const float4 p = src[i];
        if (key_none(key) || __float_as_int(p.w) < 0) continue;  // no correspondence
        const float4 t = refs[(unsigned int)(key & 0xffffffffull)];
        // (about the caller's centre: see rigid_from_sums; exact in double, a float difference would not be)
        const double px = (double)p.x - cx, py = (double)p.y - cy, pz = (double)p.z - cz;
        const double qx = (double)t.x - cx, qy = (double)t.y - cy, qz = (double)t.z - cz;
        acc[0] += px; acc[1] += py; acc[2] += pz;
        acc[3] += qx; acc[4] += qy; acc[5] += qz;
        acc[6] += qx * px; acc[7] += qx * py; acc[8] += qx * pz;
        acc[9] += qy * px; acc[10] += qy * py; acc[11] += qy * pz;
        acc[12] += qz * px; acc[13] += qz * py; acc[14] += qz * pz;
        acc[15] += (double)__uint_as_float((unsigned int)(key >> 32));
        acc[16] += 1.0;
    }
    __shared__ double red[4][17];
#pragma unroll
    for (int k = 0; k < 17; ++k) {
        double v = acc[k];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 17)
        partials[(size_t)blockIdx.x * 17 + threadIdx.x] =
            ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    // the device-resident loop on one GPU: the last workgroup to have written its row solves the pass (IcpFuse; k_icp_solve's body)
    if (fuse.st) {
        extern __shared__ double part[];
        __shared__ unsigned int last;
        __syncthreads();  // (the row is written)
        if (threadIdx.x == 0) {
            __threadfence();
            last = atomicAdd(fuse.ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
        }
        __syncthreads();
        if (last) {  // (block-uniform)
            __threadfence();
            if (threadIdx.x == 0) *fuse.ticket = 0u;  // ready for the next pass (stream order)
            icp_solve_block<true>(partials, (int)gridDim.x, fuse.st, fuse.max_iter, fuse.fixed, center, fuse.zero_word, part);
        }
    }
}


__global__ void __launch_bounds__(64)
k_icp_rows_to_sums(const double* __restrict__ partials, int n_blocks, double* __restrict__ sums) {
    if (threadIdx.x < 17) {
        double a = 0;
        for (int b = 0; b < n_blocks; ++b) a += partials[b * 17 + threadIdx.x];  // workgroup order: k_icp_solve's, the host loop's
        sums[threadIdx.x] = a;
    }
}
int launch_icp_rows_to_sums(hipStream_t s, const double* partials, int n_blocks, double* sums17) {
    hipLaunchKernelGGL(k_icp_rows_to_sums, dim3(1), dim3(64), 0, s, partials, n_blocks, sums17);
    PCC_HIP(hipGetLastError());
    return PCC_OK;
}

int launch_icp_solve(hipStream_t s, const double* partials, int n_blocks, IcpState* state, int max_iter, int fixed,
                     const double* center_dev, unsigned int* zero_word) {
    hipLaunchKernelGGL(k_icp_solve, dim3(1), dim3(1024), (size_t)n_blocks * 17 * sizeof(double), s, partials, n_blocks, state,
                       max_iter, fixed, center_dev, zero_word);
    PCC_HIP(hipGetLastError());
    return PCC_OK;
}

// The point the ICP sums are taken about: the first valid source point (any point OF the cloud keeps sum q p^T - n pm qm^T
// within a small factor of the covariance it is meant to be; the centre of a bounding box does not when stray points
// stretch the box).  Zero for an all-invalid cloud.
__global__ void __launch_bounds__(64)
k_icp_center(const float4* __restrict__ src, unsigned int n, double* __restrict__ center) {
    const unsigned int lane = threadIdx.x;
    for (unsigned int base = 0; base < n; base += 64) {  // wave-uniform
        const unsigned int i = base + lane;
        const float4 v = i < n ? src[i] : make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
        const unsigned long long ok = __ballot(__float_as_int(v.w) >= 0);
        if (ok) {
            if (lane == (unsigned int)__builtin_ctzll(ok)) { center[0] = v.x; center[1] = v.y; center[2] = v.z; }
            return;
        }
    }
    if (lane == 0) center[0] = center[1] = center[2] = 0.0;
}
int launch_icp_center(hipStream_t s, const float4* src, size_t n, double* center_dev) {
    hipLaunchKernelGGL(k_icp_center, dim3(1), dim3(64), 0, s, src, (unsigned int)n, center_dev);
    PCC_HIP(hipGetLastError());
    return PCC_OK;
}

int launch_icp_sums(hipStream_t s, const float4* src, size_t n, const unsigned long long* keys,
                    const float4* refs, double* partials, int* n_blocks, const unsigned int* mirror_dev,
                    unsigned int* mirror_host, const double* center, const IcpFuse* fuse) {
    size_t b = (n + 256 * 8 - 1) / (256 * 8);
    if (b < 1) b = 1;
    if (b > ICP_MAX_BLOCKS) b = ICP_MAX_BLOCKS;
    *n_blocks = (int)b;
    IcpFuse f{};
    if (fuse) f = *fuse;
    hipLaunchKernelGGL(k_icp_sums, dim3((unsigned)b), dim3(256), f.st ? b * 17 * sizeof(double) : 0, s, src, (unsigned int)n, keys, refs, partials,
                       mirror_dev, mirror_host, center, f);
    PCC_HIP(hipGetLastError());
    return PCC_OK;
}

}  // namespace pcc

using namespace pcc;
extern "C" {
// reduce the per-workgroup partial rows in a fixed order
static int icp_reduce(pcc_index* ix, size_t n, double sums[17], const double* center = nullptr) {
    PCC_TRY(ix->scratch_a.reserve((size_t)ICP_MAX_BLOCKS * 17 * sizeof(double)));
    int nb = 0;
    PCC_TRY(launch_icp_sums(ix->stream, ix->q_packed.as<float4>(), n, ix->out_packed.as<unsigned long long>(),
                            ix->refs.as<float4>(), ix->scratch_a.as<double>(), &nb,
                            ix->engine == PCC_ENGINE_GRID ? &ix->words()->fb_count : nullptr, &ix->pinned()->fb_mirror, center));
    std::vector<double> h((size_t)nb * 17);
    PCC_HIP(hipMemcpyAsync(h.data(), ix->scratch_a.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, ix->stream));
    PCC_HIP(hipStreamSynchronize(ix->stream));
    for (int k = 0; k < 17; ++k) sums[k] = 0;
    for (int b = 0; b < nb; ++b)
        for (int k = 0; k < 17; ++k) sums[k] += h[(size_t)b * 17 + k];
    return PCC_OK;
}

int pcc_rigid_from_sums(const double sums[17], float T[16]) { return pcc_rigid_from_sums_about(sums, nullptr, T); }

int pcc_rigid_from_sums_about(const double sums[17], const double center[3], float T[16]) {
    if (!sums || !T) { set_error("null argument"); return PCC_ERR_INVALID; }
    if (rigid_from_sums(sums, T, center) != 0) { set_error("fewer than 3 correspondences"); return PCC_ERR_INVALID; }
    return PCC_OK;
}

int pcc_icp_step(pcc_index* ix, const void* src, size_t n, size_t stride, int mem, int32_t* idx, float* d2,
                 double sums[17]) {
    return pcc_icp_step_about(ix, src, n, stride, mem, nullptr, idx, d2, sums);
}

int pcc_icp_step_about(pcc_index* ix, const void* src, size_t n, size_t stride, int mem, const double center[3],
                       int32_t* idx, float* d2, double sums[17]) {
    PCC_ENTER(ix);
    PCC_TRY(check_points(src, n, stride, mem));
    if (center && !(std::isfinite(center[0]) && std::isfinite(center[1]) && std::isfinite(center[2]))) {
        set_error("non-finite center");
        return PCC_ERR_INVALID;
    }
    if (!sums) { set_error("null sums"); return PCC_ERR_INVALID; }
    for (int k = 0; k < 17; ++k) sums[k] = 0;
    if (n == 0) return PCC_OK;
    if (ix->n_orig == 0) { set_error("index is empty"); return PCC_ERR_EMPTY; }
    ev_next(ix);
    ev_mark(ix, EV_CALL0);
    Nn1Call call;
    PCC_TRY(stage_queries(ix, src, n, stride, mem, &call));
    PCC_TRY(nn1_packed(ix, n, call));
    const double* center_dev = nullptr;
    if (center) {  // the sums are taken about it (device copy behind the ICP loop state)
        PCC_TRY(ix->icp_state.reserve(sizeof(IcpState) + (3 + 17) * sizeof(double)));
        double* cd = reinterpret_cast<double*>(ix->icp_state.as<char>() + sizeof(IcpState));
        PCC_HIP(hipMemcpyAsync(cd, center, 3 * sizeof(double), hipMemcpyHostToDevice, ix->stream));
        PCC_HIP(hipStreamSynchronize(ix->stream));  // (center is the caller's memory)
        center_dev = cd;
    }
    PCC_TRY(icp_reduce(ix, n, sums, center_dev));
    ev_mark(ix, EV_CALL1);
    if (idx || d2) {
        Out<int32_t> ri;
        Out<float> rd;
        PCC_TRY(ri.stage(idx, n, mem, ix->out_idx));
        PCC_TRY(rd.stage(d2, n, mem, ix->out_d2));
        PCC_TRY(launch_unpack(ix->stream, ix->out_packed.as<unsigned long long>(), nullptr, n, ri.dev, rd.dev));
        PCC_TRY(finish(ix, mem, ri, rd));
    }
    return PCC_OK;
}

int pcc_transform(pcc_index* ix, const float T[16], const void* src, size_t n, size_t sstride, void* dst,
                  size_t dstride, int mem) {
    PCC_ENTER(ix);
    PCC_TRY(check_points(src, n, sstride, mem));
    PCC_TRY(check_points(dst, n, dstride, mem));
    if (!T) { set_error("null T"); return PCC_ERR_INVALID; }
    if (n == 0) return PCC_OK;
    if (mem == PCC_MEM_DEVICE) return launch_transform(ix->stream, nullptr, T, src, n, sstride, dst, dstride);
    // host: stage src (and dst, so that its other fields survive) on the device
    PCC_TRY(ix->q_raw.reserve(n * sstride));
    PCC_HIP(hipMemcpyAsync(ix->q_raw.p, src, (n - 1) * sstride + 12, hipMemcpyHostToDevice, ix->stream));
    void* ddst = ix->q_raw.p;
    size_t dbytes = (n - 1) * dstride + 12;
    if (dst != src || dstride != sstride) {
        PCC_TRY(ix->scratch_d.reserve(n * dstride));
        PCC_HIP(hipMemcpyAsync(ix->scratch_d.p, dst, dbytes, hipMemcpyHostToDevice, ix->stream));
        ddst = ix->scratch_d.p;
    }
    PCC_TRY(launch_transform(ix->stream, nullptr, T, ix->q_raw.p, n, sstride, ddst, dstride));
    PCC_HIP(hipMemcpyAsync(dst, ddst, dbytes, hipMemcpyDeviceToHost, ix->stream));
    PCC_HIP(hipStreamSynchronize(ix->stream));
    return PCC_OK;
}

int pcc_icp_align(pcc_index* ix, const void* src, size_t n, size_t stride, int mem, int max_iter, int fixed,
                  float T[16], double* fitness, int* iterations, int* converged) {
    return pcc::icp_align_impl(ix, nullptr, src, n, stride, mem, max_iter, fixed, T, fitness, iterations, converged);
}
}  // extern "C"

// pcc_icp_align, and -- with `hooks` -- its sharded form: this handle holds one SHARD of the source cloud, the 17 sums of
// every pass are added up over the ranks (hooks->allreduce_sum_f64: RCCL on the handle's stream, comm.hip) before the
// solver sees them, so every rank solves the same transform and moves its shard (reference
// src/comparator.cpp:1089-1110).  With one rank the all-reduce is the identity and the result is pcc_icp_align's, bit for bit.
int pcc::icp_align_impl(pcc_index* ix, const pcc::IcpHooks* hooks, const void* src, size_t n, size_t stride, int mem, int max_iter,
                        int fixed, float T[16], double* fitness, int* iterations, int* converged) {
    // (PCC_ENTER without its early return: a device that cannot be selected is a failure of this rank alone and has to reach the
    // status exchange below like every other one -- a return here would leave the peers waiting in it)
    if (!ix) { set_error("null index"); return PCC_ERR_INVALID; }  // (the sharded entry point has checked this before its peers can wait)
    pcc::Entry entry(ix);
    const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    int it = 0;
    bool conv = false;
    double prev_mse = 1.79769313486231570e308;
    double* center_dev = nullptr;
    bool sorted = false;
    Nn1Call call;  // every search below is an ICP pass: they share the first pass's lane order (Nn1Call::order_given)
    call.icp_pass = true;
    // Everything that can fail on ONE rank alone -- argument checks, staging, allocations -- comes before the first
    // collective and ends in a status the ranks agree on (hooks->agree: all-reduce MIN of one word), so a rank that
    // cannot go on takes the others out with it instead of leaving them in the broadcast below (comm.hip).
    auto prepare = [&]() -> int {
        PCC_TRY(entry.status);
        PCC_TRY(check_points(src, n, stride, mem));
        if (!T) { set_error("null T"); return PCC_ERR_INVALID; }
        if (ix->n_orig == 0) { set_error("index is empty"); return PCC_ERR_EMPTY; }
        memcpy(T, I, sizeof(I));
        if (iterations) *iterations = 0;
        if (converged) *converged = 0;
        if (n == 0 && hooks) { set_error("sharded ICP: every rank needs a non-empty shard"); return PCC_ERR_INVALID; }
        if (n == 0) return PCC_OK;
        // the source stays resident: q_packed is the moving cloud, icp_src keeps the input
        PCC_TRY(stage_queries(ix, src, n, stride, mem, &call));
        PCC_TRY(ix->icp_src.reserve(n * sizeof(float4)));
        // Round 5: the loop's working set in the target grid's CELL order.  Nothing of the loop leaves per point -- T, fitness,
        // counts -- so the permutation that a search pays per call (queries gathered through the sort order, keys scattered
        // back: ~60 us of a 215-us pass at 2M points, tools/ubench/ubench_scatter.hip) is paid ONCE: the source is sorted by the
        // cell it starts in, gathered into that order, and every pass reads it front to back with the identity as its order
        // (a rigid motion keeps neighbouring points neighbours; any order is correct, as before).  The sums are added up in
        // this order by every form of the loop -- device-resident, host-driven, sharded -- so they agree with each other to
        // the bit as before; against the caller's order they differ in the last bits of a double sum.
        sorted = ix->opt.icp_sorted != 0 && ix->engine == PCC_ENGINE_GRID && ix->has_grid && n >= 4096;
        if (sorted) {
            unsigned int *order = nullptr, *n_sorted = nullptr;
            PCC_TRY(grid_sort_queries(ix, ix->q_packed.as<float4>(), n, &order, &n_sorted));
            PCC_TRY(launch_gather_sorted(ix->stream, ix->q_packed.as<float4>(), order, n_sorted, n, ix->icp_src.as<float4>(),
                                         &ix->words()->icp_nsorted));
            PCC_HIP(hipMemcpyAsync(ix->q_packed.p, ix->icp_src.p, n * sizeof(float4), hipMemcpyDeviceToDevice, ix->stream));
        } else
        PCC_HIP(hipMemcpyAsync(ix->icp_src.p, ix->q_packed.p, n * sizeof(float4), hipMemcpyDeviceToDevice, ix->stream));
        // the sums of every pass are taken about a point of the source cloud (k_icp_center: no cancellation in the
        // covariance for clouds far from the origin); it sits behind the loop state in device memory
        PCC_TRY(ix->icp_state.reserve(sizeof(IcpState) + (3 + 17) * sizeof(double)));
        PCC_TRY(ix->scratch_a.reserve((size_t)ICP_MAX_BLOCKS * 17 * sizeof(double)));
        center_dev = reinterpret_cast<double*>(ix->icp_state.as<char>() + sizeof(IcpState));
        PCC_TRY(launch_icp_center(ix->stream, ix->q_packed.as<float4>(), n, center_dev));
        return PCC_OK;
    };
    int st_prep = prepare();
    if (hooks) st_prep = hooks->agree(hooks->ctx, st_prep);
    if (st_prep != PCC_OK) return st_prep;
    if (n == 0) return PCC_OK;
    if (hooks) PCC_TRY(hooks->bcast_f64(hooks->ctx, center_dev, 3, 0, ix->stream));  // every rank about rank 0's point
    const int warm_env = ix->opt.icp_warm;         // 0: every pass from scratch (measurements)
    const int loop_env = hooks ? 1 : ix->opt.icp_device_loop;  // 0: the host-driven loop (kept for comparison: same bits)
    double* sums_dev = center_dev + 3;  // (sharded: the 17 sums of a pass, all-reduced in place)
    const bool fold = sorted && loop_env && grid_nn1_takes_transform(ix);  // the pass's transform applied by the next pass's search
    if (sorted) {  // (the passes take the identity as their order; the count of valid points sits in a word of its own)
        call.order_given = true; call.order_nq = n;
        call.order = nullptr; call.n_sorted = &ix->words()->icp_nsorted;
    }
    if (loop_env) {
        // The loop lives on the device: every pass is NN -> sums -> k_icp_solve (one workgroup: the transform, the running
        // product and the convergence criteria) -> transform with the matrix the solver left in device memory.  Passes
        // are enqueued in chunks without a host round trip (the host loop below pays a stream synchronisation, a
        // read-back and a launch gap per pass, ~65 us of 0.44 ms); after each chunk the host looks whether the loop
        // has stopped.  Passes enqueued past the stop are no-ops on the state (identity transform), so a chunk costs at
        // most its own length in wasted searches -- none with a fixed count, where the whole loop is one chunk.
        IcpState h0{};
        memcpy(h0.Ti, I, sizeof(I));
        memcpy(h0.T, I, sizeof(I));
        h0.prev_mse = 1.79769313486231570e308;
        PCC_HIP(hipMemcpyAsync(ix->icp_state.p, &h0, sizeof(h0), hipMemcpyHostToDevice, ix->stream));
        PCC_HIP(hipStreamSynchronize(ix->stream));  // (h0 lives on this stack frame)
        IcpState* st = ix->icp_state.as<IcpState>();
        IcpState h1 = h0;
        // passes per host look: 5 with criteria active; with a fixed count the loop would need none, but a source that
        // leaves fewer than 3 correspondences stops it on the device and every pass enqueued beyond that is a wasted
        // search -- so at most 32 at a time (one look costs ~20 us)
        const int chunk = fixed ? (max_iter < 32 ? max_iter : 32) : 5;
        for (int pass = 0; pass < max_iter && !h1.stopped;) {
            for (int c = 0; c < chunk && pass < max_iter; ++c, ++pass) {
                ev_next(ix);  // instrumentation: every pass is one "call" (NN kernel, far/fallback, whole pass)
                ev_mark(ix, EV_CALL0);
                // (cell-ordered loop: the search applies the previous pass's matrix -- the identity before the first -- to the
                // queries it reads and writes them back; no transform kernel, grid.hip k_grid_nn1_flat2)
                call.pre_transform = fold ? st->Ti : nullptr;
                PCC_TRY(nn1_packed(ix, n, call));  // determineCorrespondences: one NN per source point
                call.pre_transform = nullptr;
                call.warm = warm_env != 0;  // from now on out_packed holds the last pass's keys of these same points
                int nb = 0;
                unsigned int* zw = ix->engine == PCC_ENGINE_GRID ? &ix->words()->fb_count : nullptr;
                // (one GPU: the sums kernel's last workgroup solves the pass itself -- DevWords::icp_ticket is its ticket word;
                // PCC_OPT_FUSE_PARAMS bit 1; the sharded loop keeps the solver's own launch: its sums pass through an all-reduce)
                const bool fuse_solve = !hooks && (ix->opt.fuse_params & 2) != 0;
                const IcpFuse fuse{&ix->words()->icp_ticket, st, max_iter, fixed, fold ? zw : nullptr};
                PCC_TRY(launch_icp_sums(ix->stream, ix->q_packed.as<float4>(), n, ix->out_packed.as<unsigned long long>(),
                                        ix->refs.as<float4>(), ix->scratch_a.as<double>(), &nb, zw,
                                        &ix->pinned()->fb_mirror, center_dev, fuse_solve ? &fuse : nullptr));
                if (fuse_solve) {
                } else if (hooks) {  // rows -> 17 sums (workgroup order, as the solver adds them) -> sum over the ranks -> solve
                    PCC_TRY(launch_icp_rows_to_sums(ix->stream, ix->scratch_a.as<double>(), nb, sums_dev));
                    PCC_TRY(hooks->allreduce_sum_f64(hooks->ctx, sums_dev, 17, ix->stream));
                    PCC_TRY(launch_icp_solve(ix->stream, sums_dev, 1, st, max_iter, fixed, center_dev, fold ? zw : nullptr));
                } else
                PCC_TRY(launch_icp_solve(ix->stream, ix->scratch_a.as<double>(), nb, st, max_iter, fixed, center_dev, fold ? zw : nullptr));
                // (the transform -- or, when the next search applies it itself, the solver -- also zeroes the counters of the next
                // pass's search)
                if (!fold) PCC_TRY(launch_transform(ix->stream, st->Ti, nullptr, ix->q_packed.p, n, sizeof(float4), ix->q_packed.p, sizeof(float4), zw));
                call.counters_cleared = zw != nullptr;
                ev_mark(ix, EV_CALL1);
            }
            PCC_HIP(hipMemcpyAsync(&h1, ix->icp_state.p, sizeof(h1), hipMemcpyDeviceToHost, ix->stream));
            PCC_HIP(hipStreamSynchronize(ix->stream));
        }
        memcpy(T, h1.T, sizeof(h1.T));
        it = h1.it;
        conv = h1.converged != 0;
    } else {
    double center[3] = {0, 0, 0};
    bool have_center = false;
    while (it < max_iter) {
        ev_next(ix);  // instrumentation: every pass is one "call" (NN kernel, far/fallback, whole pass)
        ev_mark(ix, EV_CALL0);
        PCC_TRY(nn1_packed(ix, n, call));  // determineCorrespondences: one NN per source point
        call.warm = warm_env != 0;  // from now on out_packed holds the last pass's keys of these same points
        double sums[17];
        PCC_TRY(icp_reduce(ix, n, sums, center_dev));
        if (!have_center) {
            PCC_HIP(hipMemcpyAsync(center, center_dev, sizeof(center), hipMemcpyDeviceToHost, ix->stream));
            PCC_HIP(hipStreamSynchronize(ix->stream));
            have_center = true;
        }
        float Ti[16];
        if (rigid_from_sums(sums, Ti, center) != 0) { conv = false; break; }  // < 3 correspondences: not converged
        PCC_TRY(launch_transform(ix->stream, nullptr, Ti, ix->q_packed.p, n, sizeof(float4), ix->q_packed.p, sizeof(float4)));
        ev_mark(ix, EV_CALL1);
        mat4_mul_f(Ti, T, T);  // final = T_i * final
        const double mse = sums[15] / sums[16];
        ++it;
        if (it >= max_iter) { conv = true; break; }  // DefaultConvergenceCriteria: iteration cap counts as converged
        if (!fixed && std::fabs(mse - prev_mse) < 1e-12) { conv = true; break; }
        prev_mse = mse;
    }
    }
    if (iterations) *iterations = it;
    if (converged) *converged = conv ? 1 : 0;
    if (fitness) {
        // getFitnessScore: re-transform the INPUT with the final matrix, one more NN pass, mean d2
        PCC_TRY(launch_transform(ix->stream, nullptr, T, ix->icp_src.p, n, sizeof(float4), ix->q_packed.p, sizeof(float4)));
        // launch_transform writes x,y,z only: refresh the validity flags from the input
        PCC_TRY(launch_copy_w(ix->stream, ix->icp_src.as<float4>(), ix->q_packed.as<float4>(), n));
        ev_next(ix);
        ev_mark(ix, EV_CALL0);
        PCC_TRY(nn1_packed(ix, n, call));
        double sums[17];
        if (hooks) {  // sum of d2 and count over ALL shards
            int nb = 0;
            PCC_TRY(launch_icp_sums(ix->stream, ix->q_packed.as<float4>(), n, ix->out_packed.as<unsigned long long>(), ix->refs.as<float4>(),
                                    ix->scratch_a.as<double>(), &nb, nullptr, nullptr, nullptr));
            PCC_TRY(launch_icp_rows_to_sums(ix->stream, ix->scratch_a.as<double>(), nb, sums_dev));
            PCC_TRY(hooks->allreduce_sum_f64(hooks->ctx, sums_dev, 17, ix->stream));
            PCC_HIP(hipMemcpyAsync(sums, sums_dev, sizeof(sums), hipMemcpyDeviceToHost, ix->stream));
            PCC_HIP(hipStreamSynchronize(ix->stream));
        } else
        PCC_TRY(icp_reduce(ix, n, sums));
        ev_mark(ix, EV_CALL1);
        *fitness = sums[16] > 0 ? sums[15] / sums[16] : 1.79769313486231570e308;
    }
    PCC_HIP(hipStreamSynchronize(ix->stream));
    return PCC_OK;
}
