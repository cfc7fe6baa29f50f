// vfh.hip -- the VFH descriptor of ONE cloud and the distance between such descriptors (gfx950): pcc_vfh_descriptor, pcc_match_vfh.
// replaces: processVHF (reference src/comparator.cpp:482-516): pcl::NormalEstimation (setRadiusSearch 0.03) and
//   pcl::VFHEstimation with setNormalizeBins(true), setNormalizeDistance(false); and matchVHF (:471-480).
//
// VFH is a GLOBAL descriptor: one 308-bin histogram per cloud, every point voting once against the cloud's centroid and the
// centroid of its normals.  Two parts of it are serial by definition -- the six float chains of the centroids, in index order,
// and every bin's value, its increment added once per vote -- and the rest is one independent evaluation per point:
//   1. the plane fit over the sorted radius rows at normal_radius (normals.hip), the first stage of fpfh_stages;
//   2. k_vfh_centroids: one wave carries the six chains over tiles parked in LDS (k_cd_centroids' scheme) and leaves the
//      centroid, the normal centroid, the count of finite normals and d_vp_p in a small device record;
//   3. k_vfh_votes: one point per lane; the votes are counted in integers, per workgroup in LDS and then with integer atomics
//      in 263 global counters -- integer sums do not depend on the order of arrival, so the result is reproducible;
//   4. k_vfh_finish: lane b rebuilds bin b from its count, the increment added count times (fpfh_spfh_value).
// No float atomic anywhere, no host round trip between the stages; launches and waits do not depend on n.  The stages take
// (refs, normals, first point, count), so that a batch call can run them per cluster.  The arithmetic is vfh_math.hpp's, shared
// with the host mirror of the tests: same operations, same order, same bits.
#include <algorithm>

#include "entry.hpp"
#include "vfh_math.hpp"
#include "vfh_device.hpp"

namespace pcc {

namespace {

struct VfhScratch : Scratch {
    static constexpr ScratchSlot slot = SCRATCH_VFH;
    DevBuf normals;              // float4[n] plane fit
    DevBuf record, counters;     // VfhRecord; uint32[VFH_COUNTERS], zeroed on the stream in every call
    DevBuf out_hist;             // the descriptor staged for a caller in host memory
    DevBuf in1, in2, out_dist;   // pcc_match_vfh: the caller's arrays staged (host memory)
};

// ---- 2. centroids ---------------------------------------------------------------------------------------------------------------
// One wave (one 64-lane workgroup) for the cloud [first, first + n): the six chains, tile-parked in LDS (vfh_device.hpp:
// vfh_centroid_chains, the one body this kernel and the batch call's share).
__global__ void __launch_bounds__(64)
k_vfh_centroids(const float4* __restrict__ refs, const float4* __restrict__ normals, unsigned int first, unsigned int n,
                VfhRecord* __restrict__ rec) {
    vfh_centroid_chains(refs + first, normals + first, n, rec);
}

// ---- 3. votes -------------------------------------------------------------------------------------------------------------------
// Grid-stride, one point per lane: the four bins of the point (vfh_vote) counted in the workgroup's LDS table of 3 x 45 + 128
// counters; the workgroup then adds its non-zero counters to the global ones.  Every bin number is clamped to its range by
// vfh_math.hpp, so no index leaves the table.
__global__ void __launch_bounds__(256)
k_vfh_votes(const float4* __restrict__ refs, const float4* __restrict__ normals, unsigned int first, unsigned int n,
            const VfhRecord* __restrict__ rec, unsigned int* __restrict__ counters) {
    __shared__ unsigned int table[VFH_COUNTERS];
    for (unsigned int t = threadIdx.x; t < (unsigned int)VFH_COUNTERS; t += blockDim.x) table[t] = 0u;
    __syncthreads();
    const VfhRecord r = *rec;
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 pv = refs[first + i], nv = normals[first + i];
        const float p[3] = {pv.x, pv.y, pv.z}, nrm[3] = {nv.x, nv.y, nv.z};
        const VfhVote v = vfh_vote(r.centroid, r.normal_centroid, r.d_vp_p, p, nrm);
        if (v.f1 != VFH_NO_VOTE) {
            atomicAdd(&table[v.f1], 1u);
            atomicAdd(&table[VFH_F_BINS + v.f2], 1u);
            atomicAdd(&table[2 * VFH_F_BINS + v.f3], 1u);
        }
        atomicAdd(&table[3 * VFH_F_BINS + v.vp], 1u);
    }
    __syncthreads();
    for (unsigned int t = threadIdx.x; t < (unsigned int)VFH_COUNTERS; t += blockDim.x)
        if (table[t]) atomicAdd(&counters[t], table[t]);
}

// ---- 4. the bins from their counts ----------------------------------------------------------------------------------------------
// lane b < 308 rebuilds bin b: at most n additions per lane, 308 lanes side by side
__global__ void __launch_bounds__(320)
k_vfh_finish(const unsigned int* __restrict__ counters, unsigned int n, float* __restrict__ out_hist) {
    const int b = (int)threadIdx.x;
    if (b < VFH_BINS) out_hist[b] = vfh_bin_value(counters, n, b);
}

// The stages behind the normals over the points [first, first + n) of a packed cloud, n >= 2: refs and normals on the device,
// out_hist[308] on the device.  No wait.
int vfh_stages(pcc_index* ix, VfhScratch* r, const float4* refs, const float4* normals, unsigned int first, unsigned int n, float* out_hist) {
    hipStream_t s = ix->stream;
    PCC_TRY(r->record.reserve(sizeof(VfhRecord)));
    PCC_TRY(r->counters.reserve(VFH_COUNTERS * sizeof(unsigned int)));
    PCC_HIP(hipMemsetAsync(r->counters.p, 0, VFH_COUNTERS * sizeof(unsigned int), s));
    ev_mark(ix, EV_SORT0);
    hipLaunchKernelGGL(k_vfh_centroids, dim3(1), dim3(64), 0, s, refs, normals, first, n, r->record.as<VfhRecord>());
    PCC_HIP(hipGetLastError());
    ev_mark(ix, EV_SORT1);
    const unsigned int blocks = (unsigned int)std::min<size_t>(((size_t)n + 255) / 256, 1024);
    ev_mark(ix, EV_MAIN0);
    hipLaunchKernelGGL(k_vfh_votes, dim3(blocks), dim3(256), 0, s, refs, normals, first, n, r->record.as<VfhRecord>(), r->counters.as<unsigned int>());
    PCC_HIP(hipGetLastError());
    ev_mark(ix, EV_MAIN1);
    ev_mark(ix, EV_FB0);
    hipLaunchKernelGGL(k_vfh_finish, dim3(1), dim3(320), 0, s, r->counters.as<unsigned int>(), n, out_hist);
    PCC_HIP(hipGetLastError());
    ev_mark(ix, EV_FB1);
    return PCC_OK;
}

// ---- matchVHF -------------------------------------------------------------------------------------------------------------------
// one lane per pair (i, j) walks the 308 terms in order (vfh_distance); not a hot path
__global__ void __launch_bounds__(256)
k_vfh_match(const float* __restrict__ h1, const float* __restrict__ h2, unsigned int n2, unsigned int pairs, double* __restrict__ out) {
    for (unsigned int t = blockIdx.x * blockDim.x + threadIdx.x; t < pairs; t += gridDim.x * blockDim.x) {
        const unsigned int i = t / n2, j = t - i * n2;
        out[t] = vfh_distance(h1 + (size_t)i * VFH_BINS, h2 + (size_t)j * VFH_BINS);
    }
}

}  // namespace

int check_vfh_params(double normal_radius, const float* out_hist, const size_t* n_out) {
    if (!out_hist || !n_out) { set_error("null argument"); return PCC_ERR_INVALID; }
    if (!(normal_radius > 0) || !std::isfinite(normal_radius)) { set_error("bad radius"); return PCC_ERR_INVALID; }
    return PCC_OK;
}

}  // namespace pcc

using namespace pcc;
extern "C" {
int pcc_vfh_descriptor(pcc_index* ix, int mem, double normal_radius, float* out_hist, size_t* n_out) {
    // the arguments first: host arithmetic, refused before any device is looked at
    PCC_TRY(check_mem(mem));
    PCC_TRY(check_vfh_params(normal_radius, out_hist, n_out));
    PCC_ENTER(ix);
    PCC_TRY(ensure_grid(ix));
    PCC_TRY(sync_info(ix));
    const size_t n = ix->n_orig;
    if (ix->n_valid != n) {
        set_error("VFH of a cloud with %zu non-finite points: the reference strips them when it loads a cloud", n - ix->n_valid);
        return PCC_ERR_UNSUPPORTED;
    }
    if (n < 2) { *n_out = 0; return PCC_OK; }  // (PCL's initCompute fails: an empty descriptor cloud)
    ev_next(ix);
    ev_mark(ix, EV_CALL0);
    VfhScratch* r = scratch<VfhScratch>(ix);
    Out<float> rh;
    PCC_TRY(rh.stage(out_hist, VFH_BINS, mem, r->out_hist));
    PCC_TRY(r->normals.reserve(n * sizeof(float4)));
    // rows at normal_radius: the plane fit, turned to the origin; every point stays, whatever its normal holds
    const float origin[3] = {0.f, 0.f, 0.f};
    const unsigned long long* keys = nullptr;
    const unsigned int* off32 = nullptr;
    PCC_TRY(radius_csr(ix, normal_radius, &keys, &off32));
    PCC_TRY(launch_normals_csr(ix, keys, off32, origin, r->normals.as<float4>()));
    PCC_TRY(vfh_stages(ix, r, ix->refs.as<float4>(), r->normals.as<float4>(), 0u, (unsigned int)n, rh.dev));
    *n_out = 1;
    ev_mark(ix, EV_CALL1);
    return finish(ix, mem, rh);
}

int pcc_match_vfh(pcc_index* ix, const float* hist1, size_t n1, const float* hist2, size_t n2, int mem, double* out_dist) {
    PCC_TRY(check_mem(mem));
    if (n1 == 0 || n2 == 0) return PCC_OK;  // (nothing to write, no device is looked at)
    if (!hist1 || !hist2 || !out_dist) { set_error("null argument"); return PCC_ERR_INVALID; }
    if (n1 >= (1ull << 31) || n2 >= (1ull << 31) || n1 * n2 >= (1ull << 31)) { set_error("more than 2^31 - 1 pairs"); return PCC_ERR_UNSUPPORTED; }
    PCC_ENTER(ix);
    const unsigned int pairs = (unsigned int)(n1 * n2);
    VfhScratch* r = scratch<VfhScratch>(ix);
    const float *d1 = nullptr, *d2 = nullptr;
    PCC_TRY(stage_in(ix, hist1, n1 * VFH_BINS, mem, r->in1, &d1));
    PCC_TRY(stage_in(ix, hist2, n2 * VFH_BINS, mem, r->in2, &d2));
    Out<double> rd;
    PCC_TRY(rd.stage(out_dist, pairs, mem, r->out_dist));
    const unsigned int blocks = std::min<unsigned int>((pairs + 255u) / 256u, 4096u);
    hipLaunchKernelGGL(k_vfh_match, dim3(blocks), dim3(256), 0, ix->stream, d1, d2, (unsigned int)n2, pairs, rd.dev);
    PCC_HIP(hipGetLastError());
    return finish(ix, mem, rd);
}
}  // extern "C"
