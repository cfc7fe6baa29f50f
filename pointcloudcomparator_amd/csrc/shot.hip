// shot.hip -- the SHOT352 descriptor pipeline of ONE cloud (gfx950): pcc_shot_descriptors.
// replaces: processSHOT (reference src/comparator.cpp:941-986): pcl::NormalEstimation (setRadiusSearch 0.05),
//   removeNaNNormalsFromPointCloud, pcl::SHOTEstimation<PointXYZRGB, Normal, SHOT352> (setRadiusSearch 0.04).  Lines 915-939 (the
//   SIFT keypoints, the rand() draw and the snap to the cloud) stay with the caller.
//
// Both stages of SHOTEstimation -- the local reference frame and the 352 bins -- consume the sorted radius row of the indexed cloud
// at shot_radius (CSR of u64 keys, d2 bits << 32 | point index, ascending).  When shot_radius <= normal_radius (the reference's
// radii) ONE CSR is built, at normal_radius: a row is ascending, so its entries with d2 < float(shot_radius^2) are a prefix, and the
// SHOT kernels stop at its end.  As in fpfh.hip the compaction is not carried out in front: cloud2 (the points with a finite
// normal) is a subset in the same order, the consumers skip the entries of the others, and every row is written at pos[i], the
// exclusive scan of the flags.  The arithmetic is shot_math.hpp's and libm_f64.hpp's, shared with the host mirror of the tests:
// same operations, same order, same bits.
//
// The orders that are part of the result, and how the kernels keep them (a wave per row, four rows a workgroup):
//   frame sums   per chunk of 64 row entries every lane prepares the seven double terms of ONE entry; then EVERY lane walks the
//                chunk's entries in row order and adds the terms it reads from their lanes (v_readlane): one chain, the same in
//                all 64 lanes, no reduction tree.  Every lane then runs the same Jacobi on the same sums.
//   sign votes   integer ballots; an entry's position in the list of valid entries is a ballot prefix.
//   bins         per chunk every lane evaluates shot_entry for ONE entry and parks its (at most five) contributions in LDS;
//                then lane l, the owner of the bins l, l + 64, ..., walks the parked list entry by entry, contribution by
//                contribution, and adds what targets its bins: float adds in row order, no float atomic.
//   norm         every lane sums the 352 squares in index order (shot_norm: one chain in double, the same in all lanes).
#include <algorithm>

#include "entry.hpp"
#include "lane_ops.hpp"
#include "grid_device.hpp"
#include "shot_math.hpp"

namespace pcc {

namespace {

// What pcc_shot_descriptors keeps between its stages.  Buffers of their own: the radius searches in between use the handle's
// shared scratch.
struct ShotScratch : Scratch {
    static constexpr ScratchSlot slot = SCRATCH_SHOT;
    DevBuf normals;                      // float4[n] plane fit
    DevBuf rf;                           // float[n][9]: the frame of every point of cloud2, by original index
    DevBuf flags, pos, scan_tmp;         // uint32[n]: 1 for the points of cloud2; uint32[n + 1]: their exclusive scan, pos[n] = the count
    DevBuf out_desc, out_rf, out_index;  // results staged for a caller in host memory
};

// flags[i] = 1 for the points of cloud2 (every component of the normal finite); pos = the same, to be scanned
__global__ void __launch_bounds__(256)
k_shot_flags(const float4* __restrict__ normals, unsigned int n, unsigned int* __restrict__ flags, unsigned int* __restrict__ pos) {
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 nv = normals[i];
        const unsigned int in2 = shot_finite(nv.x) && shot_finite(nv.y) && shot_finite(nv.z) ? 1u : 0u;
        flags[i] = in2;
        pos[i] = in2;
    }
}

// the double of lane k (wave-uniform k)
__device__ __forceinline__ double readlane_f64(double x, int k) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), k);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), k);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ unsigned int lanes_below(unsigned long long mask, unsigned int l) {
    return (unsigned int)__popcll(mask & ((1ull << l) - 1ull));
}

// getLocalRF, a wave per row (four rows a workgroup), rows in cell order.  Pass 1: the seven sums in row order (see the top of
// the file) and `valid`; the axes (all lanes alike); pass 2 over the same entries: the sign votes as ballots.  Lane 0 writes the
// frame to rf[i][9]: NaN when valid < 5 or an eigenvalue is not finite.
__global__ void __launch_bounds__(256)
k_shot_lrf64(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ offsets, const float4* __restrict__ refs,
             const unsigned int* __restrict__ flags, const float4* __restrict__ cell_refs, const GridDev* __restrict__ gd, float r2,
             double radius, float* __restrict__ rf_out) {
    const unsigned int l = threadIdx.x & 63;
    const unsigned int n_valid = gd->n_valid;
    const unsigned int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (unsigned int t = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; t < n_valid; t += nwaves) {
        const unsigned int i = (unsigned int)__float_as_int(cell_refs[t].w);
        if (!flags[i]) continue;  // (the wave's: not in cloud2)
        const unsigned int beg = offsets[i], end = offsets[i + 1];
        const float4 p4 = refs[i];
        const float p[3] = {p4.x, p4.y, p4.z};
        double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        int valid = 0;
        for (unsigned int e0 = beg; e0 < end; e0 += 64) {
            const unsigned int e = e0 + l;
            bool past = false, use = false;
            double term[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (e < end) {
                const unsigned long long key = keys[e];
                const unsigned int j = (unsigned int)key;
                const float d2 = __uint_as_float((unsigned int)(key >> 32));
                past = !(d2 < r2);
                use = !past && flags[j] != 0u && d2 != 0.f;
                if (use) {
                    const float4 q4 = refs[j];
                    const float q[3] = {q4.x, q4.y, q4.z};
                    double v[3];
                    shot_lrf_term(p, q, d2, radius, v, term);
                }
            }
            unsigned long long todo = __ballot(use);
            valid += (int)__popcll(todo);
            while (todo) {
                const int k = __builtin_ctzll(todo);
                todo &= todo - 1;
#pragma unroll
                for (int c = 0; c < 7; ++c) acc[c] += readlane_f64(term[c], k);
            }
            if (__ballot(past)) break;  // (the row is ascending: the prefix with d2 < r2 has ended)
        }
        float rf[9];
        double x[3], z[3];
        if (valid >= SHOT_MIN_NEIGHBOURS && shot_lrf_axes(acc, x, z)) {
            int plus_x = 0, plus_z = 0, med_x = 0, med_z = 0, base = 0;
            for (unsigned int e0 = beg; e0 < end; e0 += 64) {
                const unsigned int e = e0 + l;
                bool past = false, use = false;
                double dx = 0.0, dz = 0.0;
                if (e < end) {
                    const unsigned long long key = keys[e];
                    const unsigned int j = (unsigned int)key;
                    const float d2 = __uint_as_float((unsigned int)(key >> 32));
                    past = !(d2 < r2);
                    use = !past && flags[j] != 0u && d2 != 0.f;
                    if (use) {
                        const float4 q4 = refs[j];
                        const double v[3] = {(double)(q4.x - p[0]), (double)(q4.y - p[1]), (double)(q4.z - p[2])};
                        dx = shot_dot(v, x);
                        dz = shot_dot(v, z);
                    }
                }
                const unsigned long long mask = __ballot(use);
                const bool median = use && shot_sign_median(base + (int)lanes_below(mask, l), valid);
                plus_x += (int)__popcll(__ballot(use && dx >= 0.0));
                plus_z += (int)__popcll(__ballot(use && dz >= 0.0));
                med_x += (int)__popcll(__ballot(median && dx > 0.0));
                med_z += (int)__popcll(__ballot(median && dz > 0.0));
                base += (int)__popcll(mask);
                if (__ballot(past)) break;
            }
            if (shot_sign_negate(plus_x, valid, med_x)) for (int k = 0; k < 3; ++k) x[k] = x[k] * -1.0;
            if (shot_sign_negate(plus_z, valid, med_z)) for (int k = 0; k < 3; ++k) z[k] = z[k] * -1.0;
            shot_rf(x, z, rf);
        } else {
            shot_rf_nan(rf);
        }
        if (l == 0) {
#pragma unroll
            for (int k = 0; k < 9; ++k) rf_out[(size_t)i * 9 + k] = rf[k];
        }
    }
}

// computePointSHOT, a wave per row (four rows a workgroup), rows in cell order: see the top of the file.  The descriptor (and the
// frame, when out_rf is not null) goes to row pos[i] of the output; 352 NaN when the row counts fewer than 5 entries of cloud2 or
// the frame is NaN.
constexpr unsigned int SHOT_NO_BIN = 0xffffffffu;
__global__ void __launch_bounds__(256)
k_shot_desc64(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ offsets, const float4* __restrict__ refs,
              const float4* __restrict__ normals, const unsigned int* __restrict__ flags, const unsigned int* __restrict__ pos,
              const float* __restrict__ rf_in, const float4* __restrict__ cell_refs, const GridDev* __restrict__ gd, float r2, double radius,
              float* __restrict__ out_desc, float* __restrict__ out_rf, int32_t* __restrict__ out_index) {
    __shared__ float hist_all[4][SHOT_BINS];
    __shared__ unsigned long long park_all[4][64 * 5];  // bin << 32 | the bits of the value
    const unsigned int l = threadIdx.x & 63;
    float* hist = hist_all[threadIdx.x >> 6];
    unsigned long long* park = park_all[threadIdx.x >> 6];
    const unsigned int n_valid = gd->n_valid;
    const unsigned int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (unsigned int t = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; t < n_valid; t += nwaves) {
        const unsigned int i = (unsigned int)__float_as_int(cell_refs[t].w);
        if (!flags[i]) continue;  // (the wave's: not in cloud2)
        const unsigned int beg = offsets[i], end = offsets[i + 1];
        const float4 p4 = refs[i];
        const float p[3] = {p4.x, p4.y, p4.z};
        float rf[9];
        bool frame = true;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            rf[k] = rf_in[(size_t)i * 9 + k];
            frame = frame && shot_finite(rf[k]);
        }
        wave_lds_sync();
        for (unsigned int b = l; b < (unsigned int)SHOT_BINS; b += 64) hist[b] = 0.f;
        wave_lds_sync();
        unsigned int row_len = 0;
        for (unsigned int e0 = beg; e0 < end; e0 += 64) {
            const unsigned int e = e0 + l;
            bool past = false, in2 = false, votes = false;
            int bin[5] = {-1, -1, -1, -1, -1};
            float val[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
            if (e < end) {
                const unsigned long long key = keys[e];
                const unsigned int j = (unsigned int)key;
                const float d2 = __uint_as_float((unsigned int)(key >> 32));
                past = !(d2 < r2);
                in2 = !past && flags[j] != 0u;
                if (in2 && frame) {
                    const float4 q4 = refs[j], n4 = normals[j];
                    const float q[3] = {q4.x, q4.y, q4.z}, nq[3] = {n4.x, n4.y, n4.z};
                    votes = shot_entry(p, rf, q, nq, d2, radius, bin, val);
                }
            }
            row_len += (unsigned int)__popcll(__ballot(in2));
#pragma unroll
            for (int c = 0; c < 5; ++c) {
                const unsigned int b = votes && (unsigned int)bin[c] < (unsigned int)SHOT_BINS ? (unsigned int)bin[c] : SHOT_NO_BIN;
                park[l * 5 + c] = ((unsigned long long)b << 32) | __float_as_uint(val[c]);
            }
            wave_lds_sync();
            unsigned long long todo = __ballot(votes);
            while (todo) {
                const int k = __builtin_ctzll(todo);
                todo &= todo - 1;
#pragma unroll
                for (int c = 0; c < 5; ++c) {
                    const unsigned long long w = park[k * 5 + c];
                    const unsigned int b = (unsigned int)(w >> 32);
                    if (b != SHOT_NO_BIN && (b & 63u) == l) hist[b] += __uint_as_float((unsigned int)w);
                }
            }
            wave_lds_sync();
            if (__ballot(past)) break;  // (the row is ascending: the prefix with d2 < r2 has ended)
        }
        const bool nan_row = !frame || row_len < (unsigned int)SHOT_MIN_NEIGHBOURS;
        const float norm = nan_row ? 1.f : shot_norm(hist);
        const unsigned int at = pos[i];
        for (unsigned int b = l; b < (unsigned int)SHOT_BINS; b += 64) out_desc[(size_t)at * SHOT_BINS + b] = nan_row ? shot_nan() : hist[b] / norm;
        if (out_rf && l < 9) out_rf[(size_t)at * 9 + l] = rf_in[(size_t)i * 9 + l];
        if (l == 0) out_index[at] = (int32_t)i;
    }
}

// the stages over the indexed cloud of ix: out_desc[n * 352], out_rf[n * 9] (nullable), out_index[n] on the device; *n_out on the
// host.  Waits: the totals of the CSRs (one when shot_radius <= normal_radius) and, at the end, the count.
int shot_descriptors(pcc_index* ix, double normal_radius, double shot_radius, float* out_desc, float* out_rf, int32_t* out_index, size_t* n_out) {
    hipStream_t s = ix->stream;
    ShotScratch* r = scratch<ShotScratch>(ix);
    const size_t n = ix->n_orig;
    const unsigned int un = (unsigned int)n;
    const float origin[3] = {0.f, 0.f, 0.f};
    const float4* refs = ix->refs.as<float4>();
    const float4* cell_refs = ix->cell_refs.as<float4>();
    const GridDev* gd = ix->d_grid.as<GridDev>();
    PCC_TRY(r->normals.reserve(n * sizeof(float4)));
    PCC_TRY(r->rf.reserve(n * 9 * sizeof(float)));
    PCC_TRY(r->flags.reserve(n * sizeof(unsigned int)));
    PCC_TRY(r->pos.reserve((n + 1) * sizeof(unsigned int)));
    const unsigned int blocks = blocks_for(n);
    // rows at normal_radius: the plane fit; cloud2 and the place of each of its points in the output
    const unsigned long long* keys = nullptr;
    const unsigned int* off32 = nullptr;
    PCC_TRY(radius_csr(ix, normal_radius, &keys, &off32));
    PCC_TRY(launch_normals_csr(s, refs, cell_refs, gd, n, keys, off32, origin, r->normals.as<float4>()));
    PCC_HIP(hipMemsetAsync(r->pos.as<unsigned int>() + n, 0, sizeof(unsigned int), s));
    hipLaunchKernelGGL(k_shot_flags, dim3(blocks), dim3(256), 0, s, r->normals.as<float4>(), un, r->flags.as<unsigned int>(), r->pos.as<unsigned int>());
    PCC_HIP(hipGetLastError());
    PCC_TRY(launch_exclusive_scan(ix, s, r->pos.as<unsigned int>(), n + 1, r->scan_tmp));
    // rows at shot_radius: a prefix of the rows above when it is not the larger radius, else a CSR of their own
    if (shot_radius > normal_radius) PCC_TRY(radius_csr(ix, shot_radius, &keys, &off32));
    const float r2 = radius2(shot_radius);
    const unsigned int wb = (unsigned int)std::min<size_t>((n + 3) / 4, 8192);
    ev_mark(ix, EV_MAIN0);
    hipLaunchKernelGGL(k_shot_lrf64, dim3(wb), dim3(256), 0, s, keys, off32, refs, r->flags.as<unsigned int>(), cell_refs, gd, r2, shot_radius,
                       r->rf.as<float>());
    PCC_HIP(hipGetLastError());
    ev_mark(ix, EV_MAIN1);
    ev_mark(ix, EV_FB0);
    hipLaunchKernelGGL(k_shot_desc64, dim3(wb), dim3(256), 0, s, keys, off32, refs, r->normals.as<float4>(), r->flags.as<unsigned int>(),
                       r->pos.as<unsigned int>(), r->rf.as<float>(), cell_refs, gd, r2, shot_radius, out_desc, out_rf, out_index);
    PCC_HIP(hipGetLastError());
    ev_mark(ix, EV_FB1);
    unsigned int kept = 0;
    PCC_TRY(read_back(ix, r->pos.as<unsigned int>() + n, &kept));
    *n_out = kept;
    return PCC_OK;
}

}  // namespace

}  // namespace pcc

using namespace pcc;
extern "C" {
int pcc_shot_descriptors(pcc_index* ix, int mem, double normal_radius, double shot_radius, float* out_descriptors, float* out_rf,
                         int32_t* out_point_index, size_t* n_out) {
    // the arguments first: host arithmetic, refused before any device is looked at
    PCC_TRY(check_mem(mem));
    if (!out_descriptors || !out_point_index || !n_out) { set_error("null argument"); return PCC_ERR_INVALID; }
    for (double radius : {normal_radius, shot_radius})
        if (!(radius > 0) || !std::isfinite(radius)) { set_error("bad radius"); return PCC_ERR_INVALID; }
    PCC_ENTER(ix);
    PCC_TRY(ensure_grid(ix));
    ev_next(ix);
    ev_mark(ix, EV_CALL0);
    const size_t n = ix->n_orig;
    ShotScratch* r = scratch<ShotScratch>(ix);
    Out<float> rd, rr;
    Out<int32_t> ri;
    PCC_TRY(rd.stage(out_descriptors, n * SHOT_BINS, mem, r->out_desc));
    if (out_rf) PCC_TRY(rr.stage(out_rf, n * 9, mem, r->out_rf));
    PCC_TRY(ri.stage(out_point_index, n, mem, r->out_index));
    size_t kept = 0;
    PCC_TRY(shot_descriptors(ix, normal_radius, shot_radius, rd.dev, rr.dev, ri.dev, &kept));
    *n_out = kept;
    rd.count = kept * SHOT_BINS;  // (only the rows that were written travel)
    rr.count = out_rf ? kept * 9 : 0;
    ri.count = kept;
    ev_mark(ix, EV_CALL1);
    return finish(ix, mem, rd, rr, ri);
}
}  // extern "C"
