// fpfh.hip -- the FPFH descriptor pipeline of ONE cloud (gfx950): pcc_fpfh_descriptors.
// replaces: processFPFH (reference src/comparator.cpp:824-875): pcl::NormalEstimation (setRadiusSearch 0.03),
//   removeNaNNormalsFromPointCloud, pcl::FPFHEstimation (setRadiusSearch 0.05, 11 + 11 + 11 bins).
//
// Both stages of FPFHEstimation consume the sorted radius rows of the indexed cloud at fpfh_radius (CSR of u64 keys, d2 bits << 32
// | point index, ascending); the rows at normal_radius feed the plane fit (normals.hip).  As in rift.hip the compaction is not
// carried out in front: cloud2 (the points with a finite normal) is a subset in the same order, so a row of cloud2 is the row of
// the whole cloud with the others skipped -- the consumers mask.  The positions of cloud2's points (an exclusive scan of the
// flags) are known before the descriptors are, so the weighting kernel writes every descriptor where it belongs in the output.
// The arithmetic is fpfh_math.hpp's, shared with the host mirror of the tests: same operations, same order, same bits.
#include <algorithm>

#include "entry.hpp"
#include "lane_ops.hpp"
#include "grid_device.hpp"
#include "fpfh_math.hpp"

namespace pcc {

namespace {

// What pcc_fpfh_descriptors keeps between its stages.  Buffers of their own, as RiftScratch's: the radius searches in between
// use the handle's shared scratch.
struct FpfhScratch : Scratch {
    static constexpr ScratchSlot slot = SCRATCH_FPFH;
    DevBuf normals;              // float4[n] plane fit
    DevBuf spfh;                 // float[n][33]: the SPFH signature of every point of cloud2 (the others are never read)
    DevBuf flags, pos, scan_tmp; // uint32[n]: 1 for the points of cloud2; uint32[n + 1]: their exclusive scan, pos[n] = the count
    DevBuf out_hist, out_index;  // results staged for a caller in host memory
};

// flags[i] = 1 for the points of cloud2 (every component of the normal finite); pos = the same, to be scanned
__global__ void __launch_bounds__(256)
k_fpfh_flags(const float4* __restrict__ normals, unsigned int n, unsigned int* __restrict__ flags, unsigned int* __restrict__ pos) {
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 nv = normals[i];
        const unsigned int in2 = fpfh_finite(nv.x) && fpfh_finite(nv.y) && fpfh_finite(nv.z) ? 1u : 0u;
        flags[i] = in2;
        pos[i] = in2;
    }
}

// the three bins one row entry votes into, packed b1 | b2 << 8 | b3 << 16; FPFH_NO_VOTE for the point itself and for "no pair"
constexpr unsigned int FPFH_NO_VOTE = 0xffffffffu;
__device__ __forceinline__ unsigned int fpfh_entry(const float4 p0, const float4 n0, unsigned int i, unsigned int j, const float4 nq,
                                                   const float4* __restrict__ refs) {
    if (j == i) return FPFH_NO_VOTE;
    const float4 q = refs[j];
    const float a[3] = {p0.x, p0.y, p0.z}, an[3] = {n0.x, n0.y, n0.z}, b[3] = {q.x, q.y, q.z}, bn[3] = {nq.x, nq.y, nq.z};
    const FpfhPair f = fpfh_pair(a, an, b, bn);
    if (!f.ok) return FPFH_NO_VOTE;
    return (unsigned int)fpfh_bin_f1(f.f1) | ((unsigned int)fpfh_bin_f23(f.f2) << 8) | ((unsigned int)fpfh_bin_f23(f.f3) << 16);
}

// computePointSPFHSignature, a wave per row (four rows per workgroup), rows in cell order.  Per chunk of 64 row entries every
// lane makes the two gathers of ONE entry and evaluates its pair features (a square root, the divisions, acosf twice, atan2f);
// the votes are counted in integers in LDS -- every vote of a row adds the same increment, so a bin's float is a function of its
// count alone -- and the entries of cloud2 by a ballot.  Lane b < 33 then rebuilds bin b: the increment added count times.
__global__ void __launch_bounds__(256)
k_fpfh_spfh64(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ offsets, const float4* __restrict__ refs,
              const float4* __restrict__ normals, const unsigned int* __restrict__ flags, const float4* __restrict__ cell_refs,
              const GridDev* __restrict__ gd, float* __restrict__ spfh) {
    __shared__ unsigned int counts_all[4][FPFH_BINS];
    const unsigned int l = threadIdx.x & 63;
    unsigned int* counts = counts_all[threadIdx.x >> 6];
    const unsigned int n_valid = gd->n_valid;
    const unsigned int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (unsigned int t = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; t < n_valid; t += nwaves) {
        const unsigned int i = (unsigned int)__float_as_int(cell_refs[t].w);
        if (!flags[i]) continue;  // (the wave's: not in cloud2)
        const unsigned int beg = offsets[i], end = offsets[i + 1];
        const float4 p0 = refs[i], n0 = normals[i];
        wave_lds_sync();
        if (l < FPFH_BINS) counts[l] = 0u;
        wave_lds_sync();
        unsigned int row_len = 0;
        for (unsigned int e0 = beg; e0 < end; e0 += 64) {
            const unsigned int e = e0 + l;
            bool in2 = false;
            if (e < end) {
                const unsigned int j = (unsigned int)keys[e];
                in2 = flags[j] != 0u;
                if (in2) {
                    const unsigned int v = fpfh_entry(p0, n0, i, j, normals[j], refs);
                    if (v != FPFH_NO_VOTE) {
                        atomicAdd(&counts[v & 255u], 1u);
                        atomicAdd(&counts[FPFH_F_BINS + ((v >> 8) & 255u)], 1u);
                        atomicAdd(&counts[2 * FPFH_F_BINS + (v >> 16)], 1u);
                    }
                }
            }
            row_len += (unsigned int)__popcll(__ballot(in2));
        }
        wave_lds_sync();
        if (l < FPFH_BINS) spfh[(size_t)i * FPFH_BINS + l] = fpfh_spfh_value(counts[l], fpfh_incr(row_len));
    }
}

// the same, one lane per row (the baseline the layout above is measured against, PCC_OPT_FPFH_LAYOUT = 0): PCL's loop as it
// stands, the 33 counters of every lane in LDS (bin-major: lanes of a wave touch consecutive words)
__global__ void __launch_bounds__(256)
k_fpfh_spfh1(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ offsets, const float4* __restrict__ refs,
             const float4* __restrict__ normals, const unsigned int* __restrict__ flags, const float4* __restrict__ cell_refs,
             const GridDev* __restrict__ gd, float* __restrict__ spfh) {
    __shared__ unsigned int cs[FPFH_BINS][256];
    const unsigned int n_valid = gd->n_valid;
    for (unsigned int t = blockIdx.x * blockDim.x + threadIdx.x; t < n_valid; t += gridDim.x * blockDim.x) {
        const unsigned int i = (unsigned int)__float_as_int(cell_refs[t].w);
        if (!flags[i]) continue;
        const unsigned int beg = offsets[i], end = offsets[i + 1];
        const float4 p0 = refs[i], n0 = normals[i];
        for (int k = 0; k < FPFH_BINS; ++k) cs[k][threadIdx.x] = 0u;
        unsigned int row_len = 0;
        for (unsigned int e = beg; e < end; ++e) {
            const unsigned int j = (unsigned int)keys[e];
            if (!flags[j]) continue;
            ++row_len;
            const unsigned int v = fpfh_entry(p0, n0, i, j, normals[j], refs);
            if (v == FPFH_NO_VOTE) continue;
            cs[v & 255u][threadIdx.x] += 1u;
            cs[FPFH_F_BINS + ((v >> 8) & 255u)][threadIdx.x] += 1u;
            cs[2 * FPFH_F_BINS + (v >> 16)][threadIdx.x] += 1u;
        }
        const float incr = fpfh_incr(row_len);
        for (int k = 0; k < FPFH_BINS; ++k) spfh[(size_t)i * FPFH_BINS + k] = fpfh_spfh_value(cs[k][threadIdx.x], incr);
    }
}

// weightPointSPFHSignature, a wave per row, rows in cell order.  Per chunk of 64 row entries every lane reads ONE key and
// takes its weight (the division); then the wave walks the entries that count in row order: lane b < 33 owns bin b and adds
// spfh[q][b] * w to it, so every bin accumulates in the row's order and no two lanes add to the same word.  The three running
// sums are chains over entry-major, bin-minor terms: lanes 33, 34 and 35 carry one each and collect the eleven terms of
// their feature from the owner lanes, entry by entry -- beside the bins, not in front of them.  The descriptor goes to row
// pos[i] of the output.
__global__ void __launch_bounds__(256)
k_fpfh_weight64(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ offsets, const float* __restrict__ spfh,
                const unsigned int* __restrict__ flags, const unsigned int* __restrict__ pos, const float4* __restrict__ cell_refs,
                const GridDev* __restrict__ gd, float* __restrict__ out_hist, int32_t* __restrict__ out_index) {
    const unsigned int l = threadIdx.x & 63;
    const unsigned int n_valid = gd->n_valid;
    const unsigned int nwaves = (gridDim.x * blockDim.x) >> 6;
    const bool owner = l < FPFH_BINS;
    const unsigned int chain = l - FPFH_BINS;  // 0, 1, 2 on the lanes that carry a running sum
    const int first = chain < 3u ? (int)chain * FPFH_F_BINS : 0;
    for (unsigned int t = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; t < n_valid; t += nwaves) {
        const unsigned int i = (unsigned int)__float_as_int(cell_refs[t].w);
        if (!flags[i]) continue;  // (the wave's)
        const unsigned int beg = offsets[i], end = offsets[i + 1];
        float acc = 0.f, sum = 0.f;
        for (unsigned int e0 = beg; e0 < end; e0 += 64) {
            const unsigned int e = e0 + l;
            unsigned int j = 0;
            float w = 0.f;
            bool use = false;
            if (e < end) {
                const unsigned long long key = keys[e];
                j = (unsigned int)key;
                const float d2 = __uint_as_float((unsigned int)(key >> 32));
                use = flags[j] != 0u && d2 != 0.f;
                if (use) w = fpfh_weight(d2);
            }
            unsigned long long todo = __ballot(use);
            while (todo) {
                const int k = __builtin_ctzll(todo);
                todo &= todo - 1;
                const unsigned int jk = (unsigned int)__builtin_amdgcn_readlane((int)j, k);
                const float wk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), k));
                const float val = owner ? spfh[(size_t)jk * FPFH_BINS + l] * wk : 0.f;
                acc += val;
                for (int b = 0; b < FPFH_F_BINS; ++b) sum += __shfl(val, first + b, 64);
            }
        }
        // every bin times the factor of its feature
        const float factor = fpfh_norm_factor(sum);
        const float mine = __shfl(factor, FPFH_BINS + (owner ? (int)l / FPFH_F_BINS : 0), 64);
        const unsigned int at = pos[i];
        if (owner) out_hist[(size_t)at * FPFH_BINS + l] = acc * mine;
        if (l == 0) out_index[at] = (int32_t)i;
    }
}

// the same, one lane per row (PCC_OPT_FPFH_LAYOUT = 0): PCL's loop as it stands, the 33 bins in registers
__global__ void __launch_bounds__(256)
k_fpfh_weight1(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ offsets, const float* __restrict__ spfh,
               const unsigned int* __restrict__ flags, const unsigned int* __restrict__ pos, const float4* __restrict__ cell_refs,
               const GridDev* __restrict__ gd, float* __restrict__ out_hist, int32_t* __restrict__ out_index) {
    const unsigned int n_valid = gd->n_valid;
    for (unsigned int t = blockIdx.x * blockDim.x + threadIdx.x; t < n_valid; t += gridDim.x * blockDim.x) {
        const unsigned int i = (unsigned int)__float_as_int(cell_refs[t].w);
        if (!flags[i]) continue;
        const unsigned int beg = offsets[i], end = offsets[i + 1];
        float acc[FPFH_BINS], sum[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < FPFH_BINS; ++k) acc[k] = 0.f;
        for (unsigned int e = beg; e < end; ++e) {
            const unsigned long long key = keys[e];
            const unsigned int j = (unsigned int)key;
            const float d2 = __uint_as_float((unsigned int)(key >> 32));
            if (!flags[j] || d2 == 0.f) continue;
            const float w = fpfh_weight(d2);
            const float* row = spfh + (size_t)j * FPFH_BINS;
#pragma unroll
            for (int f = 0; f < 3; ++f)
#pragma unroll
                for (int b = 0; b < FPFH_F_BINS; ++b) {
                    const float val = row[f * FPFH_F_BINS + b] * w;
                    sum[f] += val;
                    acc[f * FPFH_F_BINS + b] += val;
                }
        }
        const unsigned int at = pos[i];
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            const float factor = fpfh_norm_factor(sum[f]);
#pragma unroll
            for (int b = 0; b < FPFH_F_BINS; ++b) out_hist[(size_t)at * FPFH_BINS + f * FPFH_F_BINS + b] = acc[f * FPFH_F_BINS + b] * factor;
        }
        out_index[at] = (int32_t)i;
    }
}

}  // namespace

int check_fpfh_params(double normal_radius, double fpfh_radius, int nr_bins_f1, int nr_bins_f2, int nr_bins_f3) {
    for (double r : {normal_radius, fpfh_radius})
        if (!(r > 0) || !std::isfinite(r)) { set_error("bad radius"); return PCC_ERR_INVALID; }
    if (nr_bins_f1 != FPFH_F_BINS || nr_bins_f2 != FPFH_F_BINS || nr_bins_f3 != FPFH_F_BINS) {
        set_error("FPFH with %d + %d + %d bins: only 11 + 11 + 11 bins are built", nr_bins_f1, nr_bins_f2, nr_bins_f3);
        return PCC_ERR_UNSUPPORTED;
    }
    return PCC_OK;
}

// The stages over any packed cloud -- the indexed cloud of a handle, or the concatenation of a batch (fpfh_batch.hip): refs[n],
// `order` a cell_refs-shaped array whose first gd->n_valid entries name the points to take (their w), `rows` the sorted radius
// rows of that cloud as a CSR.  normals (nullable): the caller fits the planes itself -- it fills normals[n] and hands over the
// CSR at fpfh_radius, and `rows` is not asked.  out_hist[n * 33], out_index[n] on the device; *pos_out: uint32[n + 1] on the
// device, the exclusive scan of the flags of cloud2, pos[n] = the rows written.  Waits: the totals of the CSRs.
int fpfh_stages(pcc_index* ix, const float4* refs, const float4* cell_refs, const GridDev* gd, size_t n, const RiftRows& rows,
                double normal_radius, double fpfh_radius, const FpfhNormals* normals, float* out_hist, int32_t* out_index,
                const unsigned int** pos_out) {
    hipStream_t s = ix->stream;
    FpfhScratch* r = scratch<FpfhScratch>(ix);
    const unsigned int un = (unsigned int)n;
    const float origin[3] = {0.f, 0.f, 0.f};
    PCC_TRY(r->normals.reserve(n * sizeof(float4)));
    PCC_TRY(r->spfh.reserve(n * FPFH_BINS * sizeof(float)));
    PCC_TRY(r->flags.reserve(n * sizeof(unsigned int)));
    PCC_TRY(r->pos.reserve((n + 1) * sizeof(unsigned int)));
    const unsigned int blocks = blocks_for(n);
    // rows at normal_radius: the plane fit; cloud2 and the place of each of its points in the output
    const unsigned long long* keys = nullptr;
    const unsigned int* off32 = nullptr;
    if (normals) {
        PCC_TRY((*normals)(r->normals.as<float4>(), &keys, &off32));
    } else {
        PCC_TRY(rows(normal_radius, &keys, &off32));
        PCC_TRY(launch_normals_csr(s, refs, cell_refs, gd, n, keys, off32, origin, r->normals.as<float4>()));
    }
    PCC_HIP(hipMemsetAsync(r->pos.as<unsigned int>() + n, 0, sizeof(unsigned int), s));
    hipLaunchKernelGGL(k_fpfh_flags, dim3(blocks), dim3(256), 0, s, r->normals.as<float4>(), un, r->flags.as<unsigned int>(), r->pos.as<unsigned int>());
    PCC_HIP(hipGetLastError());
    PCC_TRY(launch_exclusive_scan(ix, s, r->pos.as<unsigned int>(), n + 1, r->scan_tmp));
    // rows at fpfh_radius (same radius: same rows): the SPFH signatures, then their weighted sums
    if (!normals && fpfh_radius != normal_radius) PCC_TRY(rows(fpfh_radius, &keys, &off32));
    const unsigned int wb = (unsigned int)std::min<size_t>((n + 3) / 4, 8192);
    ev_mark(ix, EV_MAIN0);
    if (ix->opt.fpfh_layout == 1) {
        hipLaunchKernelGGL(k_fpfh_spfh64, dim3(wb), dim3(256), 0, s, keys, off32, refs, r->normals.as<float4>(), r->flags.as<unsigned int>(), cell_refs, gd,
                           r->spfh.as<float>());
    } else {
        hipLaunchKernelGGL(k_fpfh_spfh1, dim3(blocks), dim3(256), 0, s, keys, off32, refs, r->normals.as<float4>(), r->flags.as<unsigned int>(), cell_refs, gd,
                           r->spfh.as<float>());
    }
    PCC_HIP(hipGetLastError());
    ev_mark(ix, EV_MAIN1);
    ev_mark(ix, EV_FB0);
    if (ix->opt.fpfh_layout == 1) {
        hipLaunchKernelGGL(k_fpfh_weight64, dim3(wb), dim3(256), 0, s, keys, off32, r->spfh.as<float>(), r->flags.as<unsigned int>(), r->pos.as<unsigned int>(),
                           cell_refs, gd, out_hist, out_index);
    } else {
        hipLaunchKernelGGL(k_fpfh_weight1, dim3(blocks), dim3(256), 0, s, keys, off32, r->spfh.as<float>(), r->flags.as<unsigned int>(), r->pos.as<unsigned int>(),
                           cell_refs, gd, out_hist, out_index);
    }
    PCC_HIP(hipGetLastError());
    ev_mark(ix, EV_FB1);
    *pos_out = r->pos.as<unsigned int>();
    return PCC_OK;
}

namespace {

// the stages over the indexed cloud of ix: out_hist[n * 33], out_index[n] on the device; *n_out on
// the host.  Waits: the totals of the CSRs and, at the end, the count.
int fpfh_descriptors(pcc_index* ix, double normal_radius, double fpfh_radius, float* out_hist, int32_t* out_index, size_t* n_out) {
    const size_t n = ix->n_orig;
    const RiftRows rows = [ix](double radius, const unsigned long long** keys, const unsigned int** offsets) -> int {
        return radius_csr(ix, radius, keys, offsets);
    };
    const unsigned int* pos = nullptr;
    PCC_TRY(fpfh_stages(ix, ix->refs.as<float4>(), ix->cell_refs.as<float4>(), ix->d_grid.as<GridDev>(), n, rows, normal_radius, fpfh_radius, nullptr,
                        out_hist, out_index, &pos));
    unsigned int kept = 0;
    PCC_TRY(read_back(ix, pos + n, &kept));
    *n_out = kept;
    return PCC_OK;
}

}  // namespace

}  // namespace pcc

using namespace pcc;
extern "C" {
int pcc_fpfh_descriptors(pcc_index* ix, int mem, double normal_radius, double fpfh_radius, int nr_bins_f1, int nr_bins_f2, int nr_bins_f3,
                         float* out_hist, int32_t* out_index, size_t* n_out) {
    // the arguments first: host arithmetic, refused before any device is looked at
    PCC_TRY(check_mem(mem));
    if (!out_hist || !out_index || !n_out) { set_error("null argument"); return PCC_ERR_INVALID; }
    PCC_TRY(check_fpfh_params(normal_radius, fpfh_radius, nr_bins_f1, nr_bins_f2, nr_bins_f3));
    PCC_ENTER(ix);
    PCC_TRY(ensure_grid(ix));
    ev_next(ix);
    ev_mark(ix, EV_CALL0);
    const size_t n = ix->n_orig;
    FpfhScratch* r = scratch<FpfhScratch>(ix);
    Out<float> rh;
    Out<int32_t> ri;
    PCC_TRY(rh.stage(out_hist, n * FPFH_BINS, mem, r->out_hist));
    PCC_TRY(ri.stage(out_index, n, mem, r->out_index));
    size_t kept = 0;
    PCC_TRY(fpfh_descriptors(ix, normal_radius, fpfh_radius, rh.dev, ri.dev, &kept));
    *n_out = kept;
    rh.count = kept * FPFH_BINS;  // (only the rows that were written travel)
    ri.count = kept;
    ev_mark(ix, EV_CALL1);
    return finish(ix, mem, rh, ri);
}
}  // extern "C"
