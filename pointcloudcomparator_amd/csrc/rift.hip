// rift.hip -- the RIFT descriptor pipeline of ONE cloud (gfx950): pcc_rift_descriptors.
// replaces: the middle of processRIFT (reference src/comparator.cpp:590-684): pcl::PointCloudXYZRGBtoXYZI,
//   pcl::NormalEstimation (setRadiusSearch 0.03), removeNaNNormalsFromPointCloud, pcl::IntensityGradientEstimation
//   (0.03), pcl::RIFTEstimation (0.05, 4 distance x 8 gradient bins) and the removal of non-finite descriptors.
//
// Every stage consumes sorted radius rows of the indexed cloud (CSR of u64 keys, d2 bits << 32 | point index, ascending):
// the r = normal_radius rows feed the plane fit (normals.hip) and, when gradient_radius is the same, the intensity
// gradient; the r = rift_radius rows feed the histogram.  The first compaction is not carried out: cloud2 (the points
// with a finite normal) is a subset in the same order, so a row of cloud2 is the row of the whole cloud with the
// others skipped -- the consumers mask.  Only the final compaction moves data (flags, exclusive scan, scatter).
// The arithmetic is rift_math.hpp's, shared with the host mirror of the tests: same operations, same order, same bits.
#include <algorithm>

#include "entry.hpp"
#include "lane_ops.hpp"
#include "grid_device.hpp"
#include "rift_math.hpp"

namespace pcc {

namespace {

// intensity of every point with a finite normal; NaN marks the points that are not in cloud2 (no row entry of the
// gradient stage needs a second gather to find that out)
__global__ void __launch_bounds__(256)
k_rift_intensity(const unsigned char* __restrict__ rgb, size_t stride, const float4* __restrict__ normals, unsigned int n,
                 float* __restrict__ inten) {
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 nv = normals[i];
        const bool in2 = rift_finite(nv.x) && rift_finite(nv.y) && rift_finite(nv.z);
        const uint32_t c = *reinterpret_cast<const uint32_t*>(rgb + (size_t)i * stride);
        inten[i] = in2 ? rift_intensity(c) : __uint_as_float(0x7fc00000u);
    }
}

// IntensityGradientEstimation: one lane per point of cloud2, in cell order (neighbouring lanes gather neighbouring
// points).  Two walks over the row: centroid and mean intensity, then the normal equations.  grad[i] = (gx, gy, gz, 1);
// the buffer is zeroed in front, so w = 0 marks the points outside cloud2.
__global__ void __launch_bounds__(256)
k_rift_gradient(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ offsets,
                const float4* __restrict__ refs, const float* __restrict__ inten, const float4* __restrict__ normals,
                const float4* __restrict__ cell_refs, const GridDev* __restrict__ gd, float4* __restrict__ grad) {
    const float qnan = __uint_as_float(0x7fc00000u);
    const unsigned int n_valid = gd->n_valid;
    for (unsigned int t = blockIdx.x * blockDim.x + threadIdx.x; t < n_valid; t += gridDim.x * blockDim.x) {
        const unsigned int i = (unsigned int)__float_as_int(cell_refs[t].w);
        if (inten[i] != inten[i]) continue;  // not in cloud2
        const unsigned int beg = offsets[i], end = offsets[i + 1];
        float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;
        unsigned int cnt = 0;
        for (unsigned int k = beg; k < end; ++k) {
            const unsigned int j = (unsigned int)keys[k];
            const float v = inten[j];
            if (v != v) continue;
            const float4 p = refs[j];
            sx += p.x; sy += p.y; sz += p.z; si += v;
            ++cnt;
        }
        if (cnt < 3) { grad[i] = make_float4(qnan, qnan, qnan, 1.0f); continue; }
        const float fc = (float)cnt, cx = sx / fc, cy = sy / fc, cz = sz / fc, mi = si / fc;
        float a[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0}, x[3], g[3];
        for (unsigned int k = beg; k < end; ++k) {
            const unsigned int j = (unsigned int)keys[k];
            const float v = inten[j];
            if (v != v) continue;
            const float4 p = refs[j];
            const float px = p.x - cx, py = p.y - cy, pz = p.z - cz, di = v - mi;
            a[0] += px * px; a[1] += px * py; a[2] += px * pz; a[3] += py * py; a[4] += py * pz; a[5] += pz * pz;
            b[0] += px * di; b[1] += py * di; b[2] += pz * di;
        }
        rift_solve3(a, b, x);
        const float4 nv = normals[i];
        const float nn[3] = {nv.x, nv.y, nv.z};
        rift_project(nn, x, g);
        grad[i] = make_float4(g[0], g[1], g[2], 1.0f);
    }
}

// the vote of one row entry, or nothing (w = 0 entries are outside cloud2); ranges packed into one word:
// d_lo | d_hi << 4 | (g_lo + 1) << 8 | (g_hi + 1) << 16 (g_lo >= -1), an empty d range for "no entry"
__device__ __forceinline__ float4 rift_entry(const float4 p0, unsigned long long key, const float4* __restrict__ refs,
                                             const float4* __restrict__ grad, float radius) {
    const unsigned int j = (unsigned int)key;
    const float4 gv = grad[j];
    if (gv.w != 1.0f) return make_float4(0.f, 0.f, 0.f, __uint_as_float(1u));  // d_lo = 1, d_hi = 0
    const float4 p = refs[j];
    const float a0[3] = {p0.x, p0.y, p0.z}, a[3] = {p.x, p.y, p.z}, g[3] = {gv.x, gv.y, gv.z};
    const RiftVote v = rift_vote(a0, a, g, __uint_as_float((unsigned int)(key >> 32)), radius);
    int d_lo, d_hi, g_lo, g_hi;
    rift_vote_range(v, &d_lo, &d_hi, &g_lo, &g_hi);
    // (d_hi < 0 cannot happen: d >= 0; an empty range stays empty in the packed form as long as d_lo > d_hi)
    const unsigned int w = (unsigned int)d_lo | ((unsigned int)max(d_hi, 0) << 4) | ((unsigned int)(g_lo + 1) << 8) | ((unsigned int)(g_hi + 1) << 16);
    return make_float4(v.d, v.g, v.mag, __uint_as_float(d_lo > d_hi ? 1u : w));
}

// RIFTEstimation, 32 lanes per row (two rows per wave, eight per workgroup), rows in cell order.
// Per chunk of 32 row entries: every lane computes ONE entry's vote (gathers, two square roots, the divisions, acosf) and
// leaves it in LDS; then every lane, as the owner of bin (d = lane & 3, g = lane >> 2 & 7), walks the 32 votes in row
// order and adds the share its bin receives -- the order of additions per bin is the row's, as in PCL's loop, and no
// two lanes ever add to the same word.  hist[i * 32 + bin] for every point of cloud2; keep[i] = its first bin is finite.
__global__ void __launch_bounds__(256)
k_rift_rows32(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ offsets,
              const float4* __restrict__ refs, const float4* __restrict__ grad, const float4* __restrict__ cell_refs,
              const GridDev* __restrict__ gd, float radius, float* __restrict__ hist, unsigned int* __restrict__ keep) {
    __shared__ float4 votes_all[8][32];
    const unsigned int l = threadIdx.x & 31, grp = threadIdx.x >> 5;
    float4* votes = votes_all[grp];
    const int db = (int)(l & 3), gb = (int)(l >> 2);
    const unsigned int n_valid = gd->n_valid;
    const unsigned int ngroups = (gridDim.x * blockDim.x) >> 5;
    // (the trip count is the wave's: both halves stay in step so that wave_lds_sync is reached together)
    for (unsigned int t0 = ((blockIdx.x * blockDim.x + threadIdx.x) >> 6) * 2; t0 < n_valid; t0 += ngroups) {
        const unsigned int t = t0 + (grp & 1);
        unsigned int i = 0, beg = 0, end = 0;
        float4 p0 = make_float4(0.f, 0.f, 0.f, 0.f);
        bool have = false;
        if (t < n_valid) {
            i = (unsigned int)__float_as_int(cell_refs[t].w);
            have = grad[i].w == 1.0f;
            if (have) { beg = offsets[i]; end = offsets[i + 1]; p0 = refs[i]; }
        }
        float h = 0.f;
        const unsigned int len = end - beg;
        const unsigned int other = (unsigned int)__shfl_xor((int)len, 32, 64);
        const unsigned int trips = (max(len, other) + 31) / 32;
        for (unsigned int c = 0; c < trips; ++c) {
            const unsigned int e = c * 32 + l;
            wave_lds_sync();
            votes[l] = e < len ? rift_entry(p0, keys[beg + e], refs, grad, radius) : make_float4(0.f, 0.f, 0.f, __uint_as_float(1u));
            wave_lds_sync();
            const unsigned int m = min(32u, len > c * 32 ? len - c * 32 : 0u);
            for (unsigned int k = 0; k < m; ++k) {
                const float4 q = votes[k];
                const unsigned int w = __float_as_uint(q.w);
                const int d_lo = (int)(w & 15u), d_hi = (int)((w >> 4) & 15u), g_lo = (int)((w >> 8) & 255u) - 1, g_hi = (int)(w >> 16) - 1;
                int gi = gb;  // the one g_idx of [g_lo, g_hi] (at most three values of -1 .. 9) that wraps to this lane's bin
                if (gi > g_hi) gi -= RIFT_G_BINS;
                else if (gi < g_lo) gi += RIFT_G_BINS;
                if (db >= d_lo && db <= d_hi && gi >= g_lo && gi <= g_hi) {
                    const RiftVote v = {q.x, q.y, q.z};
                    h += rift_vote_term(v, db, gi);
                }
            }
        }
        // normalise: bin (d, g) is word g * 4 + d of the output, which is this lane's number
        wave_lds_sync();
        votes[l].x = h;
        wave_lds_sync();
        const float nr = rift_norm(&votes[0].x, 4);
        const float o = h / nr;
        if (have) {
            hist[(size_t)i * RIFT_BINS + l] = o;
            if (l == 0) keep[i] = rift_finite(o) ? 1u : 0u;
        }
    }
}

// the same, one lane per row (the baseline the layout above is measured against, PCC_OPT_RIFT_LAYOUT = 0): PCL's loop as
// it stands, the 32 bins of every lane in LDS (bin-major: lanes of a wave touch consecutive words)
__global__ void __launch_bounds__(256)
k_rift_rows1(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ offsets,
             const float4* __restrict__ refs, const float4* __restrict__ grad, const float4* __restrict__ cell_refs,
             const GridDev* __restrict__ gd, float radius, float* __restrict__ hist, unsigned int* __restrict__ keep) {
    __shared__ float hs[RIFT_BINS][256];
    const unsigned int n_valid = gd->n_valid;
    for (unsigned int t = blockIdx.x * blockDim.x + threadIdx.x; t < n_valid; t += gridDim.x * blockDim.x) {
        const unsigned int i = (unsigned int)__float_as_int(cell_refs[t].w);
        if (grad[i].w != 1.0f) continue;
        const unsigned int beg = offsets[i], end = offsets[i + 1];
        const float4 p0 = refs[i];
        for (int k = 0; k < RIFT_BINS; ++k) hs[k][threadIdx.x] = 0.f;
        for (unsigned int e = beg; e < end; ++e) {
            const float4 q = rift_entry(p0, keys[e], refs, grad, radius);
            const unsigned int w = __float_as_uint(q.w);
            const int d_lo = (int)(w & 15u), d_hi = (int)((w >> 4) & 15u), g_lo = (int)((w >> 8) & 255u) - 1, g_hi = (int)(w >> 16) - 1;
            if (d_lo > d_hi) continue;
            const RiftVote v = {q.x, q.y, q.z};
            for (int g = g_lo; g <= g_hi; ++g)
                for (int d = d_lo; d <= d_hi; ++d) hs[((g + RIFT_G_BINS) % RIFT_G_BINS) * RIFT_D_BINS + d][threadIdx.x] += rift_vote_term(v, d, g);
        }
        const float nr = rift_norm(&hs[0][threadIdx.x], 256);
        float first = 0.f;
        for (int k = 0; k < RIFT_BINS; ++k) {
            const float o = hs[k][threadIdx.x] / nr;
            hist[(size_t)i * RIFT_BINS + k] = o;
            if (k == 0) first = o;
        }
        keep[i] = rift_finite(first) ? 1u : 0u;
    }
}

// second compaction: pos = exclusive scan of keep (pos[n] = the count); kept rows move to the front, in index order
__global__ void __launch_bounds__(256)
k_rift_compact(const float* __restrict__ hist, const unsigned int* __restrict__ pos, unsigned int n,
               float* __restrict__ out_hist, int32_t* __restrict__ out_index) {
    const unsigned int l = threadIdx.x & 31;
    const unsigned int ngroups = (gridDim.x * blockDim.x) >> 5;
    for (unsigned int i = (blockIdx.x * blockDim.x + threadIdx.x) >> 5; i < n; i += ngroups) {
        const unsigned int at = pos[i];
        if (pos[i + 1] == at) continue;
        out_hist[(size_t)at * RIFT_BINS + l] = hist[(size_t)i * RIFT_BINS + l];
        if (l == 0) out_index[at] = (int32_t)i;
    }
}

}  // namespace

// The stages over ANY packed cloud with sorted radius rows: refs[n] (w = the point's index), `order` a cell_refs-shaped
// array whose first gd->n_valid entries name the points to take (their w), `rows` the source of the CSR at a radius
// (keys: d2 bits << 32 | point index, ascending per row; valid until the next call of `rows`).  rgb: the colour words on
// the device (stride bytes apart); out_hist[n * 32], out_index[n] on the device.  Leaves the exclusive scan of the keep
// flags in RiftScratch::keep: keep[i] = kept descriptors in front of point i, keep[n] = their number.
int rift_stages(pcc_index* ix, const float4* refs, const float4* cell_refs, const GridDev* gd, size_t n, const RiftRows& rows,
                const unsigned char* rgb, size_t rgb_stride, double normal_radius, double gradient_radius, double rift_radius,
                float* out_hist, int32_t* out_index) {
    hipStream_t s = ix->stream;
    RiftScratch* r = scratch<RiftScratch>(ix);
    const unsigned int un = (unsigned int)n;
    const float origin[3] = {0.f, 0.f, 0.f};
    PCC_TRY(r->normals.reserve(n * sizeof(float4)));
    PCC_TRY(r->inten.reserve(n * sizeof(float)));
    PCC_TRY(r->grad.reserve(n * sizeof(float4)));
    PCC_TRY(r->hist.reserve(n * RIFT_BINS * sizeof(float)));
    PCC_TRY(r->keep.reserve((n + 1) * sizeof(unsigned int)));
    const unsigned int blocks = blocks_for(n);
    // rows at normal_radius: the plane fit, then (same radius: same rows) the intensity gradient
    const unsigned long long* keys = nullptr;
    const unsigned int* off32 = nullptr;
    PCC_TRY(rows(normal_radius, &keys, &off32));
    PCC_TRY(launch_normals_csr(s, refs, cell_refs, gd, n, keys, off32, origin, r->normals.as<float4>()));
    hipLaunchKernelGGL(k_rift_intensity, dim3(blocks), dim3(256), 0, s, rgb, rgb_stride, r->normals.as<float4>(), un, r->inten.as<float>());
    PCC_HIP(hipGetLastError());
    if (gradient_radius != normal_radius) PCC_TRY(rows(gradient_radius, &keys, &off32));
    PCC_HIP(hipMemsetAsync(r->grad.p, 0, n * sizeof(float4), s));
    hipLaunchKernelGGL(k_rift_gradient, dim3(blocks), dim3(256), 0, s, keys, off32, refs, r->inten.as<float>(), r->normals.as<float4>(),
                       cell_refs, gd, r->grad.as<float4>());
    PCC_HIP(hipGetLastError());
    // rows at rift_radius: the histograms
    PCC_TRY(rows(rift_radius, &keys, &off32));
    PCC_HIP(hipMemsetAsync(r->keep.p, 0, (n + 1) * sizeof(unsigned int), s));
    if (ix->opt.rift_layout == 1) {
        const unsigned int rb = (unsigned int)std::min<size_t>((n + 7) / 8, 8192);
        hipLaunchKernelGGL(k_rift_rows32, dim3(rb), dim3(256), 0, s, keys, off32, refs, r->grad.as<float4>(), cell_refs, gd, (float)rift_radius,
                           r->hist.as<float>(), r->keep.as<unsigned int>());
    } else {
        hipLaunchKernelGGL(k_rift_rows1, dim3(blocks), dim3(256), 0, s, keys, off32, refs, r->grad.as<float4>(), cell_refs, gd, (float)rift_radius,
                           r->hist.as<float>(), r->keep.as<unsigned int>());
    }
    PCC_HIP(hipGetLastError());
    // keep what is finite
    PCC_TRY(launch_exclusive_scan(ix, s, r->keep.as<unsigned int>(), n + 1, r->scan_tmp));
    const unsigned int cb = (unsigned int)std::min<size_t>((n + 7) / 8, 4096);
    hipLaunchKernelGGL(k_rift_compact, dim3(cb), dim3(256), 0, s, r->hist.as<float>(), r->keep.as<unsigned int>(), un, out_hist, out_index);
    PCC_HIP(hipGetLastError());
    return PCC_OK;
}

// the indexed cloud of ix: its grid's rows.  rgb: the colour words on the device (stride bytes apart); out_hist[n * 32],
// out_index[n] on the device; *n_out on the host
int rift_descriptors(pcc_index* ix, const unsigned char* rgb, size_t rgb_stride, double normal_radius, double gradient_radius,
                     double rift_radius, float* out_hist, int32_t* out_index, size_t* n_out) {
    const size_t n = ix->n_orig;
    const RiftRows rows = [ix](double radius, const unsigned long long** keys, const unsigned int** offsets) -> int {
        return radius_csr(ix, radius, keys, offsets);
    };
    PCC_TRY(rift_stages(ix, ix->refs.as<float4>(), ix->cell_refs.as<float4>(), ix->d_grid.as<GridDev>(), n, rows, rgb, rgb_stride, normal_radius,
                        gradient_radius, rift_radius, out_hist, out_index));
    unsigned int kept = 0;
    PCC_TRY(read_back(ix, scratch<RiftScratch>(ix)->keep.as<unsigned int>() + n, &kept));
    *n_out = kept;
    return PCC_OK;
}

int check_rift_params(double normal_radius, double gradient_radius, double rift_radius, int nr_distance_bins, int nr_gradient_bins) {
    for (double r : {normal_radius, gradient_radius, rift_radius})
        if (!(r > 0) || !std::isfinite(r)) { set_error("bad radius"); return PCC_ERR_INVALID; }
    if (nr_distance_bins != RIFT_D_BINS || nr_gradient_bins != RIFT_G_BINS) {
        set_error("RIFT with %d x %d bins: only %d distance x %d gradient bins are built", nr_distance_bins, nr_gradient_bins, RIFT_D_BINS, RIFT_G_BINS);
        return PCC_ERR_UNSUPPORTED;
    }
    return PCC_OK;
}

}  // namespace pcc

using namespace pcc;
extern "C" {
int pcc_rift_descriptors(pcc_index* ix, const void* rgb, size_t rgb_stride, int mem, double normal_radius, double gradient_radius,
                         double rift_radius, int nr_distance_bins, int nr_gradient_bins, float* out_hist, int32_t* out_index,
                         size_t* n_out) {
    // the arguments first: host arithmetic, refused before any device is looked at
    PCC_TRY(check_mem(mem));
    if (!rgb || !out_hist || !out_index || !n_out) { set_error("null argument"); return PCC_ERR_INVALID; }
    if (rgb_stride < 4 || rgb_stride % 4 || reinterpret_cast<uintptr_t>(rgb) % 4) {
        set_error("colour words must be 4-byte aligned, stride %zu a multiple of 4 and >= 4", rgb_stride);
        return PCC_ERR_INVALID;
    }
    PCC_TRY(check_rift_params(normal_radius, gradient_radius, rift_radius, nr_distance_bins, nr_gradient_bins));
    PCC_ENTER(ix);
    PCC_TRY(ensure_grid(ix));
    ev_next(ix);
    ev_mark(ix, EV_CALL0);
    const size_t n = ix->n_orig;
    RiftScratch* r = scratch<RiftScratch>(ix);
    const unsigned char* drgb = nullptr;
    PCC_TRY(stage_in(ix, reinterpret_cast<const unsigned char*>(rgb), (n - 1) * rgb_stride + 4, mem, r->rgb, &drgb));
    Out<float> rh;
    Out<int32_t> ri;
    PCC_TRY(rh.stage(out_hist, n * RIFT_BINS, mem, r->out_hist));
    PCC_TRY(ri.stage(out_index, n, mem, r->out_index));
    PCC_TRY(rift_descriptors(ix, drgb, rgb_stride, normal_radius, gradient_radius, rift_radius, rh.dev, ri.dev, n_out));
    rh.count = *n_out * RIFT_BINS;  // (only the rows that were written travel)
    ri.count = *n_out;
    ev_mark(ix, EV_CALL1);
    return finish(ix, mem, rh, ri);
}
}  // extern "C"
