// sift.hip -- the SIFT keypoint detector of ONE coloured cloud (gfx950): pcc_sift_keypoints.
// replaces: processSift (reference src/comparator.cpp:435-469): pcl::SIFTKeypoint<PointXYZRGB, PointWithScale> with
//   setScales(0.005f, 5, 5) and setMinimumContrast(0.001f).
//
// Per octave: the current cloud through the voxel grid (voxel.hip, leaf = the octave's scale) -> fewer than 25 points end
// the loop -> the octave cloud indexed on the work handle kept inside ctx -> intensity -> sorted radius rows at three times
// the largest scale (CSR of u64 keys, d2 bits << 32 | point index, ascending) -> the scale space (k_sift_space_*: a
// Gaussian-weighted mean intensity per point and scale over the row's prefix with d2 <= 9 sigma2, sums in ROW ORDER) -> the
// 25 nearest neighbours of every point (knn.hip) -> the extrema of the difference-of-Gaussian columns (k_sift_extrema: a
// mask and a count per point) -> exclusive scan -> the keypoints written in (point, scale) order behind those of the
// octaves before.  The arithmetic is sift_math.hpp's, shared with the host mirror of the tests: same bits.
#include <algorithm>
#include <cmath>
#include <vector>

#include "entry.hpp"
#include "lane_ops.hpp"
#include "sift_stages.hpp"

namespace pcc {

namespace {

// the caller's points and colour words (two arrays, two strides) as records
__global__ void __launch_bounds__(256)
k_sift_assemble(const unsigned char* __restrict__ pts, size_t stride, const unsigned char* __restrict__ rgb, size_t rgb_stride,
                unsigned int n, SiftRec* __restrict__ out) {
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float* p = reinterpret_cast<const float*>(pts + (size_t)i * stride);
        SiftRec r;
        r.x = p[0]; r.y = p[1]; r.z = p[2]; r.w = 1.0f;
        r.rgb = *reinterpret_cast<const uint32_t*>(rgb + (size_t)i * rgb_stride);
        r.pad[0] = r.pad[1] = r.pad[2] = 0u;
        out[i] = r;
    }
}

__global__ void __launch_bounds__(256)
k_sift_intensity(const SiftRec* __restrict__ cloud, unsigned int n, float* __restrict__ inten) {
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) inten[i] = sift_intensity(cloud[i].rgb);
}

// Scale space, PCC_OPT_SIFT_LAYOUT = 0: one lane per (point, scale) walks its own prefix of the point's row -- PCL's loop
// as it stands.  resp[i * n_scales + s].
__global__ void __launch_bounds__(256)
k_sift_space_lane(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ offsets, const float* __restrict__ inten,
                  const SiftOctave* __restrict__ oc, unsigned int n, float* __restrict__ resp) {
    const unsigned int S = (unsigned int)oc->n_scales;
    const unsigned int total = n * S;
    for (unsigned int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
        const unsigned int i = t / S, s = t - i * S;
        const float sigma2 = oc->sigma2[s], cut = oc->cut[s];
        const unsigned int beg = offsets[i], end = offsets[i + 1];
        float num = 0.f, den = 0.f;
        for (unsigned int k = beg; k < end; ++k) {
            const unsigned long long key = keys[k];
            const float d2 = __uint_as_float((unsigned int)(key >> 32));
            if (!(d2 <= cut)) break;
            sift_accumulate(inten[(unsigned int)key], sift_weight(d2, sigma2), &num, &den);
        }
        resp[t] = sift_response(num, den);
    }
}

// Scale space, PCC_OPT_SIFT_LAYOUT = 1: a wave per point.  Per chunk of 64 row entries every lane takes ONE entry and
// computes its weight and value * weight for every scale whose prefix holds it (the expf is the expensive part) into LDS;
// then lane s, the owner of scale s, adds the chunk's shares of its scale in row order and stops at the first entry beyond
// its prefix -- the order of additions per (point, scale) is the row's, and no two lanes ever add to the same word.
__global__ void __launch_bounds__(256)
k_sift_space_wave(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ offsets, const float* __restrict__ inten,
                  const SiftOctave* __restrict__ oc, unsigned int n, float* __restrict__ resp) {
    __shared__ float d2_all[4][64];
    __shared__ float2 share_all[4][SIFT_MAX_SCALES][65];  // (65: the owners read one column, lane s at row s -- a stride of 64 float2 is one bank)
    const unsigned int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float* d2s = d2_all[wv];
    float2 (*share)[65] = share_all[wv];
    const unsigned int S = (unsigned int)oc->n_scales;
    const bool owner = lane < S;
    const float my_cut = owner ? oc->cut[lane] : 0.f;
    const unsigned int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (unsigned int i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n; i += nwaves) {
        const unsigned int beg = offsets[i], len = offsets[i + 1] - beg;
        float num = 0.f, den = 0.f;
        bool open = owner;
        for (unsigned int c0 = 0; c0 < len; c0 += 64) {
            const unsigned int e = c0 + lane;
            float d2 = __builtin_inff(), v = 0.f;
            if (e < len) {
                const unsigned long long key = keys[beg + e];
                d2 = __uint_as_float((unsigned int)(key >> 32));
                v = inten[(unsigned int)key];
            }
            wave_lds_sync();  // (the owners have finished with the chunk before)
            d2s[lane] = d2;
            for (unsigned int s = 0; s < S; ++s) {
                if (d2 <= oc->cut[s]) {
                    const float w = sift_weight(d2, oc->sigma2[s]);
                    share[s][lane] = make_float2(v * w, w);
                }
            }
            wave_lds_sync();
            if (open) {
                const unsigned int m = min(64u, len - c0);
                for (unsigned int k = 0; k < m; ++k) {
                    if (!(d2s[k] <= my_cut)) { open = false; break; }
                    const float2 q = share[lane][k];
                    num += q.x;
                    den += q.y;
                }
            }
            if (__ballot(open) == 0ull) break;  // every prefix has ended
        }
        if (owner) resp[(size_t)i * S + lane] = sift_response(num, den);
    }
}

// Extrema: one lane per point.  min / max of every DoG column over the point's neighbours, the decisions for the inner
// columns, mask[i] bit s = (point i, column s) is a keypoint; count[i] = their number (scanned afterwards).
__global__ void __launch_bounds__(256)
k_sift_extrema(const float* __restrict__ resp, const int32_t* __restrict__ nbr, int K, const SiftOctave* __restrict__ oc, unsigned int n,
               unsigned int* __restrict__ mask, unsigned int* __restrict__ count) {
    const int S = oc->n_scales, D = S - 1;
    const float min_contrast = oc->min_contrast;
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float mn[SIFT_MAX_DOG], mx[SIFT_MAX_DOG], own[SIFT_MAX_DOG];
#pragma unroll
        for (int c = 0; c < SIFT_MAX_DOG; ++c) { mn[c] = 3.402823466e38f; mx[c] = -3.402823466e38f; own[c] = 0.f; }
        for (int k = 0; k < K; ++k) {
            const int32_t j = nbr[(size_t)i * K + k];
            if (j < 0) continue;
            const float* rj = resp + (size_t)j * S;
            float lo = rj[0];
#pragma unroll
            for (int c = 0; c < SIFT_MAX_DOG; ++c) {
                if (c < D) {
                    const float hi = rj[c + 1];
                    const float d = sift_dog(hi, lo);
                    mn[c] = fminf(mn[c], d);
                    mx[c] = fmaxf(mx[c], d);
                    lo = hi;
                }
            }
        }
        const float* ri = resp + (size_t)i * S;
        float lo = ri[0];
#pragma unroll
        for (int c = 0; c < SIFT_MAX_DOG; ++c) {
            if (c < D) {
                const float hi = ri[c + 1];
                own[c] = sift_dog(hi, lo);
                lo = hi;
            }
        }
        unsigned int m = 0;
#pragma unroll
        for (int c = 1; c < SIFT_MAX_DOG - 1; ++c) {
            if (c < D - 1 && sift_is_keypoint(own[c], mn[c - 1], mn[c], mn[c + 1], mx[c - 1], mx[c], mx[c + 1], min_contrast)) m |= 1u << c;
        }
        mask[i] = m;
        count[i] = (unsigned int)__popc(m);
    }
}

// pos = exclusive scan of count; the keypoints of point i behind those of the points before it, columns ascending
__global__ void __launch_bounds__(256)
k_sift_write(const SiftRec* __restrict__ cloud, const unsigned int* __restrict__ mask, const unsigned int* __restrict__ pos,
             const SiftOctave* __restrict__ oc, unsigned int n, float4* __restrict__ out) {
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        unsigned int m = mask[i], at = pos[i];
        if (!m) continue;
        const SiftRec p = cloud[i];
        while (m) {
            const int c = __ffs((int)m) - 1;
            m &= m - 1;
            out[at++] = make_float4(p.x, p.y, p.z, oc->scales[c]);
        }
    }
}

}  // namespace

// ---- the stages behind the voxel grid, the rows and the neighbours (sift_stages.hpp: shared with sift_batch.hip) --------------
int sift_intensity_stage(pcc_index* ix, const SiftRec* cloud, size_t n) {
    SiftScratch* r = scratch<SiftScratch>(ix);
    PCC_TRY(r->inten.reserve(n * sizeof(float)));
    const unsigned int blocks = blocks_for(n);
    hipLaunchKernelGGL(k_sift_intensity, dim3(blocks), dim3(256), 0, ix->stream, cloud, (unsigned int)n, r->inten.as<float>());
    PCC_HIP(hipGetLastError());
    return PCC_OK;
}

int sift_space_stage(pcc_index* ix, size_t n, const unsigned long long* keys, const unsigned int* offsets, const SiftOctave* oc, int n_scales) {
    SiftScratch* r = scratch<SiftScratch>(ix);
    const size_t S = (size_t)n_scales;
    PCC_TRY(r->resp.reserve(n * S * sizeof(float)));
    if (ix->opt.sift_layout == 1) {
        const unsigned int wb = (unsigned int)std::min<size_t>((n + 3) / 4, 8192);
        hipLaunchKernelGGL(k_sift_space_wave, dim3(wb), dim3(256), 0, ix->stream, keys, offsets, r->inten.as<float>(), oc, (unsigned int)n,
                           r->resp.as<float>());
    } else {
        const unsigned int lb = (unsigned int)std::min<size_t>((n * S + 255) / 256, 8192);
        hipLaunchKernelGGL(k_sift_space_lane, dim3(lb), dim3(256), 0, ix->stream, keys, offsets, r->inten.as<float>(), oc, (unsigned int)n,
                           r->resp.as<float>());
    }
    PCC_HIP(hipGetLastError());
    return PCC_OK;
}

int sift_extrema_stage(pcc_index* ix, size_t n, const int32_t* nbr, int K, const SiftOctave* oc) {
    hipStream_t s = ix->stream;
    SiftScratch* r = scratch<SiftScratch>(ix);
    PCC_TRY(r->mask.reserve(n * sizeof(unsigned int)));
    PCC_TRY(r->count.reserve((n + 1) * sizeof(unsigned int)));
    PCC_HIP(hipMemsetAsync(r->count.p, 0, (n + 1) * sizeof(unsigned int), s));
    const unsigned int blocks = blocks_for(n);
    hipLaunchKernelGGL(k_sift_extrema, dim3(blocks), dim3(256), 0, s, r->resp.as<float>(), nbr, K, oc, (unsigned int)n, r->mask.as<unsigned int>(),
                       r->count.as<unsigned int>());
    PCC_HIP(hipGetLastError());
    return launch_exclusive_scan(ix, s, r->count.as<unsigned int>(), n + 1, r->scan_tmp);
}

int sift_write_stage(pcc_index* ix, const SiftRec* cloud, size_t n, const SiftOctave* oc, size_t have, size_t found) {
    SiftScratch* r = scratch<SiftScratch>(ix);
    if (!found) return PCC_OK;
    PCC_TRY(r->kp.grow_keep(ix->stream, have * sizeof(float4), (have + found) * sizeof(float4)));
    const unsigned int blocks = blocks_for(n);
    hipLaunchKernelGGL(k_sift_write, dim3(blocks), dim3(256), 0, ix->stream, cloud, r->mask.as<unsigned int>(), r->count.as<unsigned int>(), oc,
                       (unsigned int)n, r->kp.as<float4>() + have);
    PCC_HIP(hipGetLastError());
    return PCC_OK;
}

// pts / rgb on the device; the keypoints are left in SiftScratch::kp (device), *n_out of them
int sift_keypoints(pcc_index* ix, const unsigned char* pts, size_t n, size_t stride, const unsigned char* rgb, size_t rgb_stride,
                   float min_scale, int nr_octaves, int nr_scales_per_octave, float min_contrast, size_t* n_out) {
    hipStream_t s = ix->stream;
    SiftScratch* r = scratch<SiftScratch>(ix);
    *n_out = 0;
    // the work handle's launches join the caller's queue for the length of this call (under options of its own)
    WorkLease lease;
    PCC_TRY(lease.take(ix, r->work, false));
    pcc_index* w = lease.w;
    PCC_TRY(r->cloud[0].reserve(n * sizeof(SiftRec)));
    PCC_TRY(r->cloud[1].reserve(n * sizeof(SiftRec)));
    // (a float doubles fewer than 300 times before it is +inf: the 25-point gate has ended the loop long before)
    nr_octaves = std::min(nr_octaves, 300);
    PCC_TRY(r->octaves.reserve((size_t)nr_octaves * sizeof(SiftOctave)));
    const unsigned int blocks0 = blocks_for(n);
    hipLaunchKernelGGL(k_sift_assemble, dim3(blocks0), dim3(256), 0, s, pts, stride, rgb, rgb_stride, (unsigned int)n, r->cloud[0].as<SiftRec>());
    PCC_HIP(hipGetLastError());
    // every octave's scales: scale = min_scale * 2^o (doubled per octave, as PCL does).  (The first octave's voxel grid waits
    // for the stream before h_octaves goes away.)
    std::vector<SiftOctave> h_octaves((size_t)nr_octaves);
    {
        float sc = min_scale;
        for (int o = 0; o < nr_octaves; ++o, sc *= 2.0f) sift_octave_scales(sc, nr_scales_per_octave, min_contrast, &h_octaves[(size_t)o]);
    }
    PCC_HIP(hipMemcpyAsync(r->octaves.p, h_octaves.data(), h_octaves.size() * sizeof(SiftOctave), hipMemcpyHostToDevice, s));
    int cur = 0;
    size_t n_cur = n, total = 0;
    float scale = min_scale;
    for (int o = 0; o < nr_octaves; ++o, scale *= 2.0f) {
        // 1. down-sample (two waits of its own: the lattice is sized on the host, the voxel count comes back)
        size_t n_oct = 0;
        PCC_TRY(voxel_grid(ix, r->cloud[cur].p, n_cur, sizeof(SiftRec), PCC_MEM_DEVICE, scale, 1, r->cloud[cur ^ 1].p, sizeof(SiftRec), &n_oct));
        cur ^= 1;
        n_cur = n_oct;
        // 2. PCL's min_nr_points
        if (n_oct < (size_t)SIFT_MIN_POINTS) break;
        const SiftRec* cloud = r->cloud[cur].as<SiftRec>();
        // 3. the octave's scales (uploaded in front of the loop)
        const SiftOctave& h_oc = h_octaves[(size_t)o];
        const int S = h_oc.n_scales;
        const SiftOctave* oc = r->octaves.as<SiftOctave>() + o;
        // the octave cloud indexed on the work handle
        PCC_TRY(set_input(w, cloud, n_oct, sizeof(SiftRec), PCC_MEM_DEVICE));
        entered(w);
        // 4. intensity
        PCC_TRY(sift_intensity_stage(ix, cloud, n_oct));
        // 5. scale space over the sorted rows at 3 x the largest scale
        const float radius = 3.0f * h_oc.scales[S - 1];
        const unsigned long long* keys = nullptr;
        const unsigned int* off32 = nullptr;
        PCC_TRY(radius_csr(w, (double)radius, &keys, &off32));
        PCC_TRY(sift_space_stage(ix, n_oct, keys, off32, oc, S));
        // 6. extrema over the 25 nearest neighbours (the gate above: the cloud holds at least that many)
        const int K = (int)std::min<size_t>(SIFT_NEIGHBOURS, n_oct);
        PCC_TRY(r->nbr.reserve(n_oct * (size_t)K * sizeof(int32_t)));
        PCC_TRY(r->nbr_d2.reserve(n_oct * (size_t)K * sizeof(float)));
        PCC_TRY(grid_knn(w, w->refs.as<float4>(), n_oct, K, nullptr, r->nbr.as<int32_t>(), r->nbr_d2.as<float>()));
        PCC_TRY(sift_extrema_stage(ix, n_oct, r->nbr.as<int32_t>(), K, oc));
        unsigned int found = 0;
        PCC_TRY(read_back(ix, r->count.as<unsigned int>() + n_oct, &found));  // the octave's wait
        // 7. behind the keypoints of the octaves before
        PCC_TRY(sift_write_stage(ix, cloud, n_oct, oc, total, found));
        total += found;
    }
    *n_out = total;
    return PCC_OK;
}

int check_sift_params(float min_scale, int nr_octaves, int nr_scales_per_octave, float min_contrast) {
    if (!(min_scale > 0.f) || !std::isfinite(min_scale)) { set_error("min_scale must be positive and finite"); return PCC_ERR_INVALID; }
    if (!(min_contrast >= 0.f)) { set_error("min_contrast must not be negative"); return PCC_ERR_INVALID; }
    if (nr_octaves < 1) { set_error("nr_octaves %d: at least one octave", nr_octaves); return PCC_ERR_INVALID; }
    if (nr_scales_per_octave < SIFT_MIN_SCALES_PER_OCTAVE || nr_scales_per_octave > SIFT_MAX_SCALES_PER_OCTAVE) {
        set_error("SIFT with %d scales per octave: %d to %d scales per octave are built", nr_scales_per_octave, SIFT_MIN_SCALES_PER_OCTAVE,
                  SIFT_MAX_SCALES_PER_OCTAVE);
        return PCC_ERR_UNSUPPORTED;
    }
    return PCC_OK;
}

}  // namespace pcc

using namespace pcc;
extern "C" {
int pcc_sift_keypoints(pcc_index* ix, const void* pts, size_t n, size_t stride, const void* rgb, size_t rgb_stride, int mem, float min_scale,
                       int nr_octaves, int nr_scales_per_octave, float min_contrast, float* out_keypoints, size_t capacity, size_t* n_out) {
    // the arguments first: host arithmetic, refused before any device is looked at
    PCC_TRY(check_points(pts, n, stride, mem));
    if (!n_out || (n && !rgb) || (capacity && !out_keypoints)) { set_error("null argument"); return PCC_ERR_INVALID; }
    if (rgb_stride < 4 || rgb_stride % 4 || (n && (reinterpret_cast<uintptr_t>(rgb) % 4 || reinterpret_cast<uintptr_t>(pts) % 4)) ||
        (capacity && reinterpret_cast<uintptr_t>(out_keypoints) % 4)) {
        set_error("points, colour words and keypoints must be 4-byte aligned, the colour stride %zu a multiple of 4 and >= 4", rgb_stride);
        return PCC_ERR_INVALID;
    }
    PCC_TRY(check_sift_params(min_scale, nr_octaves, nr_scales_per_octave, min_contrast));
    PCC_ENTER(ix);
    *n_out = 0;
    if (n == 0) { PCC_NOTHING_ENQUEUED(ix); return PCC_OK; }
    ev_next(ix);
    ev_mark(ix, EV_CALL0);
    SiftScratch* r = scratch<SiftScratch>(ix);
    const unsigned char *dpts = nullptr, *drgb = nullptr;
    PCC_TRY(stage_in(ix, reinterpret_cast<const unsigned char*>(pts), (n - 1) * stride + 12, mem, r->pts, &dpts));
    PCC_TRY(stage_in(ix, reinterpret_cast<const unsigned char*>(rgb), (n - 1) * rgb_stride + 4, mem, r->rgb, &drgb));
    size_t found = 0;
    PCC_TRY(sift_keypoints(ix, dpts, n, stride, drgb, rgb_stride, min_scale, nr_octaves, nr_scales_per_octave, min_contrast, &found));
    ev_mark(ix, EV_CALL1);
    *n_out = found;
    if (found > capacity) {
        set_error("%zu keypoints, room for %zu", found, capacity);
        return PCC_ERR_OVERFLOW;
    }
    if (found == 0) return PCC_OK;
    // (no Out / finish: the keypoints collect in the scratch's own buffer and leave it by one plain copy in either memory space)
    PCC_TRY(copy_out(ix, out_keypoints, r->kp.p, found * 4 * sizeof(float), mem));
    if (mem == PCC_MEM_HOST) PCC_HIP(hipStreamSynchronize(ix->stream));
    return PCC_OK;
}
}  // extern "C"
