// sift_math.hpp -- the arithmetic of the SIFT keypoint detector (pcl::SIFTKeypoint<PointXYZRGB, PointWithScale>, reference
// src/comparator.cpp:435-469), shared by the kernels (sift.hip) and by the host mirror of the tests
// (tests/cpp/sift_host.cpp): same operations, same order, same bits.  float32 throughout, every operation rounded on its
// own (-ffp-contract=off on both sides), expf from libm_f32.hpp.
//   scale space: response(point, scale) = sum(value * w) / sum(w) over the row entries with d2 <= 9 sigma2, in row order,
//                w = expf(-0.5f * d2 / sigma2); dog(point, i - 1) = response_i - response_{i-1}
//   extrema:     min / max of every DoG column over the point's nearest neighbours; column s is a keypoint when
//                |v| >= min_contrast and v is the column's minimum and below the minima of both neighbouring columns, or
//                the mirrored maximum test
#pragma once
#include "libm_f32.hpp"

namespace pcc {

constexpr int SIFT_MIN_SCALES_PER_OCTAVE = 1;
constexpr int SIFT_MAX_SCALES_PER_OCTAVE = 13;
constexpr int SIFT_MAX_SCALES = SIFT_MAX_SCALES_PER_OCTAVE + 3;  // scales of one octave
constexpr int SIFT_MAX_DOG = SIFT_MAX_SCALES - 1;                // DoG columns
constexpr int SIFT_NEIGHBOURS = 25;                              // rows of the extremum test (self included)
constexpr int SIFT_MIN_POINTS = 25;                              // an octave cloud below it ends the loop

// what an octave's kernels are told (device memory, one per octave)
struct SiftOctave {
    float scales[SIFT_MAX_SCALES];
    float sigma2[SIFT_MAX_SCALES];  // powf(scale, 2.0f), taken on the host
    float cut[SIFT_MAX_SCALES];     // 9 * sigma2: the row prefix a scale takes
    int n_scales;
    float min_contrast;
};

// intensity of PCL's packed colour word (bytes b, g, r from the low byte)
__host__ __device__ inline float sift_intensity(uint32_t c) {
    const int r = (int)((c >> 16) & 0xffu), g = (int)((c >> 8) & 0xffu), b = (int)(c & 0xffu);
    return (float)(299 * r + 587 * g + 114 * b) / 1000.0f;
}
__host__ __device__ inline float sift_cut(float sigma2) { return 9.0f * sigma2; }
__host__ __device__ inline float sift_weight(float d2, float sigma2) { return lm_expf(-0.5f * d2 / sigma2); }
// one row entry into the running sums of one scale
__host__ __device__ inline void sift_accumulate(float value, float w, float* num, float* den) {
    *num += value * w;
    *den += w;
}
__host__ __device__ inline float sift_response(float num, float den) { return num / den; }
__host__ __device__ inline float sift_dog(float response_hi, float response_lo) { return response_hi - response_lo; }
// v = dog(point, s); the minima / maxima of columns s - 1, s, s + 1 over the point's neighbours
__host__ __device__ inline bool sift_is_keypoint(float v, float min_lo, float min_s, float min_hi, float max_lo, float max_s, float max_hi,
                                                 float min_contrast) {
    if (!(fabsf(v) >= min_contrast)) return false;
    if (v == min_s && v < min_lo && v < min_hi) return true;
    return v == max_s && v > max_lo && v > max_hi;
}

// (host only) the scales of one octave (PCL's detectKeypointsForOctave): scales[i] = base * powf(2, (i - 1) / n),
// sigma2 = powf(scale, 2).  powf is the host libm's; its arguments are kept from the compiler so that no build folds a call
// into something that rounds differently (the library and the host mirror come from different compilers).
inline void sift_octave_scales(float base_scale, int nr_scales_per_octave, float min_contrast, SiftOctave* oc) {
    memset(oc, 0, sizeof(*oc));
    volatile float two = 2.0f;
    oc->n_scales = nr_scales_per_octave + 3;
    oc->min_contrast = min_contrast;
    for (int i = 0; i < oc->n_scales; ++i) {
        volatile float e = ((float)i - 1.0f) / (float)nr_scales_per_octave;
        const float s = base_scale * powf(two, e);
        volatile float sv = s;
        oc->scales[i] = s;
        oc->sigma2[i] = powf(sv, two);
        oc->cut[i] = sift_cut(oc->sigma2[i]);
    }
}

}  // namespace pcc
