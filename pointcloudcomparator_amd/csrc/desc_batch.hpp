// desc_batch.hpp -- what the descriptor batch calls share across their translation units: the halves of
// pcc_sift_keypoints_batch (sift_batch.hip) and pcc_rift_descriptors_batch (rift_batch.hip) that run over a DEVICE-RESIDENT
// concatenation (their scratch stays in their own files).  The two entry points stage their host clouds and call them;
// pcc_cluster_descriptors (cluster_desc.hip) stages the clusters once, in either memory space, and calls the same halves.
#pragma once
#include <algorithm>
#include <vector>

#include "entry.hpp"
#include "sift_stages.hpp"
#include "sift_batch_plan.hpp"

namespace pcc {

// ---- sift_batch.hip ---------------------------------------------------------------------------------------------------------
// every octave's scales, scale = min_scale * 2^o (doubled per octave, as PCL does); at most 300 octaves (a float doubles fewer
// than 300 times before it is +inf: the 25-point gate has ended every cloud long before)
inline std::vector<SiftOctave> sift_batch_octaves(float min_scale, int nr_octaves, int nr_scales_per_octave, float min_contrast) {
    std::vector<SiftOctave> oc((size_t)std::min(nr_octaves, 300));
    float sc = min_scale;
    for (SiftOctave& o : oc) { sift_octave_scales(sc, nr_scales_per_octave, min_contrast, &o); sc *= 2.0f; }
    return oc;
}

// The first concatenation of a call as the rounds find it on the device: the table in front of the first round (round0, built
// by sift_batch_round with min_points = 0; its items are not used), the octaves, and cloud c's records at d_rec0[bases0[c] ..].
struct SiftBatchInput {
    const SiftBatchRound* round0 = nullptr;
    const std::vector<SiftOctave>* h_octaves = nullptr;
    const SiftOctave* d_octaves = nullptr;
    const unsigned int* d_bases0 = nullptr;
    const int64_t* d_bases64_0 = nullptr;
    const SiftRec* d_rec0 = nullptr;
};
// What the rounds leave behind: the keypoints of every round on the device (SiftScratch::kp, round-major) and, on the host, how
// many each round found in each cloud.
struct SiftBatchResult {
    std::vector<std::vector<uint32_t>> counts;  // [round][cloud]
    std::vector<uint32_t> bases0;               // the first concatenation's bases (the snap's clouds)
    const unsigned int* d_bases0 = nullptr;
    const SiftRec* d_rec0 = nullptr;
    size_t total = 0;                           // keypoints on the device
    unsigned int rounds = 0;
};
// the octave rounds over a staged concatenation
int sift_batch_rounds(pcc_index* ix, size_t n_clouds, const SiftBatchInput& in, float min_scale, SiftBatchResult* res);
// d_snap[k] for the res.total keypoints of the rounds, in their round-major order: k_sb_snap over the first concatenation
int sift_batch_snap(pcc_index* ix, const SiftBatchResult& res, size_t n_clouds, double snap_radius, int32_t* d_snap);

// ---- rift_batch.hip ---------------------------------------------------------------------------------------------------------
// A concatenation of clouds on the device with its table: bases[n_clouds + 1], the builder's work items, the points with
// w = bits(concatenated index), one colour word a point, and a GridDev of which n_valid = total is all that is read.
struct RiftBatchInput {
    size_t n_clouds = 0, total = 0;
    const GridDev* gd = nullptr;
    const unsigned int* d_bases = nullptr;
    const RiftBatchItem* d_items = nullptr;
    unsigned int n_items = 0;
    const float4* d_pts = nullptr;
    const unsigned char* d_rgb = nullptr;
};
// The stages of the single call once over the concatenation, then k_batch_finish: the kept rows in RiftScratch::out_hist /
// out_index (device, indices local to their cloud), the slice bounds (n_clouds + 1) in *d_slice (device).  total > 0.
int rift_batch_run(pcc_index* ix, const RiftBatchInput& in, double normal_radius, double gradient_radius, double rift_radius,
                   const unsigned int** d_slice);
// the slice bounds of the run on the host (one wait); valid until the batch scratch's `down` is used again
int rift_batch_slices(pcc_index* ix, size_t n_clouds, const unsigned int** h_slice);
// the first `kept` rows of the run into host arrays (one wait)
int rift_batch_fetch(pcc_index* ix, size_t kept, float* out_hist, int32_t* out_index);

}  // namespace pcc
