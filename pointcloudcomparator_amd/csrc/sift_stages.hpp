// sift_stages.hpp -- the stages of the SIFT detector behind the voxel grid, the radius rows and the k-NN rows (sift.hip), over any
// cloud of 32-byte records whose rows and neighbours are indexed like the records: one octave cloud on the single path
// (pcc_sift_keypoints), the concatenation of a round on the batch path (sift_batch.hip).  Every launch goes to ix->stream, every
// buffer is the handle's SiftScratch.
#pragma once
#include "pcc_internal.hpp"
#include "sift_math.hpp"

namespace pcc {

// a record of an octave cloud: pcl::PointXYZRGB's layout, what the voxel grids read and write with colour
struct SiftRec {
    float x, y, z, w;
    uint32_t rgb;
    uint32_t pad[3];
};
static_assert(sizeof(SiftRec) == 32, "SiftRec layout");

// the four detector parameters as pcc_sift_keypoints and its batch form check them (sift.hip)
int check_sift_params(float min_scale, int nr_octaves, int nr_scales_per_octave, float min_contrast);
// SiftScratch::inten[i] = intensity of record i
int sift_intensity_stage(pcc_index* ix, const SiftRec* cloud, size_t n);
// SiftScratch::resp[i][s]: the Gaussian responses over the sorted radius rows (keys / offsets), either PCC_OPT_SIFT_LAYOUT
int sift_space_stage(pcc_index* ix, size_t n, const unsigned long long* keys, const unsigned int* offsets, const SiftOctave* oc, int n_scales);
// SiftScratch::mask / count from the extrema over nbr[i][K]; count scanned in place, count[n] = the keypoints of the cloud
int sift_extrema_stage(pcc_index* ix, size_t n, const int32_t* nbr, int K, const SiftOctave* oc);
// the `found` keypoints of the cloud into SiftScratch::kp behind the `have` it holds (the buffer grows as needed), in (point, scale) order
int sift_write_stage(pcc_index* ix, const SiftRec* cloud, size_t n, const SiftOctave* oc, size_t have, size_t found);

}  // namespace pcc
