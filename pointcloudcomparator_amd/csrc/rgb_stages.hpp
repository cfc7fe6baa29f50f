// rgb_stages.hpp -- the stages of colour region growing behind the k-NN rows (region_rgb.hip: prepare, link, flatten, the label
// sweeps, segment ids, per-segment records, the pair table, the host half, labels), for whoever brings the rows: the indexed
// cloud of a handle (pcc_region_growing_rgb) or the concatenation of a batch (region_rgb_batch.hip).  Every launch goes to
// ix->stream, the scratch is ix's; the kernels exist once, in region_rgb.hip, with the order of the points as a template
// parameter.
#pragma once
#include <functional>
#include <vector>

#include "pcc_internal.hpp"
#include "rgb_merge.hpp"

namespace pcc {

struct RgbRun {
    const float4* refs = nullptr;  // the n points in index order (device): w < 0 flags a non-finite point
    unsigned int n = 0;
    const unsigned long long* keys = nullptr;  // self k-NN rows, n x K, ascending (d2, index), unused entries ~0 (device)
    int K = 0;
    const unsigned char* rgb = nullptr;  // the colour word of point i at rgb + i * rgb_stride (device)
    size_t rgb_stride = 4;
    // The points the wave-per-point kernels take: the first gd->n_valid entries of cell_refs name them (an indexed cloud in cell
    // order) -- or, both null, every index 0 .. n itself (a concatenation: rows of non-finite points are empty)
    const float4* cell_refs = nullptr;
    const GridDev* gd = nullptr;
    float point_color_threshold = 0.f;
    unsigned int nr_neighbours = 0;
    // A concatenation of n_clouds clouds, cloud c = the points d_bases[c] .. d_bases[c + 1] (device, d_bases[n_clouds] = n): the
    // first segment id of every cloud -- ids are dense over the concatenation in index order -- is written to d_id_bases and
    // copied to h_id_bases (pinned) in the wait that brings the segment count, h_id_bases[n_clouds].  Null: one cloud.
    const unsigned int* d_bases = nullptr;
    unsigned int n_clouds = 0;
    unsigned int* d_id_bases = nullptr;
    unsigned int* h_id_bases = nullptr;
    int32_t* labels_dev = nullptr;   // labels[n] (device).  Null: counts only -- the host half's result is all the caller wants, so
                                     // no cluster id goes up, no label is written and the last wait falls away
    int32_t* labels_host = nullptr;  // nullable, pinned: the labels are copied there in front of the last wait
};

// The host half: segs[ns] and pairs[np] (any order; may be sorted in place) as rgb_merge.hpp takes them -> the cluster of every
// segment, cluster_of_segment[ns].  Returns a pcc_status.
typedef std::function<int(const RgbSegment* segs, unsigned int ns, RgbSegmentPair* pairs, unsigned int np,
                          std::vector<int32_t>& cluster_of_segment)>
    RgbHostHalf;

// the thresholds and neighbour counts as pcc_region_growing_rgb and its batch form check them (region_rgb.hip)
int check_rgb_params(float distance_threshold, float point_color_threshold, float region_color_threshold, unsigned int nr_neighbours,
                     unsigned int nr_region_neighbours);

// Waits: one per label sweep, one for the segment count (and the clouds' first ids), one for the pair count, one for the pair
// list (a second one beyond 2^18 pairs), one at the end.  Leaves segments, pairs and sweeps in ix->stats[0], [1], [7].
int rgb_stages(pcc_index* ix, const RgbRun& run, const RgbHostHalf& host_half);

// region_rgb_batch.hip: the rows of a concatenation, keys[total][K], for whoever brings its points (w = bits(concatenated index),
// negative for a non-finite point) and rift_batch_plan.hpp's items on the device: k_rgb_batch_knn, one launch.  K <= RGB_BATCH_MAX_K.
constexpr unsigned int RGB_BATCH_MAX_K = 128;  // the longest row the batch kernel builds (two registers of top list per lane)
int rgb_batch_rows(pcc_index* ix, const RiftBatchItem* d_items, unsigned int n_items, const float4* d_pts, int K, unsigned long long* keys);

}  // namespace pcc
