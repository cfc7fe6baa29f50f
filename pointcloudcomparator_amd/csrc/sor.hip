// sor.hip -- pcl::StatisticalOutlierRemoval (reference src/comparator.cpp:1523-1541): pcc_sor, pcc_sor_partial / pcc_sor_threshold, and
// the stages pcc_sor_sharded (comm.hip) shares with them.  Host code only: the kernels are pack.hip's (launch_sor_*), the search knn.hip's.
#include "entry.hpp"
#include <cmath>

namespace pcc {

int sor_begin(pcc_index* ix, size_t start, size_t count, int mean_k) {
    if (mean_k < 1 || mean_k + 1 > PCC_KNN_MAX_K) { set_error("mean_k=%d outside [1, %d]", mean_k, PCC_KNN_MAX_K - 1); return PCC_ERR_UNSUPPORTED; }
    if (start > ix->n_orig || count > ix->n_orig - start) { set_error("shard [%zu, %zu) outside the cloud (%zu points)", start, start + count, ix->n_orig); return PCC_ERR_INVALID; }
    return ensure_grid(ix);
}

int sor_means(pcc_index* ix, size_t start, size_t count, int K, float** dmean_out) {
    // self query: the packed references ARE the queries (non-finite points are flagged, are
    // skipped by the search and keep distance 0, as in PCL's applyFilterIndices)
    // the mean needs the distances only: the search delivers rows of d2 (4 bytes an entry) where its wave kernels serve K
    // and the staged mean kernel's tile fits LDS (K <= 126), rows of keys otherwise
    const bool d2_only = grid_knn_delivers(K) && (size_t)2 * 64 * (K + 1) * sizeof(unsigned int) <= 64 * 1024;
    PCC_TRY(ix->out_packed.reserve(count * (size_t)K * (d2_only ? sizeof(float) : sizeof(unsigned long long))));
    auto* keys = d2_only ? nullptr : ix->out_packed.as<unsigned long long>();
    float* d2_rows = d2_only ? ix->out_packed.as<float>() : nullptr;
    const float4* q = ix->refs.as<float4>() + start;  // (the whole cloud: q == refs, which the query sort recognises as a self query)
    if (count) PCC_TRY(grid_knn(ix, q, count, K, keys, nullptr, d2_rows));
    PCC_TRY(ix->out_d2.reserve(count * sizeof(float)));
    float* dmean = ix->out_d2.as<float>();
    if (count) {
        PCC_HIP(hipMemsetAsync(dmean, 0, count * sizeof(float), ix->stream));
        PCC_TRY(launch_sor_mean(ix->stream, keys, q, count, K, dmean, d2_rows));
    }
    *dmean_out = dmean;
    return PCC_OK;
}

void sor_in_order(const float* hm, size_t no, size_t n_valid, int K, double stddev_mult, size_t start, size_t count, double* thr_out,
                  size_t* kept_out, uint8_t* mask) {
    const size_t valid = n_valid >= (size_t)K ? n_valid : 0;
    double sum = 0, sq = 0;
    for (size_t i = 0; i < no; ++i) { const float f = hm[i]; sum += f; sq += (double)(f * f); }  // PCL squares in float, then widens
    const double mean = sum / (double)valid;
    const double var = (sq - sum * sum / (double)valid) / ((double)valid - 1);
    const double thr = mean + stddev_mult * std::sqrt(var);
    size_t kept = 0;
    for (size_t i = 0; i < no; ++i) {
        const uint8_t in = !(hm[i] > thr);
        kept += in;
        if (i - start < count) mask[i - start] = in;  // (i < start wraps around to a huge value)
    }
    *thr_out = thr;
    *kept_out = kept;
}

}  // namespace pcc

using namespace pcc;
extern "C" {
int pcc_sor(pcc_index* ix, int mean_k, double stddev_mult, int mem, float* mean_dist, uint8_t* inlier,
            double* threshold, size_t* kept) {
    PCC_ENTER(ix);
    PCC_TRY(check_mem(mem));
    PCC_TRY(sor_begin(ix, 0, ix->n_orig, mean_k));
    ev_next(ix);
    ev_mark(ix, EV_CALL0);
    const size_t no = ix->n_orig;
    const int K = mean_k + 1;
    float* dmean = nullptr;
    PCC_TRY(sor_means(ix, 0, no, K, &dmean));
    // statistics, threshold and mask on the device (pack.hip: exact whenever no addition of PCL's in-order sums rounds);
    // the host sees one SorStats.  Round 3 copied the means back, added them up on one host thread and sent a mask: 0.94 ms
    // beside a 1.2 ms search at 1M points
    SorStats hs{};
    PCC_TRY(ix->scratch_a.reserve(SOR_STATS_SCRATCH_BYTES));
    PCC_TRY(ix->scratch_b.reserve(no + 64));
    SorStats* st_dev = &ix->words()->sor;
    uint8_t* dmask = mem == PCC_MEM_DEVICE && inlier ? inlier : ix->scratch_b.as<uint8_t>();
    PCC_TRY(launch_sor_stats(ix->stream, dmean, no, ix->d_grid.as<GridDev>(), K, stddev_mult, ix->scratch_a.as<double>(), st_dev, dmask));
    ev_mark(ix, EV_CALL1);
    PCC_HIP(hipMemcpyAsync(&hs, st_dev, sizeof(hs), hipMemcpyDeviceToHost, ix->stream));
    // (no Out / finish: host results come back through the pinned host_a / host_b, which the in-order sums walk too -- never the host pipe)
    if (mem == PCC_MEM_HOST) {
        PCC_TRY(ix->host_a.reserve(no * sizeof(float)));
        PCC_TRY(ix->host_b.reserve(no));
        if (mean_dist) PCC_HIP(hipMemcpyAsync(ix->host_a.p, dmean, no * sizeof(float), hipMemcpyDeviceToHost, ix->stream));
        if (inlier) PCC_HIP(hipMemcpyAsync(ix->host_b.p, dmask, no, hipMemcpyDeviceToHost, ix->stream));
    } else if (mean_dist) {
        PCC_HIP(hipMemcpyAsync(mean_dist, dmean, no * sizeof(float), hipMemcpyDeviceToDevice, ix->stream));
    }
    PCC_HIP(hipStreamSynchronize(ix->stream));
    double thr = hs.thr;
    size_t k_in = (size_t)hs.kept;
    if (!hs.exact) {
        // some addition of the in-order sums rounds (terms spread over more than 28 bits below the total): PCL's order
        // decides the last bits, so the sums are taken in that order -- on the host, as round 3 always did
        PCC_TRY(ix->host_a.reserve(no * sizeof(float)));
        PCC_TRY(ix->host_b.reserve(no));
        float* hm = ix->host_a.as<float>();
        uint8_t* hin = ix->host_b.as<uint8_t>();
        PCC_HIP(hipMemcpyAsync(hm, dmean, no * sizeof(float), hipMemcpyDeviceToHost, ix->stream));
        PCC_HIP(hipStreamSynchronize(ix->stream));
        PCC_TRY(sync_info(ix));
        sor_in_order(hm, no, ix->n_valid, K, stddev_mult, 0, no, &thr, &k_in, hin);
        if (mem == PCC_MEM_DEVICE && inlier) {
            PCC_HIP(hipMemcpyAsync(inlier, hin, no, hipMemcpyHostToDevice, ix->stream));
            PCC_HIP(hipStreamSynchronize(ix->stream));
        }
    }
    if (threshold) *threshold = thr;
    if (kept) *kept = k_in;
    if (mem == PCC_MEM_HOST) {
        if (mean_dist) memcpy(mean_dist, ix->host_a.p, no * sizeof(float));
        if (inlier) memcpy(inlier, ix->host_b.p, no);
    }
    ix->sor_exact_last = hs.exact != 0;
    return PCC_OK;
}

int pcc_index_sor_on_device(const pcc_index* ix, int* on_device) {
    if (!ix || !on_device) { set_error("null argument"); return PCC_ERR_INVALID; }
    *on_device = ix->sor_exact_last ? 1 : 0;
    return PCC_OK;
}

// mean distances of the points [start, start + count) of the indexed cloud (self query with mean_k + 1 neighbours, as
// pcc_sor) and this shard's share of PCL's statistics: sums[0] = sum of the means, [1] = sum of their float squares,
// [2], [3] = bit patterns (as doubles) of the smallest positive term of either sum (+inf's pattern when there is none).
// Combine over shards with (+, +, min, min) and hand the result to pcc_sor_threshold.
int pcc_sor_partial(pcc_index* ix, size_t start, size_t count, int mean_k, int mem, float* mean_dist, double sums[4]) {
    PCC_ENTER(ix);
    PCC_TRY(check_mem(mem));
    if (!sums) { set_error("null sums"); return PCC_ERR_INVALID; }
    float* dmean = nullptr;
    PCC_TRY(sor_begin(ix, start, count, mean_k));
    PCC_TRY(sor_means(ix, start, count, mean_k + 1, &dmean));
    PCC_TRY(ix->scratch_a.reserve(SOR_STATS_SCRATCH_BYTES));
    double* out4 = ix->scratch_a.as<double>() + SOR_STATS_OUT4;
    PCC_TRY(launch_sor_partial(ix->stream, dmean, count, ix->scratch_a.as<double>(), out4));
    PCC_HIP(hipMemcpyAsync(sums, out4, 4 * sizeof(double), hipMemcpyDeviceToHost, ix->stream));
    // (no Out / finish: the means leave the handle's own buffer by a plain copy in either memory space; `sums` needs the wait in both)
    if (mean_dist && count) PCC_TRY(copy_out(ix, mean_dist, dmean, count * sizeof(float), mem));
    PCC_HIP(hipStreamSynchronize(ix->stream));
    return PCC_OK;
}

// PCL's threshold from the combined sums of all shards (pure host arithmetic, no handle): *exact = 0 says that PCL's
// in-order additions would round -- the combined sums then need not be PCL's bits and the caller should take the
// sums of all mean distances in index order instead (pcc_sor does that on one GPU).
int pcc_sor_threshold(const double sums[4], uint64_t n_valid, int mean_k, double stddev_mult, double* threshold, int* exact) {
    if (!sums || !threshold || !exact) { set_error("null argument"); return PCC_ERR_INVALID; }
    sor_threshold_host(sums, (double)n_valid, mean_k + 1, stddev_mult, threshold, exact);
    return PCC_OK;
}
}  // extern "C"
