// range_batch.hip -- what the batch calls over ranges of ONE array of records share on the device (gfx950):
// the argument checks 1 - 4 of pcc_fpfh_descriptors_batch and pcc_vfh_descriptors_batch (check_range_batch) and the staging of
// the batch route as one concatenated cloud (stage_ranges: one pinned buffer, one copy, for a device caller k_range_pack).
// Routes, upload layout and host pack: range_batch_plan.hpp; declarations and the loop over the work handle: entry.hpp.
#include "entry.hpp"
#include "lane_ops.hpp"

namespace pcc {

namespace {

// ---- the pack from device memory --------------------------------------------------------------------------------------------
// Point e of the concatenation lies in cluster c = the last one with bases[c] <= e (a cluster off the batch route is empty here
// and never the answer) and is the caller's record src[c] + (e - bases[c]): out[e] = x, y, z, w = bits(e).  V16: the records are
// 16-byte aligned and a multiple of 16 bytes apart: x, y, z in one load; else three scalar loads.  FLAG: a non-finite point
// leaves its cluster's number in *bad when no lower one is there (bad is not read without FLAG).
template <bool V16, bool FLAG>
__global__ void __launch_bounds__(256)
k_range_pack(const unsigned char* __restrict__ pts, size_t stride, const unsigned int* __restrict__ src, const unsigned int* __restrict__ bases,
             unsigned int n_clusters, unsigned int total, float4* __restrict__ out, unsigned int* __restrict__ bad) {
    for (unsigned int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const unsigned int c = range_of(bases, n_clusters, e);
        const size_t rec = (size_t)src[c] + (e - bases[c]);
        float x, y, z;
        if constexpr (V16) {
            const float4 v = *reinterpret_cast<const float4*>(pts + rec * stride);
            x = v.x; y = v.y; z = v.z;
        } else {
            const float* v = reinterpret_cast<const float*>(pts + rec * stride);
            x = v[0]; y = v[1]; z = v[2];
        }
        if constexpr (FLAG)
            if (!finite3(x, y, z)) atomicMin(bad, c);
        out[e] = make_float4(x, y, z, __uint_as_float(e));
    }
}

}  // namespace

int check_range_batch(const ClusterRanges& r, const size_t* out_offsets, std::initializer_list<const void*> outs) {
    // 1. the memory space
    PCC_TRY(check_mem(r.mem));
    // 2. null arrays (the clusters' arrays may be null while no cluster holds a point)
    if (!r.offsets || !out_offsets) { set_error("null argument"); return PCC_ERR_INVALID; }
    bool null_array = !r.pts, misaligned = reinterpret_cast<uintptr_t>(r.pts) % 4 != 0;
    for (const void* out : outs) {
        null_array |= !out;
        misaligned |= reinterpret_cast<uintptr_t>(out) % 4 != 0;
    }
    const bool any_points = r.n_clusters && r.offsets[r.n_clusters] != r.offsets[0];
    if (any_points && null_array) { set_error("null argument"); return PCC_ERR_INVALID; }
    // 3. the stride and the alignment
    PCC_TRY(check_points(nullptr, 0, r.stride, r.mem));  // (the stride alone)
    if (misaligned) { set_error("points and descriptors must be 4-byte aligned"); return PCC_ERR_INVALID; }
    // 4. the offsets
    return check_cluster_offsets({{r.offsets, r.n_clusters}}, "points in one batch");
}

int stage_ranges(pcc_index* ix, RangeStaging& b, const ClusterRanges& r, const RangeBatchPlan& plan, size_t extra_bytes,
                 const std::function<void(char*)>& fill_extra, bool flag_non_finite, RangeStaged* staged) {
    static_assert(sizeof(GridDev) == RANGE_GRID_BYTES && RANGE_GRID_BYTES % 16 == 0 && offsetof(GridDev, n_valid) == RANGE_GRID_N_VALID_AT,
                  "range_batch_plan.hpp lays the upload out behind a GridDev it cannot see");
    hipStream_t s = ix->stream;
    const bool host = r.mem == PCC_MEM_HOST;
    const RangeUpload up(plan, extra_bytes);
    PCC_TRY(b.up.reserve(up.bytes(host)));
    PCC_TRY(b.dev.reserve(up.device_bytes()));
    char *u = b.up.as<char>(), *d = b.dev.as<char>();
    *staged = RangeStaged{reinterpret_cast<const GridDev*>(d), up.src(d), up.bases(d), up.items(d), (unsigned int)plan.items.size(),
                          reinterpret_cast<float4*>(up.pts(d)), plan.total(), up.extra(d), RANGE_FLAG_NONE, nullptr};
    // (a host caller's points pass through the pack loop: with the flag, a non-finite one refuses the call before any launch)
    size_t bad = 0;
    if (!up.fill(u, r, plan, host, flag_non_finite, &bad)) { staged->host_bad = (unsigned int)bad; return PCC_OK; }
    if (fill_extra) fill_extra(up.extra(u));
    unsigned int *h_flag = nullptr, *d_flag = nullptr;
    if (flag_non_finite) {
        PCC_TRY(b.flag.reserve(sizeof(unsigned int)));
        PCC_TRY(b.down.reserve(sizeof(unsigned int)));
        d_flag = b.flag.as<unsigned int>();
        staged->h_flag = h_flag = b.down.as<unsigned int>();
        *h_flag = RANGE_FLAG_NONE;
    }
    PCC_HIP(hipMemcpyAsync(d, u, up.bytes(host), hipMemcpyHostToDevice, s));
    if (host) return PCC_OK;

    const unsigned char* p0 = r.cluster(0);
    const bool v16 = r.stride % 16 == 0 && reinterpret_cast<uintptr_t>(p0) % 16 == 0;
    if (flag_non_finite) PCC_HIP(hipMemsetAsync(d_flag, 0xff, sizeof(unsigned int), s));
    const auto pack = flag_non_finite ? (v16 ? k_range_pack<true, true> : k_range_pack<false, true>)
                                      : (v16 ? k_range_pack<true, false> : k_range_pack<false, false>);
    hipLaunchKernelGGL(pack, dim3(blocks_for(staged->total)), dim3(256), 0, s, p0, r.stride, staged->d_src, staged->d_bases,
                       (unsigned int)r.n_clusters, (unsigned int)staged->total, staged->d_pts, d_flag);
    PCC_HIP(hipGetLastError());
    // (the flag word on its way down beside the next wait's word: no wait of its own)
    if (flag_non_finite) PCC_HIP(hipMemcpyAsync(h_flag, d_flag, sizeof(unsigned int), hipMemcpyDeviceToHost, s));
    return PCC_OK;
}

}  // namespace pcc
