// vfh_device.hpp -- the device code pcc_vfh_descriptor (vfh.hip) and pcc_vfh_descriptors_batch (vfh_batch.hip) share: the record
// the centroid kernel leaves and the tile-parked centroid chains of ONE cloud in one wave.  One body: the batch call returns the single
// call's bits because it runs the single call's code.
#pragma once
#include <hip/hip_runtime.h>

#include "vfh_math.hpp"

namespace pcc {

// what the centroid kernel leaves for the kernels behind it
struct VfhRecord {
    float centroid[3], normal_centroid[3], d_vp_p[3];
    unsigned int cp;  // the points with a finite normal
};

// One wave (one 64-lane workgroup) for the cloud pts[0 .. n), nrm[0 .. n): the xyz centroid (compute3DCentroid: three float chains
// from 0.0f over the points in index order, each divided by float(n)) and the centroid of the normals (the same over the cp
// points whose normal has three finite components, divided by float(cp); cp == 0 gives 0.0f / 0.0f = NaN).  The tile-parking
// scheme of k_cd_centroids (cluster_desc.hip): the wave loads points and normals 64 at a time, coalesced, VFH_CENT_ROWS such
// rows in flight, and parks the six components in LDS; lanes 0 .. 5 then each carry one serial chain over the parked tile while
// the loads of the NEXT tile are under way.
// A normal that is skipped is parked as +0.0f in its three components and ADDED like the others: the chain stays one loop without a
// branch, and the addition leaves the accumulator's bits alone.  x + (+0.0f) == x bit for bit for every x but -0.0f, and a
// chain that starts at +0.0f never holds -0.0f: under round-to-nearest a sum is -0.0f only when both terms are -0.0f (an
// exact cancellation gives +0.0f), and the accumulator is never the first -0.0f term.
constexpr unsigned int VFH_CENT_ROWS = 8;
constexpr unsigned int VFH_CENT_TILE = 64 * VFH_CENT_ROWS;

// called by all 64 lanes of a 64-lane workgroup, n and the pointers workgroup-uniform; lane 0 writes *rec
__device__ __forceinline__ void vfh_centroid_chains(const float4* __restrict__ pts, const float4* __restrict__ nrm, unsigned int n,
                                                    VfhRecord* __restrict__ rec) {
    __shared__ __attribute__((aligned(16))) float park[6][VFH_CENT_TILE];
    __shared__ unsigned int cp_all;
    __shared__ float mean[6];
    const unsigned int lane = threadIdx.x;
    if (lane == 0) cp_all = 0u;
    float4 next_p[VFH_CENT_ROWS], next_n[VFH_CENT_ROWS];
    unsigned int mine = 0;  // finite normals this lane has loaded
    auto load = [&](unsigned int t0) {
#pragma unroll
        for (unsigned int r = 0; r < VFH_CENT_ROWS; ++r) {
            const unsigned int i = t0 + r * 64 + lane;
            const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
            next_p[r] = i < n ? pts[i] : zero;
            const float4 nv = i < n ? nrm[i] : zero;
            const bool use = i < n && fpfh_finite(nv.x) && fpfh_finite(nv.y) && fpfh_finite(nv.z);
            next_n[r] = use ? nv : zero;
            mine += use ? 1u : 0u;
        }
    };
    float acc = 0.0f;
    if (n) load(0);
    for (unsigned int t0 = 0; t0 < n; t0 += VFH_CENT_TILE) {
        const unsigned int tn = min(VFH_CENT_TILE, n - t0);
        __syncthreads();  // (the tile before has been added up)
#pragma unroll
        for (unsigned int r = 0; r < VFH_CENT_ROWS; ++r) {
            const unsigned int at = r * 64 + lane;
            park[0][at] = next_p[r].x; park[1][at] = next_p[r].y; park[2][at] = next_p[r].z;
            park[3][at] = next_n[r].x; park[4][at] = next_n[r].y; park[5][at] = next_n[r].z;
        }
        __syncthreads();
        if (t0 + VFH_CENT_TILE < n) load(t0 + VFH_CENT_TILE);
        if (lane < 6) {
            // the chain, 32 links at a time: eight 16-byte LDS reads in flight, then their additions in index order
            const float* __restrict__ row = park[lane];
            unsigned int j = 0;
            for (; j + 32 <= tn; j += 32) {
                float4 q[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) q[k] = *reinterpret_cast<const float4*>(row + j + 4 * k);
#pragma unroll
                for (int k = 0; k < 8; ++k) { acc += q[k].x; acc += q[k].y; acc += q[k].z; acc += q[k].w; }
            }
            for (; j < tn; ++j) acc += row[j];  // (entries at tn and beyond are not added)
        }
    }
    __syncthreads();  // (cp_all = 0 is visible)
    if (mine) atomicAdd(&cp_all, mine);
    __syncthreads();
    const unsigned int cp = cp_all;
    if (lane < 6) mean[lane] = acc / (lane < 3 ? (float)n : (float)cp);
    __syncthreads();
    if (lane == 0) {
        VfhRecord r;
        for (int k = 0; k < 3; ++k) { r.centroid[k] = mean[k]; r.normal_centroid[k] = mean[3 + k]; }
        vfh_view_direction(r.centroid, r.d_vp_p);
        r.cp = cp;
        *rec = r;
    }
}

}  // namespace pcc
