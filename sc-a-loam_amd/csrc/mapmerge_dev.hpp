// The map merge's per-point arithmetic (mapmerge.hip), shared with the multiview refine (refine.hip), which must move a keyframe
// into the global frame with exactly the bits a scal_mapmerge_add of that frame gives: near-range rule, f64 rigid transform in the
// order of a column-major 4x4 product, ballot-ranked stable write.  A workgroup handles MM_TILE consecutive points of ONE frame.
#pragma once
#include "common.hpp"
#include "device_utils.hpp"

namespace scal {

struct MMBlock {
    int first;  // first point of the workgroup in the concatenated input
    int end;    // end of its frame
    int frame;
};

__device__ __forceinline__ bool mm_keep(const float4& p, double thres) {
    const double x = p.x, y = p.y, z = p.z;
    return sqrt((x * x + y * y) + z * z) > thres;  // LA.norm(local, axis=1) > thres_near_removal (makeMergedMap.py:109, :112)
}

constexpr int MM_ITEMS = 4;                 // points per thread
constexpr int MM_TILE = 256 * MM_ITEMS;    // points per workgroup; point (j, t) of a workgroup = first + j*256 + t

// kept points of the workgroup -> blkcnt[blockIdx.x]
__device__ __forceinline__ void mm_count_body(const float4* __restrict__ in, const MMBlock* __restrict__ blocks, double thres,
                                              int* __restrict__ blkcnt) {
    __shared__ int s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const MMBlock b = blocks[blockIdx.x];
    int mine = 0;
#pragma unroll
    for (int j = 0; j < MM_ITEMS; ++j) {
        const int i = b.first + j * 256 + threadIdx.x;
        const bool keep = i < b.end && mm_keep(in[i], thres);
        mine += __popcll(__ballot(keep));
    }
    if (lane_id() == 0 && mine) atomicAdd(&s_cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) blkcnt[blockIdx.x] = s_cnt;
}

// the kept points of the workgroup, moved, to out[base + blkoff[blockIdx.x] + rank]; WITH_FRAME: their frame beside them
template <bool WITH_FRAME>
__device__ __forceinline__ void mm_write_body(const float4* __restrict__ in, const MMBlock* __restrict__ blocks, const double* __restrict__ poses,
                                              double thres, const int* __restrict__ blkoff, long long base, long long cap,
                                              float4* __restrict__ out, int* __restrict__ frame_of) {
    __shared__ int s_cnt[MM_ITEMS][4];
    const MMBlock b = blocks[blockIdx.x];
    const int w = wave_id();
    float4 p[MM_ITEMS];
    bool keep[MM_ITEMS];
    int rank[MM_ITEMS];
#pragma unroll
    for (int j = 0; j < MM_ITEMS; ++j) {
        const int i = b.first + j * 256 + threadIdx.x;
        keep[j] = false;
        if (i < b.end) {
            p[j] = in[i];
            keep[j] = mm_keep(p[j], thres);
        }
        const uint64_t m = __ballot(keep[j]);
        rank[j] = __popcll(m & lanemask_lt());
        if (lane_id() == 0) s_cnt[j][w] = __popcll(m);
    }
    __syncthreads();
    const double* T = poses + 12 * b.frame;
    int before = 0;  // kept points of the workgroup in front of (j, wave w)
#pragma unroll
    for (int j = 0; j < MM_ITEMS; ++j) {
        int mine = before;
        for (int q = 0; q < w; ++q) mine += s_cnt[j][q];
        before += s_cnt[j][0] + s_cnt[j][1] + s_cnt[j][2] + s_cnt[j][3];
        if (!keep[j]) continue;
        const long long o = base + blkoff[blockIdx.x] + mine + rank[j];
        if (o >= cap) continue;  // k_mm_scan has flagged the overflow
        const double x = p[j].x, y = p[j].y, z = p[j].z;
        float4 g;  // T * [x y z 1]^T, column-major product order; the 4th row is (0 0 0 1), so the division by w is by 1
        g.x = static_cast<float>(((T[0] * x + T[1] * y) + T[2] * z) + T[3]);
        g.y = static_cast<float>(((T[4] * x + T[5] * y) + T[6] * z) + T[7]);
        g.z = static_cast<float>(((T[8] * x + T[9] * y) + T[10] * z) + T[11]);
        g.w = p[j].w;
        out[o] = g;
        if (WITH_FRAME) frame_of[o] = b.frame;
    }
}

}  // namespace scal
