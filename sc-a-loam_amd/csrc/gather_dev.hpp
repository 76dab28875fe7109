// Moving stored keyframe clouds: the f32 rigid transform of a point and the gather table of the kernels that concatenate several
// keyframes: k_submap_gather (submap.hip, every loop check's submap) and k_pgo_gather (keyframes.hip, the pose-graph map).
#pragma once

namespace scal {

// One keyframe of a gather: output positions [dst, next entry's dst) are arena records src, src + 1, ... moved by m (row-major 3x4),
// or copied as they are when `copy` is set.  The table ends with a sentinel whose dst is the size of the output.
struct GatherXf {
    float m[12];
    int src, dst, copy, pad;
};

#ifdef __HIPCC__
// the last entry with dst <= i (entries of empty keyframes share their dst)
__device__ __forceinline__ int gather_find(const GatherXf* __restrict__ xf, int n_sel, int i) {
    int s = 0;
    for (int hi = n_sel - 1; s < hi;) {
        const int mid = (s + hi + 1) >> 1;
        if (xf[mid].dst <= i) s = mid;
        else hi = mid - 1;
    }
    return s;
}

// local2global (laserPosegraphOptimization.cpp:338-359): each coordinate ((m0 * x + m1 * y) + m2 * z) + m3 in f32, rounded operation by
// operation (Eigen's expression, no contraction); the intensity is kept.  The order of the sums is part of the interface.
__device__ __forceinline__ float4 xf_point(const float m[12], const float4 p) {
    float4 q;
    q.x = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], p.x), __fmul_rn(m[1], p.y)), __fmul_rn(m[2], p.z)), m[3]);
    q.y = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[4], p.x), __fmul_rn(m[5], p.y)), __fmul_rn(m[6], p.z)), m[7]);
    q.z = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[8], p.x), __fmul_rn(m[9], p.y)), __fmul_rn(m[10], p.z)), m[11]);
    q.w = p.w;
    return q;
}
#endif

}  // namespace scal
