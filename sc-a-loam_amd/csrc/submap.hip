// The shared loop check (submap.hpp): k_submap_gather -> k_deinterleave -> voxel filter -> k_interleave4, then the ICP.
// k_pgo_gather (keyframes.hip) reads the same table and is deliberately NOT folded in: it writes the filter's SoA planes and bounding-box
// parts in the same pass over millions of points, and that fusion was measured.
#include "submap.hpp"
#include <algorithm>

namespace scal {

// Streaming gather of a submap (GatherXf table; `copy` marks a keyframe taken as it is): one 16-byte load and one 16-byte store per
// point.  The table has at most 2 h + 2 entries (52 at the reference's h = 25): every thread finds its entry by bisection (six steps
// over a table that stays in cache) and re-reads the transform only when the entry changes along its grid-stride walk.
__global__ void __launch_bounds__(256) k_submap_gather(const float4* __restrict__ arena, const GatherXf* __restrict__ xf, int n_sel, int n,
                                                       float4* __restrict__ out, int* __restrict__ d_n) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *d_n = n;  // the filter's device-side count
    int cur = -1, s_src = 0, s_dst = 0, s_copy = 1;
    float T[12];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int s = gather_find(xf, n_sel, i);
        if (s != cur) {
            cur = s;
            s_src = xf[s].src, s_dst = xf[s].dst, s_copy = xf[s].copy;
#pragma unroll
            for (int k = 0; k < 12; ++k) T[k] = xf[s].m[k];
        }
        const float4 p = arena[s_src + (i - s_dst)];
        out[i] = s_copy ? p : xf_point(T, p);
    }
}

int SubmapVerifier::init(int device, int lane, int capacity, int table_entries, float leaf_m, scal_icp_config ic, const char* tag, const char* who_) {
    leaf = leaf_m, who = who_;
    // the clouds ICP reads in front of the filter's buffers: measured in scal_reloc, queries are 0.4 % slower the other way round
    for (DevBuf<float4>* b : {&raw, &ds_src, &ds_tgt}) SCAL_TRY(b->alloc(static_cast<size_t>(capacity)));
    SCAL_TRY(cf.init(capacity));
    cf.set_tag(tag);
    SCAL_TRY(d_xf.alloc(static_cast<size_t>(table_entries)));
    SCAL_TRY(h_xf.alloc(static_cast<size_t>(table_entries)));
    ic.max_source = capacity, ic.max_target = capacity, ic.device = device;
    return icp_create_on_lane(&ic, lane, &icp);
}

int SubmapVerifier::filter(hipStream_t s, int n, float4* d_out) {
    SCAL_TRY(cf.filter(s, n, leaf));
    cf.store(s, n, reinterpret_cast<float*>(d_out));
    return cf.wait(s, who);
}

int SubmapVerifier::gather_filter(hipStream_t s, const float4* arena, int n_sel, float4* d_out) {
    const int n = h_xf.p[n_sel].dst;
    if (n <= 0) return 0;
    SCAL_HIP(hipMemcpyAsync(d_xf.p, h_xf.p, sizeof(GatherXf) * (static_cast<size_t>(n_sel) + 1), hipMemcpyHostToDevice, s));
    SCAL_LAUNCH_PROF("k_submap_gather", k_submap_gather, dim3(std::min(div_up(n, 256), 1024)), dim3(256), 0, s, arena, d_xf.p, n_sel, n, raw.p,
                     cf.d_n_in());
    SCAL_HIP(hipGetLastError());
    cf.load_counted(s, reinterpret_cast<const float*>(raw.p), n);
    return filter(s, n, d_out);
}

}  // namespace scal
