// Host side of lm_dev.hpp, shared by stage B (odometry.hip) and stage C (mapping.hip): the buffers a context's solves work on and the
// back end of its Ceres-adapter mode.  A header, because the kernels of lm_dev.hpp are static per translation unit (SCAL_KERNEL).
// The extern "C" entry points keep their own argument and state checks, error texts and hipSetDevice.
#pragma once
#include <algorithm>
#include "common.hpp"
#include "voxel_dev.hpp"
#include "lm_dev.hpp"

namespace scal {

// Hamilton product and rotation of quaternions stored x y z w (Eigen's operator* / _transformVector term by term); the mapping
// kernels that call them reproduce the reference's rounding bit for bit
__host__ __device__ inline void q_mul(const double* a, const double* b, double* o) {
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
__host__ __device__ inline void q_rot(const double* q, const double* v, double* o) {
    double ux = q[1] * v[2] - q[2] * v[1], uy = q[2] * v[0] - q[0] * v[2], uz = q[0] * v[1] - q[1] * v[0];
    ux += ux, uy += uy, uz += uz;
    const double cx = q[1] * uz - q[2] * uy, cy = q[2] * ux - q[0] * uz, cz = q[0] * uy - q[1] * ux;
    o[0] = (v[0] + q[3] * ux) + cx, o[1] = (v[1] + q[3] * uy) + cy, o[2] = (v[2] + q[3] * uz) + cz;
}

// a cloud as four device columns x[] y[] z[] intensity[]
struct SoAStore {
    DevBuf<float> x, y, z, w;
    int alloc(size_t n) {
        SCAL_TRY(x.alloc(n));
        SCAL_TRY(y.alloc(n));
        SCAL_TRY(z.alloc(n));
        SCAL_TRY(w.alloc(n));
        return SCAL_OK;
    }
    SoA4 v() { return SoA4{x.p, y.p, z.p, w.p}; }
    CSoA4 cv() const { return CSoA4{x.p, y.p, z.p, w.p}; }
};

// What launch_lm_solve works on: the residual-block slots, the workgroups' exchange (partials + LMSync) and the solver state.
struct LMStore {
    DevBuf<int> fvalid, fkind;
    DevBuf<double> fcp, fpa, fpb, partials;
    DevBuf<LMSync> lm_sync;
    DevBuf<LMState> d_st;
    int slot_cap = 0;
    int alloc(int slots) {
        slot_cap = slots;
        const size_t sc = slots;
        SCAL_TRY(fvalid.alloc(sc));
        SCAL_TRY(fkind.alloc(sc));
        SCAL_TRY(fcp.alloc(3 * sc));
        SCAL_TRY(fpa.alloc(3 * sc));
        SCAL_TRY(fpb.alloc(3 * sc));
        SCAL_TRY(partials.alloc(LM_PARTIAL_WORDS));
        SCAL_TRY(lm_sync.alloc(1));
        return d_st.alloc(1);
    }
    // on the context's own stream (the legacy null stream is not ordered against it)
    int init(hipStream_t s) {
        SCAL_HIP(op_memset_async(lm_sync.p, 0, sizeof(LMSync), s));
        SCAL_TRY(partials.zero(s));  // sequence number 0 = never published
        SCAL_HIP(op_memset_async(d_st.p, 0, sizeof(LMState), s));
        return SCAL_OK;
    }
    FactorSoA factors() { return FactorSoA{fvalid.p, fkind.p, fcp.p, fpa.p, fpb.p, slot_cap}; }
    // after an abandoned solve, once everything queued on `s` has drained: the sticky flag and the tagged words go back to "never published"
    int clear_exchange(hipStream_t s) {
        SCAL_HIP(op_stream_synchronize(s));
        SCAL_HIP(op_memset_async(lm_sync.p, 0, sizeof(LMSync), s));
        SCAL_TRY(partials.zero(s));
        SCAL_HIP(op_stream_synchronize(s));
        return SCAL_OK;
    }
};

// Ceres-adapter mode: the live blocks of a FactorSoA compacted, exported as scal_block records and evaluated in batches
// at the host solver's pose.  The pinned h_x7 is rewritten only behind a stream synchronisation.
struct BlockAdapter {
    static_assert(sizeof(scal_block) == 80, "scal_block layout (k_blocks_export writes 10 doubles per block)");
    DevBuf<int> bl_live, bl_rowoff, bl_counts;
    DevBuf<double> d_x7, d_res, d_jac, d_blocks;
    PinBuf<int> h_counts;   // [0] live blocks, [1] residual rows of the last compact()
    PinBuf<double> h_x7;
    int alloc(int slots) {
        const size_t sc = slots;
        SCAL_TRY(bl_live.alloc(sc));
        SCAL_TRY(bl_rowoff.alloc(sc + 1));
        SCAL_TRY(bl_counts.alloc(2));
        SCAL_TRY(h_counts.alloc(2));
        SCAL_TRY(h_x7.alloc(8));
        SCAL_TRY(d_x7.alloc(8));
        SCAL_TRY(d_res.alloc(3 * sc));
        SCAL_TRY(d_jac.alloc(21 * sc));
        h_counts.p[0] = h_counts.p[1] = 0;
        return d_blocks.alloc(10 * sc);
    }
    BlockList block_list() { return BlockList{bl_live.p, bl_rowoff.p, bl_counts.p}; }
    int n_blocks() const { return h_counts.p[0]; }
    int n_residuals() const { return h_counts.p[1]; }
    void set_empty() { h_counts.p[0] = h_counts.p[1] = 0; }
    // queues the compaction and the copy of the two counts; they are valid once the caller has synchronised `s`
    int compact(hipStream_t s, const FactorSoA& F, const int* d_nslots) {
        SCAL_LAUNCH("k_blocks_compact", k_blocks_compact, dim3(1), dim3(1024), 0, s, F, d_nslots, block_list());
        SCAL_HIP(hipGetLastError());
        SCAL_HIP(op_memcpy_async(h_counts.p, bl_counts.p, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
        return SCAL_OK;
    }
    // q (4) and t (3) to the 7 doubles at d_x
    int set_pose(hipStream_t s, double* d_x, const double* q, const double* t) {
        SCAL_HIP(op_stream_synchronize(s));
        for (int i = 0; i < 4; ++i) h_x7.p[i] = q[i];
        for (int i = 0; i < 3; ++i) h_x7.p[4 + i] = t[i];
        SCAL_HIP(op_memcpy_async(d_x, h_x7.p, sizeof(double) * 7, hipMemcpyHostToDevice, s));
        return SCAL_OK;
    }
    // the first min(cap, n_blocks()) blocks; returns their number
    int get_blocks(hipStream_t s, const FactorSoA& F, scal_block* out, int cap) {
        const int n = std::min(cap, n_blocks());
        if (n <= 0) return 0;
        SCAL_LAUNCH("k_blocks_export", k_blocks_export, dim3(div_up(n_blocks(), 256)), dim3(256), 0, s, F, block_list(), d_blocks.p);
        SCAL_HIP(op_memcpy_async(out, d_blocks.p, sizeof(scal_block) * n, hipMemcpyDeviceToHost, s));
        SCAL_HIP(op_stream_synchronize(s));
        return n;
    }
    int eval_blocks(hipStream_t s, const FactorSoA& F, const double* x7, int want_jac, double* residuals, double* jacobians) {
        const int nb = n_blocks(), nr = n_residuals();
        if (nb == 0) return SCAL_OK;
        SCAL_HIP(op_stream_synchronize(s));
        for (int i = 0; i < 7; ++i) h_x7.p[i] = x7[i];
        SCAL_HIP(op_memcpy_async(d_x7.p, h_x7.p, sizeof(double) * 7, hipMemcpyHostToDevice, s));
        SCAL_LAUNCH("k_blocks_eval", k_blocks_eval, dim3(div_up(nb, 256)), dim3(256), 0, s, F, block_list(), d_x7.p, want_jac ? 1 : 0, d_res.p, d_jac.p);
        SCAL_HIP(hipGetLastError());
        SCAL_HIP(op_memcpy_async(residuals, d_res.p, sizeof(double) * nr, hipMemcpyDeviceToHost, s));
        if (want_jac) SCAL_HIP(op_memcpy_async(jacobians, d_jac.p, sizeof(double) * 7 * nr, hipMemcpyDeviceToHost, s));
        SCAL_HIP(op_stream_synchronize(s));
        return SCAL_OK;
    }
};

}  // namespace scal
