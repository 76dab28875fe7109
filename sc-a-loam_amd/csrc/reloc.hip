// Relocalisation against a stored session (scal_reloc_*, include/scaloam_hip.h): the reference's "multi-session localization" TODO,
// built from the hooks it ships uncalled - saveScancontextAndKeys (Scancontext.cpp:236-246) reloads a session's descriptors,
// detectLoopClosureIDBetweenSession (:272-333) finds the place - and from the verification it runs for its own loops
// (loopFindNearKeyframesCloud / doICPVirtualRelative, laserPosegraphOptimization.cpp:472-548).
//
// One context = one session in HBM: every keyframe's VoxelGrid(leaf) cloud in an AoS xyzi arena (host-side offsets), its pose on the
// host, its descriptor in a ScanContext database.  Everything runs on ONE stream (lane 0: the voxel filter's kernels, the ScanContext
// context created with the shared layout, the ICP context), so a query is one launch chain and needs no events:
//   k_deinterleave -> voxel filter -> k_interleave4              the source
//   k_sc_bin, k_sc_finish                                        its descriptor (not inserted)
//   k_sc_keys, k_sc_topk, k_sc_detect                            scal_sc_detect_between_device
//   k_rl_submap -> k_deinterleave -> voxel filter -> k_interleave4   the target: keyframes c-h .. c+h, each in keyframe c's frame
//   scal_icp_align_guess_device                                  from Rz(-yaw)
#include "common.hpp"
#include "voxel_dev.hpp"
#include "gather_dev.hpp"
#include <algorithm>
#include <cmath>
#include <vector>

namespace scal {

// Streaming gather of a submap (GatherXf table; `copy` marks the candidate keyframe itself): one 16-byte load and one 16-byte store per
// point.  The table has at most 2 h + 2 entries (52 at the reference's h = 25): every thread finds its entry by bisection (six steps
// over a table that stays in cache) and re-reads the transform only when the entry changes along its grid-stride walk.
__global__ void __launch_bounds__(256) k_rl_submap(const float4* __restrict__ arena, const GatherXf* __restrict__ xf, int n_sel, int n,
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

}  // namespace scal

using namespace scal;

struct scal_reloc {
    scal_reloc_config cfg;  // zeros replaced by the defaults
    LaneStream stream;      // released by `delete c`, after scal_reloc_destroy has synchronised it
    scal_sc_t* sc = nullptr;
    scal_icp_t* icp = nullptr;
    CloudFilter cf;
    int work = 0;                          // records the work buffers hold (max_query_points)
    DevBuf<float4> arena, raw, ds_src, ds_tgt;
    DevBuf<double> d_desc;                 // the query's descriptor (single query)
    DevBuf<GatherXf> d_xf;
    PinBuf<GatherXf> h_xf;
    std::vector<int> off{0};               // arena offsets, one more than keyframes
    std::vector<double> poses;             // 12 per keyframe
    // query_batch: the filtered sources and descriptors of all queries (grown on demand)
    DevBuf<float4> b_src;
    DevBuf<double> b_desc;
    int size() const { return static_cast<int>(off.size()) - 1; }
};

extern "C" int scal_reloc_create(const scal_reloc_config* cfg, scal_reloc_t** out) {
    if (!cfg || !out || cfg->max_keyframes <= 0 || cfg->max_points <= 0 || cfg->max_query_points <= 0 || cfg->max_points > (1 << 30) ||
        cfg->max_query_points > (1 << 30) || !(cfg->sc_max_radius >= 0) || !(cfg->sc_dist_thres >= 0) || !(cfg->leaf >= 0.f) || std::isinf(cfg->leaf) ||
        cfg->submap_half < -1 || !(cfg->fitness_thres >= 0) || !(cfg->max_corr_dist >= 0) || !(cfg->transformation_epsilon >= 0) ||
        !(cfg->fitness_epsilon >= 0) || cfg->max_iterations < 0) {
        set_error("scal_reloc_create: bad argument");
        return SCAL_E_ARG;
    }
    *out = nullptr;
    SCAL_TRY(select_device(cfg->device));
    auto* c = new scal_reloc();
    c->cfg = *cfg;
    scal_reloc_config& g = c->cfg;
    if (g.sc_max_radius == 0) g.sc_max_radius = 80.0;
    if (g.sc_dist_thres == 0) g.sc_dist_thres = 0.2;
    if (g.leaf == 0.f) g.leaf = 0.4f;
    if (g.submap_half == 0) g.submap_half = 25;
    if (g.fitness_thres == 0) g.fitness_thres = 0.3;
    if (g.max_corr_dist == 0) g.max_corr_dist = 150.0;
    if (g.transformation_epsilon == 0) g.transformation_epsilon = 1e-6;
    if (g.fitness_epsilon == 0) g.fitness_epsilon = 1e-6;
    if (g.max_iterations == 0) g.max_iterations = 100;
    c->work = g.max_query_points;
    const size_t w = static_cast<size_t>(c->work);
    const int n_xf = (g.submap_half < 0 ? 0 : 2 * std::min(g.submap_half, g.max_keyframes)) + 2;
    int rc = SCAL_OK;
    auto A = [&](int r) { if (rc == SCAL_OK) rc = r; };
    A(c->stream.acquire(g.device, 0));
    // the arena and the clouds ICP reads in front of the filter's buffers: measured, queries are 0.4 % slower the other way round
    A(c->arena.alloc(static_cast<size_t>(g.max_points)));
    A(c->raw.alloc(w)); A(c->ds_src.alloc(w)); A(c->ds_tgt.alloc(w));
    A(c->cf.init(c->work));
    A(c->d_desc.alloc(1200)); A(c->d_xf.alloc(n_xf)); A(c->h_xf.alloc(n_xf));
    if (rc == SCAL_OK) {
        c->cf.set_tag(".R");
        scal_sc_config sc{};
        sc.max_radius = g.sc_max_radius, sc.dist_thres = g.sc_dist_thres, sc.max_keyframes = g.max_keyframes, sc.float_math = g.float_math;
        sc.device = g.device, sc.n_shards = 1;
        rc = sc_create(&sc, StreamLayout::Shared, &c->sc);  // lane 0: the stream of everything else in this context
    }
    if (rc == SCAL_OK) {
        scal_icp_config ic{};
        ic.max_corr_dist = g.max_corr_dist, ic.transformation_epsilon = g.transformation_epsilon, ic.fitness_epsilon = g.fitness_epsilon;
        ic.max_iterations = g.max_iterations, ic.max_source = c->work, ic.max_target = c->work, ic.device = g.device;
        rc = icp_create_on_lane(&ic, 0, &c->icp);
    }
    if (rc != SCAL_OK) {
        scal_reloc_destroy(c);
        return rc;
    }
    c->off.reserve(static_cast<size_t>(g.max_keyframes) + 1);
    c->poses.reserve(static_cast<size_t>(g.max_keyframes) * 12);
    *out = c;
    return SCAL_OK;
}

extern "C" void scal_reloc_destroy(scal_reloc_t* c) {
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->icp) scal_icp_destroy(c->icp);
    if (c->sc) scal_sc_destroy(c->sc);
    delete c;
}

extern "C" int scal_reloc_size(scal_reloc_t* c) {
    if (!c) return SCAL_E_ARG;
    return c->size();
}

extern "C" scal_sc_t* scal_reloc_sc(scal_reloc_t* c) { return c ? c->sc : nullptr; }

// VoxelGrid(leaf) of the n > 0 records loaded into the filter, exactly as scal_voxel_downsample_device runs it, into d_out; waits
static int reloc_filter(scal_reloc* c, int n, float4* d_out, int* n_out) {
    SCAL_TRY(c->cf.filter(c->stream, n, c->cfg.leaf));
    c->cf.store(c->stream, n, reinterpret_cast<float*>(d_out));
    const int m = c->cf.wait(c->stream, "scal_reloc");
    if (m < 0) return m;
    *n_out = m;
    return SCAL_OK;
}

static int reloc_check_cloud(scal_reloc* c, const char* who, const float* xyzi, int n) {
    if (n < 0 || (n > 0 && !xyzi)) {
        set_error("%s: bad argument", who);
        return SCAL_E_ARG;
    }
    if (n > c->work) {
        set_error("%s: cloud has %d points, max_query_points is %d", who, n, c->work);
        return SCAL_E_TOO_MANY;
    }
    return SCAL_OK;
}

extern "C" int scal_reloc_add_keyframe(scal_reloc_t* c, const float* xyzi, int n, const double pose12[12], const double* desc) {
    if (!c || !pose12) {
        set_error("scal_reloc_add_keyframe: bad argument");
        return SCAL_E_ARG;
    }
    SCAL_TRY(reloc_check_cloud(c, "scal_reloc_add_keyframe", xyzi, n));
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(pose12[k])) {
            set_error("scal_reloc_add_keyframe: the pose is not finite");
            return SCAL_E_ARG;
        }
    const int j = c->size();
    if (j >= c->cfg.max_keyframes) {
        set_error("scal_reloc_add_keyframe: the session is full (max_keyframes = %d)", c->cfg.max_keyframes);
        return SCAL_E_CAPACITY;
    }
    SCAL_HIP(hipSetDevice(c->cfg.device));
    hipStream_t s = c->stream;
    int m = 0;
    if (n > 0) {
        SCAL_HIP(hipMemcpyAsync(c->raw.p, xyzi, sizeof(float4) * static_cast<size_t>(n), hipMemcpyHostToDevice, s));
        SCAL_TRY(c->cf.load(s, reinterpret_cast<const float*>(c->raw.p), n));
        SCAL_TRY(reloc_filter(c, n, c->ds_src.p, &m));  // downSizeFilterScancontext (:629-631)
    }
    if (m > c->cfg.max_points - c->off[j]) {
        set_error("scal_reloc_add_keyframe: the cloud store is full (max_points = %d, keyframe %d has %d points after the filter)", c->cfg.max_points,
                  j, m);
        return SCAL_E_CAPACITY;
    }
    // the descriptor first: a full database must leave nothing stored
    if (desc) {
        SCAL_TRY(scal_sc_insert_descriptor(c->sc, desc));  // saveScancontextAndKeys
    } else {
        // an empty cloud: the filter did not run, the count it would have left is zero
        if (m == 0) SCAL_HIP(hipMemsetAsync(c->cf.d_n_out(), 0, sizeof(int), s));
        const SoA4 o = c->cf.out();
        SCAL_TRY(scal_sc_insert_cloud_device(c->sc, o.x, o.y, o.z, c->cf.d_n_out(), m));  // makeAndSaveScancontextAndKeys (:639)
    }
    if (m > 0) SCAL_HIP(hipMemcpyAsync(c->arena.p + c->off[j], c->ds_src.p, sizeof(float4) * static_cast<size_t>(m), hipMemcpyDeviceToDevice, s));
    SCAL_HIP(hipStreamSynchronize(s));
    c->off.push_back(c->off[j] + m);
    c->poses.insert(c->poses.end(), pose12, pose12 + 12);
    return j;
}

// M = Pc^-1 Pj as an f32 3x4 (the order of the sums is part of the interface: include/scaloam_hip.h)
static void reloc_relative(const double* Pc, const double* Pj, float* m) {
    double Ri[3][3], ti[3];
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) Ri[r][k] = Pc[4 * k + r];
    for (int r = 0; r < 3; ++r) ti[r] = -((Ri[r][0] * Pc[3] + Ri[r][1] * Pc[7]) + Ri[r][2] * Pc[11]);
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 4; ++k) {
            double v = (Ri[r][0] * Pj[k] + Ri[r][1] * Pj[4 + k]) + Ri[r][2] * Pj[8 + k];
            if (k == 3) v += ti[r];
            m[4 * r + k] = static_cast<float>(v);
        }
}

// steps 4-7 for one query whose filtered source (n_src records at d_src) and search result (out->sc) are known
static int reloc_verify(scal_reloc* c, const float4* d_src, int n_src, scal_reloc_result* out) {
    out->n_src = n_src;
    const int cand = out->sc.loop_id;
    if (cand < 0) return SCAL_OK;  // status 0
    hipStream_t s = c->stream;
    const int h = c->cfg.submap_half < 0 ? 0 : c->cfg.submap_half;
    const int j0 = std::max(0, cand - h), j1 = std::min(c->size() - 1, cand + h);
    const long long n_raw = static_cast<long long>(c->off[j1 + 1]) - c->off[j0];
    if (n_raw > c->work) {
        set_error("scal_reloc_query: the submap of keyframes %d..%d has %lld points, max_query_points is %d", j0, j1, n_raw, c->work);
        return SCAL_E_CAPACITY;
    }
    const double* Pc = c->poses.data() + 12 * static_cast<size_t>(cand);
    int n_sel = 0, dst = 0;
    for (int j = j0; j <= j1; ++j, ++n_sel) {
        GatherXf& e = c->h_xf.p[n_sel];
        e.src = c->off[j], e.dst = dst, e.copy = j == cand ? 1 : 0, e.pad = 0;
        reloc_relative(Pc, c->poses.data() + 12 * static_cast<size_t>(j), e.m);
        dst += c->off[j + 1] - c->off[j];
    }
    GatherXf& end = c->h_xf.p[n_sel];
    std::memset(&end, 0, sizeof end);
    end.dst = dst, end.copy = 1;
    const int n = dst;
    int n_tgt = 0;
    if (n > 0) {
        SCAL_HIP(hipMemcpyAsync(c->d_xf.p, c->h_xf.p, sizeof(GatherXf) * (static_cast<size_t>(n_sel) + 1), hipMemcpyHostToDevice, s));
        SCAL_LAUNCH_PROF("k_rl_submap", k_rl_submap, dim3(std::min(div_up(n, 256), 1024)), dim3(256), 0, s, c->arena.p, c->d_xf.p, n_sel, n, c->raw.p,
                         c->cf.d_n_in());
        SCAL_HIP(hipGetLastError());
        c->cf.load_counted(s, reinterpret_cast<const float*>(c->raw.p), n);
        SCAL_TRY(reloc_filter(c, n, c->ds_tgt.p, &n_tgt));  // downSizeFilterICP (:491-492)
    }
    out->n_tgt = n_tgt;
    float G[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (!c->cfg.no_yaw_guess) {  // Rz(-yaw)
        const float cs = static_cast<float>(std::cos(static_cast<double>(out->sc.yaw_rad))), sn = static_cast<float>(std::sin(static_cast<double>(out->sc.yaw_rad)));
        G[0] = cs, G[1] = sn, G[4] = -sn, G[5] = cs;
    }
    SCAL_TRY(scal_icp_align_guess_device(c->icp, reinterpret_cast<const float*>(d_src), n_src, reinterpret_cast<const float*>(c->ds_tgt.p), n_tgt, G,
                                         &out->icp));
    out->status = (out->icp.converged && out->icp.fitness <= c->cfg.fitness_thres) ? 1 : 2;
    const double* T = out->icp.T;
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 4; ++k) {
            double v = (Pc[4 * r] * T[k] + Pc[4 * r + 1] * T[4 + k]) + Pc[4 * r + 2] * T[8 + k];
            if (k == 3) v += Pc[4 * r + 3];
            out->pose12[4 * r + k] = v;
        }
    return SCAL_OK;
}

// steps 1-2 for one query: filtered source -> d_src, descriptor -> d_desc (queued, not waited for)
static int reloc_front(scal_reloc* c, const float* xyzi, int n, float4* d_src, double* d_desc, int* n_src) {
    hipStream_t s = c->stream;
    *n_src = 0;
    if (n > 0) {
        SCAL_HIP(hipMemcpyAsync(c->raw.p, xyzi, sizeof(float4) * static_cast<size_t>(n), hipMemcpyHostToDevice, s));
        SCAL_TRY(c->cf.load(s, reinterpret_cast<const float*>(c->raw.p), n));
        SCAL_TRY(reloc_filter(c, n, d_src, n_src));
    } else {  // no pinned word involved: nothing waits for this before the next query's filter writes its own count
        SCAL_HIP(hipMemsetAsync(c->cf.d_n_out(), 0, sizeof(int), s));
    }
    const SoA4 o = c->cf.out();
    return sc_make_cloud_device(c->sc, o.x, o.y, o.z, c->cf.d_n_out(), *n_src, d_desc);
}

extern "C" int scal_reloc_query(scal_reloc_t* c, const float* xyzi, int n, scal_reloc_result* out) {
    if (!c || !out) {
        set_error("scal_reloc_query: bad argument");
        return SCAL_E_ARG;
    }
    SCAL_TRY(reloc_check_cloud(c, "scal_reloc_query", xyzi, n));
    std::memset(out, 0, sizeof *out);
    if (c->size() == 0) {
        set_error("scal_reloc_query: no keyframe stored");
        return SCAL_E_STATE;
    }
    SCAL_HIP(hipSetDevice(c->cfg.device));
    int n_src = 0;
    SCAL_TRY(reloc_front(c, xyzi, n, c->ds_src.p, c->d_desc.p, &n_src));
    SCAL_TRY(scal_sc_detect_between_device(c->sc, c->d_desc.p, 1, &out->sc));
    return reloc_verify(c, c->ds_src.p, n_src, out);
}

extern "C" int scal_reloc_query_batch(scal_reloc_t* c, const float* xyzi, const int* offsets, int nq, scal_reloc_result* out) {
    if (!c || !offsets || nq < 0 || (nq > 0 && !out) || offsets[0] != 0) {
        set_error("scal_reloc_query_batch: bad argument");
        return SCAL_E_ARG;
    }
    for (int q = 0; q < nq; ++q) {
        if (offsets[q + 1] < offsets[q]) {
            set_error("scal_reloc_query_batch: offsets must not decrease");
            return SCAL_E_ARG;
        }
        SCAL_TRY(reloc_check_cloud(c, "scal_reloc_query_batch", xyzi, offsets[q + 1] - offsets[q]));
    }
    if (nq == 0) return SCAL_OK;
    std::memset(out, 0, sizeof *out * static_cast<size_t>(nq));
    if (c->size() == 0) {
        set_error("scal_reloc_query_batch: no keyframe stored");
        return SCAL_E_STATE;
    }
    SCAL_HIP(hipSetDevice(c->cfg.device));
    // a filtered cloud is no larger than the cloud: the sources of all queries fit in as many records as the batch has
    const size_t total = static_cast<size_t>(offsets[nq]);
    if (c->b_src.n < total || !c->b_src.p) {
        SCAL_HIP(hipStreamSynchronize(c->stream));
        SCAL_TRY(c->b_src.alloc(total));
    }
    if (c->b_desc.n < static_cast<size_t>(nq) * 1200 || !c->b_desc.p) {
        SCAL_HIP(hipStreamSynchronize(c->stream));
        SCAL_TRY(c->b_desc.alloc(static_cast<size_t>(nq) * 1200));
    }
    std::vector<int> src_off(static_cast<size_t>(nq) + 1, 0);
    for (int q = 0; q < nq; ++q) {
        int n_src = 0;
        SCAL_TRY(reloc_front(c, xyzi + 4 * static_cast<size_t>(offsets[q]), offsets[q + 1] - offsets[q], c->b_src.p + src_off[q],
                             c->b_desc.p + 1200 * static_cast<size_t>(q), &n_src));
        src_off[q + 1] = src_off[q] + n_src;
    }
    std::vector<scal_sc_result> found(static_cast<size_t>(nq));
    SCAL_TRY(scal_sc_detect_between_device(c->sc, c->b_desc.p, nq, found.data()));
    for (int q = 0; q < nq; ++q) {
        out[q].sc = found[q];
        SCAL_TRY(reloc_verify(c, c->b_src.p + src_off[q], src_off[q + 1] - src_off[q], &out[q]));
    }
    return SCAL_OK;
}
