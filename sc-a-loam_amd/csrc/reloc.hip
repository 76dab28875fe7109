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
//   SubmapVerifier::gather_filter (submap.hip)                   the target: keyframes c-h .. c+h, each in keyframe c's frame
//   SubmapVerifier::align                                        from Rz(-yaw)
// The verifier (filter, work clouds, gather table, ICP context) is shared with scal_pipeline's keyframe mode; the table's contents are not.
#include "submap.hpp"
#include <algorithm>
#include <cmath>
#include <vector>

using namespace scal;

struct scal_reloc {
    scal_reloc_config cfg;  // zeros replaced by the defaults
    LaneStream stream;      // released by `delete c`, after scal_reloc_destroy has synchronised it
    scal_sc_t* sc = nullptr;
    int work = 0;                          // records the work buffers hold (max_query_points)
    DevBuf<float4> arena;
    SubmapVerifier v;                      // filter, raw / ds_src / ds_tgt, gather table, ICP context
    DevBuf<double> d_desc;                 // the query's descriptor (single query)
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
    if (g.leaf == 0.f) g.leaf = LOOP_LEAF;
    if (g.submap_half == 0) g.submap_half = LOOP_SUBMAP_HALF;
    if (g.fitness_thres == 0) g.fitness_thres = LOOP_FITNESS_THRES;
    if (g.max_corr_dist == 0) g.max_corr_dist = LOOP_ICP_MAX_CORR_DIST;
    if (g.transformation_epsilon == 0) g.transformation_epsilon = LOOP_ICP_TRANSFORMATION_EPS;
    if (g.fitness_epsilon == 0) g.fitness_epsilon = LOOP_ICP_FITNESS_EPS;
    if (g.max_iterations == 0) g.max_iterations = LOOP_ICP_MAX_ITERATIONS;
    c->work = g.max_query_points;
    const int n_xf = (g.submap_half < 0 ? 0 : 2 * std::min(g.submap_half, g.max_keyframes)) + 2;
    int rc = SCAL_OK;
    auto A = [&](int r) { if (rc == SCAL_OK) rc = r; };
    A(c->stream.acquire(g.device, 0));
    scal_icp_config ic{};
    ic.max_corr_dist = g.max_corr_dist, ic.transformation_epsilon = g.transformation_epsilon, ic.fitness_epsilon = g.fitness_epsilon;
    ic.max_iterations = g.max_iterations;
    // the arena and the clouds ICP reads in front of the filter's buffers (the verifier's order): measured, queries are 0.4 % slower otherwise
    A(c->arena.alloc(static_cast<size_t>(g.max_points)));
    if (rc == SCAL_OK) rc = c->v.init(g.device, 0, c->work, n_xf, g.leaf, ic, ".R", "scal_reloc");
    A(c->d_desc.alloc(1200));
    if (rc == SCAL_OK) {
        scal_sc_config sc{};
        sc.max_radius = g.sc_max_radius, sc.dist_thres = g.sc_dist_thres, sc.max_keyframes = g.max_keyframes, sc.float_math = g.float_math;
        sc.device = g.device, sc.n_shards = 1;
        rc = sc_create(&sc, StreamLayout::Shared, &c->sc);  // lane 0: the stream of everything else in this context
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
    if (c->sc) scal_sc_destroy(c->sc);
    delete c;  // the verifier's ICP context with it
}

extern "C" int scal_reloc_size(scal_reloc_t* c) {
    if (!c) return SCAL_E_ARG;
    return c->size();
}

extern "C" scal_sc_t* scal_reloc_sc(scal_reloc_t* c) { return c ? c->sc : nullptr; }

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
        SCAL_HIP(hipMemcpyAsync(c->v.raw.p, xyzi, sizeof(float4) * static_cast<size_t>(n), hipMemcpyHostToDevice, s));
        SCAL_TRY(c->v.cf.load(s, reinterpret_cast<const float*>(c->v.raw.p), n));
        if ((m = c->v.filter(s, n, c->v.ds_src.p)) < 0) return m;  // downSizeFilterScancontext (:629-631)
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
        if (m == 0) SCAL_HIP(hipMemsetAsync(c->v.cf.d_n_out(), 0, sizeof(int), s));
        const SoA4 o = c->v.cf.out();
        SCAL_TRY(scal_sc_insert_cloud_device(c->sc, o.x, o.y, o.z, c->v.cf.d_n_out(), m));  // makeAndSaveScancontextAndKeys (:639)
    }
    if (m > 0) SCAL_HIP(hipMemcpyAsync(c->arena.p + c->off[j], c->v.ds_src.p, sizeof(float4) * static_cast<size_t>(m), hipMemcpyDeviceToDevice, s));
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
        GatherXf& e = c->v.h_xf.p[n_sel];
        e.src = c->off[j], e.dst = dst, e.copy = j == cand ? 1 : 0, e.pad = 0;
        reloc_relative(Pc, c->poses.data() + 12 * static_cast<size_t>(j), e.m);
        dst += c->off[j + 1] - c->off[j];
    }
    GatherXf& end = c->v.h_xf.p[n_sel];
    std::memset(&end, 0, sizeof end);
    end.dst = dst, end.copy = 1;
    const int n_tgt = c->v.gather_filter(c->stream, c->arena.p, n_sel, c->v.ds_tgt.p);  // downSizeFilterICP (:491-492)
    if (n_tgt < 0) return n_tgt;
    out->n_tgt = n_tgt;
    float G[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (!c->cfg.no_yaw_guess) {  // Rz(-yaw)
        const float cs = static_cast<float>(std::cos(static_cast<double>(out->sc.yaw_rad))), sn = static_cast<float>(std::sin(static_cast<double>(out->sc.yaw_rad)));
        G[0] = cs, G[1] = sn, G[4] = -sn, G[5] = cs;
    }
    SCAL_TRY(c->v.align(d_src, n_src, n_tgt, G, &out->icp));
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
        SCAL_HIP(hipMemcpyAsync(c->v.raw.p, xyzi, sizeof(float4) * static_cast<size_t>(n), hipMemcpyHostToDevice, s));
        SCAL_TRY(c->v.cf.load(s, reinterpret_cast<const float*>(c->v.raw.p), n));
        if ((*n_src = c->v.filter(s, n, d_src)) < 0) return *n_src;
    } else {  // no pinned word involved: nothing waits for this before the next query's filter writes its own count
        SCAL_HIP(hipMemsetAsync(c->v.cf.d_n_out(), 0, sizeof(int), s));
    }
    const SoA4 o = c->v.cf.out();
    return sc_make_cloud_device(c->sc, o.x, o.y, o.z, c->v.cf.d_n_out(), *n_src, d_desc);
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
    SCAL_TRY(reloc_front(c, xyzi, n, c->v.ds_src.p, c->d_desc.p, &n_src));
    SCAL_TRY(scal_sc_detect_between_device(c->sc, c->d_desc.p, 1, &out->sc));
    return reloc_verify(c, c->v.ds_src.p, n_src, out);
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
