// The pose-graph node's keyframe path for scal_pipeline's sc_mode 3 (laserPosegraphOptimization.cpp):
//  - the keyframe gate (:598-617, getOdom :312-323, diffTransformation :325-336), host only;
//  - the keyframe store (keyframeLaserClouds / keyframePoses, :629-637): stage D appends each keyframe's 0.4 m cloud - the output of
//    ScanContext's keyframe filter, still in HBM - to an xyzi arena on the ScanContext stream (k_kf_append), nothing is read back;
//  - the loop verification (loopFindNearKeyframesCloud / doICPVirtualRelative, :472-548) on a stream of its own: the source and the
//    target submap are moved by the loop keyframe's pose (local2global, :338-359: a one-entry gather table each for the shared
//    SubmapVerifier of submap.hip), filtered at 0.4 m by the device voxel filter and aligned by the exact-NN ICP; the acceptance test
//    (:531) and the relative pose (:536-547) are computed on the host;
//  - the caller's optimized poses (updatePoses, :408-431 -> keyframePosesUpdated), versioned by the push counter so that each
//    verification sees the poses that held when its query scan was pushed;
//  - the pose-graph map (pubMap, :810-834) on a stream of its own: every skip-th keyframe moved by its current pose (k_pgo_gather: one
//    launch for all of them, straight into the voxel filter's SoA planes with the filter's bounding box), then the device voxel filter.
// The clouds never leave HBM.
#include "keyframes.hpp"
#include <algorithm>
#include <cmath>
#include <limits>

namespace scal {

// pubMap's local2global + concatenation (:815-822) of n_sel keyframes into map positions [0, n): position i lies in table entry s with
// xf[s].dst <= i < xf[s + 1].dst and is arena record xf[s].src + (i - xf[s].dst), moved by xf[s].m exactly as k_submap_gather moves it.
// A fixed grid (<= 256 workgroups: the filter's key kernel reduces one bounding box per workgroup in every workgroup) of contiguous
// chunks; each thread carries its table entry forward (positions only grow), so the table is searched once per workgroup.  Per point
// one 16-byte load (PGO_ITEMS of them in flight per thread) and four coalesced 4-byte stores into the planes the filter reads.
constexpr int PGO_ITEMS = 4, PGO_TILE = 256 * PGO_ITEMS, PGO_MAX_BLOCKS = 256;
static __global__ void __launch_bounds__(256) k_pgo_gather(const float4* __restrict__ arena, const GatherXf* __restrict__ xf, int n_sel, int n, int chunk,
                                                           float* __restrict__ ox, float* __restrict__ oy, float* __restrict__ oz,
                                                           float* __restrict__ ow, unsigned* __restrict__ parts, int* __restrict__ d_n) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *d_n = n;  // the filter's device-side count
    const int c0 = blockIdx.x * chunk, c1 = static_cast<int>(min(static_cast<long long>(n), static_cast<long long>(c0) + chunk));
    int s = gather_find(xf, n_sel, c0);
    int s_src = xf[s].src, s_dst = xf[s].dst, next = xf[s + 1].dst;
    int cur = -1;
    float T[12];
    unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    for (int t0 = c0; t0 < c1; t0 += PGO_TILE) {
        float4 p[PGO_ITEMS];
        int seg[PGO_ITEMS];
#pragma unroll
        for (int j = 0; j < PGO_ITEMS; ++j) {
            const int i = t0 + j * 256 + static_cast<int>(threadIdx.x);
            seg[j] = -1;
            if (i < c1) {
                while (i >= next) s_dst = next, s_src = xf[++s].src, next = xf[s + 1].dst;
                seg[j] = s;
                p[j] = arena[s_src + (i - s_dst)];
            }
        }
#pragma unroll
        for (int j = 0; j < PGO_ITEMS; ++j) {
            if (seg[j] < 0) continue;
            if (seg[j] != cur) {
                cur = seg[j];
                const float4* m = reinterpret_cast<const float4*>(xf[cur].m);
                const float4 a = m[0], b = m[1], c = m[2];
                T[0] = a.x, T[1] = a.y, T[2] = a.z, T[3] = a.w, T[4] = b.x, T[5] = b.y, T[6] = b.z, T[7] = b.w;
                T[8] = c.x, T[9] = c.y, T[10] = c.z, T[11] = c.w;
            }
            const float4 q = xf_point(T, p[j]);
            const int i = t0 + j * 256 + static_cast<int>(threadIdx.x);
            ox[i] = q.x, oy[i] = q.y, oz[i] = q.z, ow[i] = q.w;
            const unsigned u[3] = {vox_ordered(q.x), vox_ordered(q.y), vox_ordered(q.z)};
#pragma unroll
            for (int a = 0; a < 3; ++a) lo[a] = min(lo[a], u[a]), hi[a] = max(hi[a], u[a]);
        }
    }
    vox_bbox_block_store(parts, blockIdx.x, lo, hi);
}

namespace {

struct Aff34 {
    float m[12];  // row-major top 3x4 of pcl::getTransformation's Affine3f
};

// keyframe j's cloud (the keyframe filter's SoA output, *d_n points) -> arena[off[j] ..), off[j + 1] = off[j] + n.  A cloud that does
// not fit writes nothing, leaves off[j + 1] = off[j] and raises *overflow.  Grid-stride: 16-byte stores, coalesced reads of four planes.
__global__ void k_kf_append(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, const float* __restrict__ w,
                            const int* __restrict__ d_n, float4* __restrict__ arena, int* __restrict__ off, int j, int cap,
                            int* __restrict__ overflow) {
    const int n = *d_n, base = off[j];
    const bool fits = n >= 0 && n <= cap - base;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        off[j + 1] = fits ? base + n : base;
        if (!fits) *overflow = 1;
    }
    if (!fits) return;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) arena[base + i] = make_float4(x[i], y[i], z[i], w[i]);
}

// pcl::getTransformation (f32 Affine3f, R = Rz(yaw) Ry(pitch) Rx(roll)), as scaloam.pgo._affine_f32 states it: the sines and cosines
// in double rounded to f32, the products in f32
Aff34 affine_f32(const double p[6]) {
    const float A = static_cast<float>(std::cos(p[5])), B = static_cast<float>(std::sin(p[5]));
    const float C = static_cast<float>(std::cos(p[4])), D = static_cast<float>(std::sin(p[4]));
    const float E = static_cast<float>(std::cos(p[3])), F = static_cast<float>(std::sin(p[3]));
    const float DE = D * E, DF = D * F;
    Aff34 T;
    const float m[12] = {A * C, A * DF - B * E, B * F + A * DE, static_cast<float>(p[0]),
                         B * C, A * E + B * DF, B * DE - A * F, static_cast<float>(p[1]),
                         -D,    C * F,          C * E,          static_cast<float>(p[2])};
    std::memcpy(T.m, m, sizeof m);
    return T;
}

// tf::Matrix3x3(q).getRPY (:318-320), in double
void rpy_from_quat(const double q[4], double* roll, double* pitch, double* yaw) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double n = x * x + y * y + z * z + w * w, s = 2.0 / n;
    const double m00 = 1 - s * (y * y + z * z), m01 = s * (x * y - w * z), m02 = s * (x * z + w * y);
    const double m10 = s * (x * y + w * z);
    const double m20 = s * (x * z - w * y), m21 = s * (y * z + w * x), m22 = 1 - s * (x * x + y * y);
    if (std::fabs(m20) >= 1.0) {  // gimbal lock branch of tf's getEulerYPR
        *yaw = 0.0;
        if (m20 < 0)
            *pitch = M_PI / 2, *roll = std::atan2(m01, m02);
        else
            *pitch = -M_PI / 2, *roll = std::atan2(-m01, -m02);
        return;
    }
    *pitch = -std::asin(m20);
    const double cp = std::cos(*pitch);
    *roll = std::atan2(m21 / cp, m22 / cp);
    *yaw = std::atan2(m10 / cp, m00 / cp);
}

// Eigen::Quaterniond(const Matrix3d&) (gtsam Rot3::toQuaternion): x y z w
void quat_from_matrix(const double m[3][3], double q[4]) {
    const double t = m[0][0] + m[1][1] + m[2][2];
    if (t > 0) {
        double s = std::sqrt(t + 1.0);
        q[3] = 0.5 * s;
        s = 0.5 / s;
        q[0] = (m[2][1] - m[1][2]) * s, q[1] = (m[0][2] - m[2][0]) * s, q[2] = (m[1][0] - m[0][1]) * s;
        return;
    }
    int i = 0;
    if (m[1][1] > m[0][0]) i = 1;
    if (m[2][2] > m[i][i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    double s = std::sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0);
    q[i] = 0.5 * s;
    s = 0.5 / s;
    q[3] = (m[k][j] - m[j][k]) * s;
    q[j] = (m[j][i] + m[i][j]) * s;
    q[k] = (m[k][i] + m[i][k]) * s;
}

// doICPVirtualRelative's return value (:536-547): getTranslationAndEulerAngles of the f32 transform, poseFrom = (RzRyRx(roll, pitch,
// yaw), (x, y, z)), poseFrom.between(identity) = poseFrom^-1, in double
void relative_pose(const double T[16], double q[4], double t[3]) {
    const float x = static_cast<float>(T[3]), y = static_cast<float>(T[7]), z = static_cast<float>(T[11]);
    const float roll = std::atan2(static_cast<float>(T[9]), static_cast<float>(T[10]));
    const float pitch = std::asin(-static_cast<float>(T[8]));
    const float yaw = std::atan2(static_cast<float>(T[4]), static_cast<float>(T[0]));
    // gtsam Rot3::RzRyRx (Rot3M.cpp)
    const double cx = std::cos(double(roll)), sx = std::sin(double(roll)), cy = std::cos(double(pitch)), sy = std::sin(double(pitch));
    const double cz = std::cos(double(yaw)), sz = std::sin(double(yaw));
    const double ss_ = sx * sy, cs_ = cx * sy, sc_ = sx * cy, cc_ = cx * cy, c_s = cx * sz, s_s = sx * sz, _cs = cy * sz, _cc = cy * cz;
    const double s_c = sx * cz, c_c = cx * cz, ssc = ss_ * cz, csc = cs_ * cz, sss = ss_ * sz, css = cs_ * sz;
    const double R[3][3] = {{_cc, -c_s + ssc, s_s + csc}, {_cs, c_c + sss, -s_c + css}, {-sy, sc_, cc_}};
    double Rt[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Rt[r][c] = R[c][r];
    const double p[3] = {x, y, z};
    for (int r = 0; r < 3; ++r) t[r] = -((Rt[r][0] * p[0] + Rt[r][1] * p[1]) + Rt[r][2] * p[2]);
    quat_from_matrix(Rt, q);
}

}  // namespace

void pose6_from(const double q[4], const double t[3], double p6[6]) {
    p6[0] = t[0], p6[1] = t[1], p6[2] = t[2];
    rpy_from_quat(q, &p6[3], &p6[4], &p6[5]);
}

KeyframeStore::~KeyframeStore() {
    (void)hipSetDevice(device);
    if (vstream) (void)hipStreamSynchronize(vstream);
    if (mstream) (void)hipStreamSynchronize(mstream);
}

int KeyframeStore::init(int dev, int points, int keyframes, int map_points) {
    device = dev, max_points = points, max_keyframes = keyframes, map_cap = map_points;
    db_of_own.reserve(static_cast<size_t>(keyframes));
    pose6.reserve(static_cast<size_t>(keyframes));
    upd.reserve(static_cast<size_t>(keyframes));
    if (!keeps_clouds()) return SCAL_OK;
    SCAL_TRY(arena.alloc(static_cast<size_t>(points)));
    SCAL_TRY(d_off.alloc(static_cast<size_t>(keyframes) + 1));
    SCAL_TRY(d_overflow.alloc(1));
    SCAL_TRY(h_off.alloc(static_cast<size_t>(keyframes) + 1));
    SCAL_TRY(h_overflow.alloc(1));
    SCAL_TRY(ev_append.create(hipEventDisableTiming));
    h_off.p[0] = 0, h_overflow.p[0] = 0;
    // verification: lane 5 (scal_pipeline's busy chains are on lanes 0, 1, 3 and 4)
    SCAL_TRY(vstream.acquire(dev, 5));
    scal_icp_config ic{};
    ic.max_corr_dist = LOOP_ICP_MAX_CORR_DIST, ic.max_iterations = LOOP_ICP_MAX_ITERATIONS;
    ic.transformation_epsilon = LOOP_ICP_TRANSFORMATION_EPS, ic.fitness_epsilon = LOOP_ICP_FITNESS_EPS;
    SCAL_TRY(v.init(dev, 5, points, 2, LOOP_LEAF, ic, ".V", "scal_pipeline: loop verification"));
    SCAL_HIP(hipMemsetAsync(d_off.p, 0, sizeof(int), vstream));
    SCAL_HIP(hipMemsetAsync(d_overflow.p, 0, sizeof(int), vstream));
    SCAL_HIP(hipStreamSynchronize(vstream));
    if (map_cap == 0) return SCAL_OK;
    // pose-graph map: lane 2 - the pipeline's busy chains are on lanes 0, 1, 3 and 4, and on lane 5 the map would queue behind loop
    // verifications
    SCAL_TRY(mstream.acquire(dev, 2));
    SCAL_TRY(mcf.init(map_cap));
    mcf.set_tag(".M");
    SCAL_TRY(d_xf.alloc(static_cast<size_t>(keyframes) + 1));
    SCAL_TRY(h_xf.alloc(static_cast<size_t>(keyframes) + 1));
    SCAL_TRY(d_parts.alloc(6 * PGO_MAX_BLOCKS));
    SCAL_TRY(d_map.alloc(static_cast<size_t>(map_cap)));
    return SCAL_OK;
}

int KeyframeStore::own_count() {
    std::lock_guard<std::mutex> lk(mu);
    return static_cast<int>(db_of_own.size());
}

namespace {
struct AppendArgs {
    KeyframeStore* st;
    int j;
};
int append_hook(void* user, hipStream_t s, const ScFilterOut& ds) {
    auto* a = static_cast<AppendArgs*>(user);
    KeyframeStore* st = a->st;
    const int grid = std::max(1, std::min(div_up(ds.cap, 256), 256));
    hipLaunchKernelGGL(k_kf_append, dim3(grid), dim3(256), 0, s, ds.x, ds.y, ds.z, ds.w, ds.d_n, st->arena.p, st->d_off.p, a->j, st->max_points,
                       st->d_overflow.p);
    SCAL_HIP(hipGetLastError());
    SCAL_HIP(hipMemcpyAsync(st->h_off.p + a->j + 1, st->d_off.p + a->j + 1, sizeof(int), hipMemcpyDeviceToHost, s));
    SCAL_HIP(hipMemcpyAsync(st->h_overflow.p, st->d_overflow.p, sizeof(int), hipMemcpyDeviceToHost, s));
    SCAL_HIP(hipEventRecord(st->ev_append, s));
    return SCAL_OK;
}
}  // namespace

int KeyframeStore::insert(scal_sc_t* sc, scal_features_t* feat, int db_index, const double p6[6]) {
    int j;
    {
        std::lock_guard<std::mutex> lk(mu);
        j = static_cast<int>(db_of_own.size());
    }
    if (j >= max_keyframes) {
        set_error("scal_pipeline: more than %d keyframes (sc_max_keyframes)", max_keyframes);
        return SCAL_E_CAPACITY;
    }
    if (keeps_clouds()) {
        AppendArgs a{this, j};
        SCAL_TRY(sc_insert_features_then(sc, feat, append_hook, &a));
    } else {
        SCAL_TRY(scal_sc_insert_features(sc, feat));
    }
    std::lock_guard<std::mutex> lk(mu);
    db_of_own.push_back(db_index);
    pose6.push_back({p6[0], p6[1], p6[2], p6[3], p6[4], p6[5]});
    upd.emplace_back();
    return SCAL_OK;
}

int KeyframeStore::check() {
    if (!keeps_clouds()) return SCAL_OK;
    const int n = own_count();  // only stage D's thread inserts and checks
    if (checked == n) return SCAL_OK;
    SCAL_HIP(hipSetDevice(device));
    SCAL_HIP(hipEventSynchronize(ev_append));
    if (h_overflow.p[0]) {
        set_error("scal_pipeline: the keyframe cloud store is full (kf_max_points = %d, keyframe %d does not fit)", max_points, n - 1);
        return SCAL_E_CAPACITY;
    }
    std::lock_guard<std::mutex> lk(mu);
    checked = n;
    return SCAL_OK;
}

int KeyframeStore::verify(const KfLoopJob& job, double fitness_thres, scal_pipeline_loop* out) {
    std::memset(out, 0, sizeof *out);
    out->seq = job.seq, out->curr_kf = job.curr_kf, out->loop_kf = job.loop_kf, out->yaw_rad = job.yaw_rad, out->min_dist = job.min_dist;
    out->verified = -1;
    out->fitness = std::numeric_limits<double>::max();
    for (int k = 0; k < 16; ++k) out->T[k] = (k % 5 == 0) ? 1.0 : 0.0;
    out->q_rel[3] = 1.0;
    int jc, jl, j0, j1;
    Aff34 T;
    {
        std::lock_guard<std::mutex> lk(mu);
        if (!keeps_clouds()) return SCAL_OK;
        auto own = [&](int db) {
            auto it = std::lower_bound(db_of_own.begin(), db_of_own.end(), db);
            return (it != db_of_own.end() && *it == db) ? static_cast<int>(it - db_of_own.begin()) : -1;
        };
        jc = own(job.curr_kf), jl = own(job.loop_kf);
        if (jc < 0 || jl < 0 || jc >= checked) return SCAL_OK;
        // loopFindNearKeyframesCloud(target, loop, 25, loop): keyframes loop-25 .. loop+25 that have a cloud, in keyframe order
        const int submap = LOOP_SUBMAP_HALF;
        j0 = static_cast<int>(std::lower_bound(db_of_own.begin(), db_of_own.end(), job.loop_kf - submap) - db_of_own.begin());
        j1 = static_cast<int>(std::upper_bound(db_of_own.begin(), db_of_own.end(), job.loop_kf + submap) - db_of_own.begin()) - 1;
        j1 = std::min(j1, checked - 1);
        // every keyframe is moved by the ROOT (loop) keyframe's pose (:506-507): keyframePosesUpdated's, as it was when scan seq was pushed
        T = affine_f32(pose_at(jl, job.seq).data());
    }
    SCAL_HIP(hipSetDevice(device));
    hipStream_t s = vstream;
    SCAL_HIP(hipStreamWaitEvent(s, ev_append, 0));  // behind the current keyframe's append (and every earlier one)
    // the source [jc, jc], then the target [j0, j1]: a one-entry table with T and the sentinel over an arena range whose offsets the
    // host has confirmed (jc < checked, j1 <= checked - 1); downSizeFilterICP (:491-492) behind the gather
    float4* ds[2] = {v.ds_src.p, v.ds_tgt.p};
    const int a[2] = {h_off.p[jc], h_off.p[j0]}, b[2] = {h_off.p[jc + 1], h_off.p[j1 + 1]};
    int n_ds[2];
    for (int c = 0; c < 2; ++c) {
        GatherXf* t = v.h_xf.p;  // free again: the source's run has waited
        std::memset(t, 0, 2 * sizeof *t);
        std::memcpy(t[0].m, T.m, sizeof T.m);
        t[0].src = a[c], t[1].dst = b[c] - a[c];
        if ((n_ds[c] = v.gather_filter(s, arena.p, 1, ds[c])) < 0) return n_ds[c];
    }
    out->n_src = n_ds[0], out->n_tgt = n_ds[1];
    scal_icp_result r;
    SCAL_TRY(v.align(v.ds_src.p, n_ds[0], n_ds[1], nullptr, &r));
    out->converged = r.converged, out->iterations = r.iterations, out->state = r.state, out->fitness = r.fitness;
    std::memcpy(out->T, r.T, sizeof out->T);
    out->verified = (r.converged && r.fitness <= fitness_thres) ? 1 : 0;  // :531
    relative_pose(r.T, out->q_rel, out->t_rel);
    return SCAL_OK;
}

const std::array<double, 6>& KeyframeStore::pose_at(int j, long long seq) const {
    const std::vector<PoseVersion>& v = upd[static_cast<size_t>(j)];
    for (size_t k = v.size(); k-- > 0;)
        if (v[k].stamp <= seq) return v[k].p;
    return pose6[static_cast<size_t>(j)];  // keyframePosesUpdated starts as keyframePoses (:636)
}

int KeyframeStore::update_poses(const int* db_index, const double* p6, int n, long long stamp, long long floor) {
    std::lock_guard<std::mutex> lk(mu);
    std::vector<int> js(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) {
        auto it = std::lower_bound(db_of_own.begin(), db_of_own.end(), db_index[i]);
        if (it == db_of_own.end() || *it != db_index[i]) {
            set_error("scal_pipeline_update_keyframe_poses: %d is not a keyframe of this pipeline", db_index[i]);
            return SCAL_E_ARG;
        }
        for (int k = 0; k < 6; ++k)
            if (!std::isfinite(p6[6 * i + k])) {
                set_error("scal_pipeline_update_keyframe_poses: the pose of keyframe %d is not finite", db_index[i]);
                return SCAL_E_ARG;
            }
        js[static_cast<size_t>(i)] = static_cast<int>(it - db_of_own.begin());
    }
    for (int i = 0; i < n; ++i) {
        std::vector<PoseVersion>& v = upd[static_cast<size_t>(js[static_cast<size_t>(i)])];
        size_t keep = 0;  // the newest version that a loop of seq >= floor can still pick, and everything after it
        while (keep + 1 < v.size() && v[keep + 1].stamp <= floor) ++keep;
        v.erase(v.begin(), v.begin() + static_cast<std::ptrdiff_t>(keep));
        std::array<double, 6> q;
        std::memcpy(q.data(), p6 + 6 * i, sizeof(double) * 6);
        if (!v.empty() && v.back().stamp == stamp)
            v.back().p = q;  // no scan was pushed since the last update: the later one wins
        else
            v.push_back(PoseVersion{stamp, q});
    }
    return SCAL_OK;
}

int KeyframeStore::pgo_map(int kf_end, int skip, float leaf, float* out_xyzi, long long cap, long long* n_out) {
    std::lock_guard<std::mutex> map_lk(map_mu);
    *n_out = 0;
    int n_sel = 0;
    long long n = 0;
    {
        std::lock_guard<std::mutex> lk(mu);
        // only keyframes whose append stage D has confirmed (check() synchronised on it): kf_end must not reach past them
        const int end_ok = checked > 0 ? db_of_own[static_cast<size_t>(checked - 1)] + 1 : 0;
        if (kf_end > end_ok) {
            set_error("scal_pipeline_pgo_map: kf_end %d is beyond the confirmed keyframes (%d)", kf_end, end_ok);
            return SCAL_E_STATE;
        }
        const int j_end = static_cast<int>(std::lower_bound(db_of_own.begin(), db_of_own.end(), kf_end) - db_of_own.begin());
        for (int j = 0; j < j_end; j += skip) n += h_off.p[j + 1] - h_off.p[j];
        if (n > map_cap) {
            *n_out = n;
            set_error("scal_pipeline_pgo_map: the map needs %lld points, pgo_map_max_points is %d", n, map_cap);
            return SCAL_E_CAPACITY;
        }
        int dst = 0;
        for (int j = 0; j < j_end; j += skip, ++n_sel) {  // updatePoses' result as it stands now (:815-822 under mKF)
            GatherXf& e = h_xf.p[n_sel];
            const std::vector<PoseVersion>& v = upd[static_cast<size_t>(j)];
            const Aff34 T = affine_f32(v.empty() ? pose6[static_cast<size_t>(j)].data() : v.back().p.data());
            std::memcpy(e.m, T.m, sizeof e.m);
            e.src = h_off.p[j], e.dst = dst, e.copy = 0, e.pad = 0;
            dst += h_off.p[j + 1] - h_off.p[j];
        }
        h_xf.p[n_sel].src = 0, h_xf.p[n_sel].dst = dst;
    }
    SCAL_HIP(hipSetDevice(device));
    hipStream_t s = mstream;
    if (n == 0) {
        map_n = 0;
        return SCAL_OK;
    }
    // No event against stage D's appends: the gather reads only the arena ranges of confirmed keyframes, whose appends the host has
    // already synchronised on (check()), and later appends write behind them.  The verification stream only reads the arena too.
    const int ni = static_cast<int>(n);
    SCAL_HIP(hipMemcpyAsync(d_xf.p, h_xf.p, sizeof(GatherXf) * (static_cast<size_t>(n_sel) + 1), hipMemcpyHostToDevice, s));
    int grid = std::min(PGO_MAX_BLOCKS, div_up(ni, PGO_TILE));
    const int chunk = div_up(div_up(ni, grid), PGO_TILE) * PGO_TILE;
    grid = div_up(ni, chunk);  // every workgroup has points
    const SoA4 in = mcf.in();
    SCAL_LAUNCH_PROF("k_pgo_gather", k_pgo_gather, dim3(grid), dim3(256), 0, s, arena.p, d_xf.p, n_sel, ni, chunk, in.x, in.y, in.z, in.w, d_parts.p,
                     mcf.d_n_in());
    SCAL_HIP(hipGetLastError());
    SCAL_TRY(mcf.filter(s, ni, leaf, d_parts.p, grid));
    mcf.store(s, ni, reinterpret_cast<float*>(d_map.p));
    const int m_all = mcf.wait(s, "scal_pipeline_pgo_map");
    map_n = m_all < 0 ? -1 : m_all;
    if (m_all < 0) return m_all;
    *n_out = map_n;
    const long long m = std::min(map_n, cap);
    if (m > 0) {  // on the map's stream: a copy on the null stream would wait for the pipeline's lanes
        SCAL_HIP(hipMemcpyAsync(out_xyzi, d_map.p, sizeof(float4) * static_cast<size_t>(m), hipMemcpyDeviceToHost, s));
        SCAL_HIP(hipStreamSynchronize(s));
    }
    return SCAL_OK;
}

int KeyframeStore::pgo_snapshot(int kf_end, std::vector<int>* ids, std::vector<std::array<double, 6>>* gated, std::vector<std::array<double, 6>>* current) {
    std::lock_guard<std::mutex> lk(mu);
    // a store without clouds has no appends to confirm: its keyframes count once stage D has inserted them
    const int conf = keeps_clouds() ? checked : static_cast<int>(db_of_own.size());
    const int end_ok = conf > 0 ? db_of_own[static_cast<size_t>(conf - 1)] + 1 : 0;
    if (kf_end > end_ok) {
        set_error("scal_pipeline_optimize_keyframes: kf_end %d is beyond the confirmed keyframes (%d)", kf_end, end_ok);
        return SCAL_E_STATE;
    }
    const size_t j_end = static_cast<size_t>(std::lower_bound(db_of_own.begin(), db_of_own.end(), kf_end) - db_of_own.begin());
    ids->assign(db_of_own.begin(), db_of_own.begin() + static_cast<std::ptrdiff_t>(j_end));
    gated->assign(pose6.begin(), pose6.begin() + static_cast<std::ptrdiff_t>(j_end));
    current->resize(j_end);
    for (size_t j = 0; j < j_end; ++j) (*current)[j] = upd[j].empty() ? pose6[j] : upd[j].back().p;
    return SCAL_OK;
}

const float* KeyframeStore::pgo_map_device(long long* n) {
    std::lock_guard<std::mutex> lk(map_mu);
    *n = map_n < 0 ? 0 : map_n;
    return map_n < 0 ? nullptr : reinterpret_cast<const float*>(d_map.p);
}

int KeyframeStore::read(int db_index, double p6[6], float* xyzi, int cap, int* n) {
    int j, a = 0, b = 0;
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = std::lower_bound(db_of_own.begin(), db_of_own.end(), db_index);
        if (it == db_of_own.end() || *it != db_index) {
            set_error("scal_pipeline_keyframe: %d is not a keyframe of this pipeline", db_index);
            return SCAL_E_ARG;
        }
        j = static_cast<int>(it - db_of_own.begin());
        for (int k = 0; k < 6; ++k) p6[k] = pose6[static_cast<size_t>(j)][static_cast<size_t>(k)];
        if (keeps_clouds() && j < checked) a = h_off.p[j], b = h_off.p[j + 1];
    }
    *n = b - a;
    const int m = std::min(b - a, cap);
    if (m > 0) {
        SCAL_HIP(hipSetDevice(device));
        SCAL_HIP(hipMemcpy(xyzi, arena.p + a, sizeof(float4) * static_cast<size_t>(m), hipMemcpyDeviceToHost));
    }
    return SCAL_OK;
}

}  // namespace scal

using namespace scal;

// ------------------------------------------------------------------------------------------------ the keyframe gate (host only)
extern "C" int scal_keyframe_gate_init(scal_keyframe_gate_state* st, double meter_gap, double deg_gap) {
    if (!st || !std::isfinite(meter_gap) || !std::isfinite(deg_gap) || meter_gap < 0 || deg_gap < 0) {
        set_error("scal_keyframe_gate_init: bad argument");
        return SCAL_E_ARG;
    }
    std::memset(st, 0, sizeof *st);
    st->meter_gap = meter_gap;
    st->rad_gap = deg_gap * (M_PI / 180.0);  // :875-876
    st->translation_accumulated = 1000000.0, st->rotation_accumulated = 1000000.0;  // :67-68
    return SCAL_OK;
}

extern "C" int scal_keyframe_gate(scal_keyframe_gate_state* st, const double q[4], const double t[3], int* is_keyframe) {
    if (!st || !q || !t || !is_keyframe) {
        set_error("scal_keyframe_gate: null argument");
        return SCAL_E_ARG;
    }
    const double nq = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    if (!(nq > 0) || !std::isfinite(nq) || !std::isfinite(t[0]) || !std::isfinite(t[1]) || !std::isfinite(t[2])) {
        set_error("scal_keyframe_gate: the pose must be finite with a non-zero quaternion");
        return SCAL_E_ARG;
    }
    double cur[6];
    pose6_from(q, t, cur);
    // diffTransformation (:325-336): SE3_p1^-1 * SE3_p2 in f32 (the inverse of a rigid transform), then getTranslationAndEulerAngles
    const Aff34 A = affine_f32(st->curr), B = affine_f32(cur);
    float Ri[3][3], ti[3], D[3][4];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Ri[r][c] = A.m[4 * c + r];
    for (int r = 0; r < 3; ++r) ti[r] = -((Ri[r][0] * A.m[3] + Ri[r][1] * A.m[7]) + Ri[r][2] * A.m[11]);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) D[r][c] = (Ri[r][0] * B.m[c] + Ri[r][1] * B.m[4 + c]) + Ri[r][2] * B.m[8 + c] + (c == 3 ? ti[r] : 0.0f);
    const double dx = std::fabs(double(D[0][3])), dy = std::fabs(double(D[1][3])), dz = std::fabs(double(D[2][3]));
    const double droll = std::fabs(double(std::atan2(D[2][1], D[2][2]))), dpitch = std::fabs(double(std::asin(-D[2][0])));
    const double dyaw = std::fabs(double(std::atan2(D[1][0], D[0][0])));
    std::memcpy(st->curr, cur, sizeof cur);
    st->translation_accumulated += std::sqrt(dx * dx + dy * dy + dz * dz);
    st->rotation_accumulated += droll + dpitch + dyaw;  // "sum just naive approach"
    *is_keyframe = 0;
    if (st->translation_accumulated > st->meter_gap || st->rotation_accumulated > st->rad_gap) {
        *is_keyframe = 1;
        st->translation_accumulated = 0.0, st->rotation_accumulated = 0.0;
    }
    return SCAL_OK;
}
