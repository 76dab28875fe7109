// scal_pipeline's keyframe store and loop verification (sc_mode 3); the gather, filter and ICP of a verification are submap.hpp's
// SubmapVerifier, shared with scal_reloc.  See keyframes.hip.
#pragma once
#include "submap.hpp"
#include <array>
#include <vector>

namespace scal {

// getOdom (:312-323): x y z from t, roll pitch yaw from tf's getRPY of q, in double
void pose6_from(const double q_xyzw[4], const double t_xyz[3], double p6[6]);

struct KfLoopJob {  // one detected loop handed from stage D to the verification thread
    long long seq;
    int curr_kf, loop_kf;  // database indices
    float yaw_rad;
    double min_dist;
};

// one version of a keyframe's updated pose (keyframePosesUpdated, :408-431): made by the update call that ran while `stamp` scans had
// been pushed, so it holds for the loops of scans seq >= stamp
struct PoseVersion {
    long long stamp;
    std::array<double, 6> p;
};

// The pose-graph node's keyframeLaserClouds / keyframePoses (:629-637): an AoS xyzi arena of `max_points` records with the per-keyframe
// offsets on the device (off[j] .. off[j + 1] = the pipeline's keyframe j), the poses and the database index of every keyframe on the
// host.  Stage D appends (one thread), the verification thread reads: the host metadata is guarded by `mu`.
struct KeyframeStore {
    int device = 0, max_points = 0, max_keyframes = 0;
    DevBuf<float4> arena;
    DevBuf<int> d_off;       // [max_keyframes + 1], d_off[0] = 0; read by k_kf_append only (every other reader takes h_off)
    DevBuf<int> d_overflow;  // set by k_kf_append when a keyframe does not fit (nothing is written then)
    PinBuf<int> h_off;       // host mirror of d_off, copied behind every append
    PinBuf<int> h_overflow;
    Event ev_append;         // the newest append and its mirror copies on the ScanContext stream
    std::mutex mu;
    std::vector<int> db_of_own;                // database index of the pipeline's keyframe j
    std::vector<std::array<double, 6>> pose6;  // its Pose6D (getOdom)
    int checked = 0;                           // keyframes whose append has been confirmed on the host
    std::vector<std::vector<PoseVersion>> upd; // keyframe j's updated poses, oldest first (none: its gated pose holds)
    // verification (own stream, lane 5): the source's submap (one keyframe), then the target's, through one SubmapVerifier - its
    // filter, its single raw buffer and its two-entry gather table are free again behind each cloud's wait
    LaneStream vstream;
    SubmapVerifier v;
    // pose-graph map (pubMap, :810-834; pgo_map_max_points > 0): its own stream (lane 2, which scal_pipeline's layout leaves empty),
    // filter and buffers; one map at a time (map_mu)
    int map_cap = 0;
    std::mutex map_mu;
    LaneStream mstream;
    CloudFilter mcf;              // k_pgo_gather writes its input planes and count
    DevBuf<GatherXf> d_xf;        // one entry per selected keyframe (m: affine_f32 of its current pose, never `copy`) and the sentinel
    PinBuf<GatherXf> h_xf;
    DevBuf<unsigned> d_parts;     // per-workgroup bounding boxes of the gather, reduced by the filter's key kernel
    DevBuf<float4> d_map;         // the last map, xyzi
    long long map_n = -1;         // points of the last map, -1 before the first

    ~KeyframeStore();
    int init(int dev, int points, int keyframes, int map_points);
    bool keeps_clouds() const { return max_points > 0; }
    // stage D: insert the keyframe into ScanContext and (clouds kept) append its 0.4 m cloud behind the descriptor
    int insert(scal_sc_t* sc, scal_features_t* feat, int db_index, const double p6[6]);
    // stage D: wait for the newest append; SCAL_E_CAPACITY when the arena has overflowed
    int check();
    int own_count();
    int verify(const KfLoopJob& job, double fitness_thres, scal_pipeline_loop* out);
    int read(int db_index, double p6[6], float* xyzi, int cap, int* n);
    // a new version of n keyframes' poses, stamped `stamp`; versions older than the newest one with stamp <= floor (the smallest seq a
    // loop still to be verified can have) are dropped.  All or nothing.
    int update_poses(const int* db_index, const double* p6, int n, long long stamp, long long floor);
    int pgo_map(int kf_end, int skip, float leaf, float* out_xyzi, long long cap, long long* n_out);
    const float* pgo_map_device(long long* n);
    // scal_pipeline_optimize_keyframes: the own keyframes with database index < kf_end - database index, gated pose and current pose (the
    // latest update, else the gated one); SCAL_E_STATE by pgo_map's rule when kf_end is beyond the confirmed keyframes
    int pgo_snapshot(int kf_end, std::vector<int>* ids, std::vector<std::array<double, 6>>* gated, std::vector<std::array<double, 6>>* current);
    const std::array<double, 6>& pose_at(int j, long long seq) const;  // keyframe j's pose for the loop of scan seq; mu held
};

}  // namespace scal
