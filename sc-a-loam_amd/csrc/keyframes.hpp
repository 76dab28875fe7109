// scal_pipeline's keyframe store and loop verification (sc_mode 3).  See keyframes.hip.
#pragma once
#include "common.hpp"
#include "voxel_dev.hpp"
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

// The pose-graph node's keyframeLaserClouds / keyframePoses (:629-637): an AoS xyzi arena of `max_points` records with the per-keyframe
// offsets on the device (off[j] .. off[j + 1] = the pipeline's keyframe j), the poses and the database index of every keyframe on the
// host.  Stage D appends (one thread), the verification thread reads: the host metadata is guarded by `mu`.
struct KeyframeStore {
    int device = 0, max_points = 0, max_keyframes = 0;
    DevBuf<float4> arena;
    DevBuf<int> d_off;       // [max_keyframes + 1], d_off[0] = 0
    DevBuf<int> d_overflow;  // set by k_kf_append when a keyframe does not fit (nothing is written then)
    PinBuf<int> h_off;       // host mirror of d_off, copied behind every append
    PinBuf<int> h_overflow;
    Event ev_append;         // the newest append and its mirror copies on the ScanContext stream
    std::mutex mu;
    std::vector<int> db_of_own;                // database index of the pipeline's keyframe j
    std::vector<std::array<double, 6>> pose6;  // its Pose6D (getOdom)
    int checked = 0;                           // keyframes whose append has been confirmed on the host
    // verification (own stream, lane 5): submaps, their 0.4 m filter, ICP
    LaneStream vstream;
    VoxelFilter vf;
    DevBuf<float4> raw_src, raw_tgt, ds_src, ds_tgt;
    DevBuf<float> sx, sy, sz, sw, ox, oy, oz, ow;
    DevBuf<int> d_n;          // [0] submap size, [1] filtered size
    PinBuf<int> h_cnt;
    scal_icp_t* icp = nullptr;

    ~KeyframeStore();
    int init(int dev, int points, int keyframes);
    bool keeps_clouds() const { return max_points > 0; }
    // stage D: insert the keyframe into ScanContext and (clouds kept) append its 0.4 m cloud behind the descriptor
    int insert(scal_sc_t* sc, scal_features_t* feat, int db_index, const double p6[6]);
    // stage D: wait for the newest append; SCAL_E_CAPACITY when the arena has overflowed
    int check();
    int own_count();
    int verify(const KfLoopJob& job, double fitness_thres, scal_pipeline_loop* out);
    int read(int db_index, double p6[6], float* xyzi, int cap, int* n);
};

}  // namespace scal
