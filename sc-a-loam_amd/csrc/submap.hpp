// The reference's loop check (loopFindNearKeyframesCloud, doICPVirtualRelative: laserPosegraphOptimization.cpp:472-548) behind both of
// its users, scal_reloc and scal_pipeline's keyframe mode: they differ in their arenas and in the gather table they build.  submap.hip.
#pragma once
#include "common.hpp"
#include "voxel_dev.hpp"
#include "gather_dev.hpp"

namespace scal {

// the values laserPosegraphOptimization.cpp fixes for the check
constexpr double LOOP_ICP_MAX_CORR_DIST = 150.0;      // icp.setMaxCorrespondenceDistance(150), :519
constexpr int LOOP_ICP_MAX_ITERATIONS = 100;          // icp.setMaximumIterations(100), :520
constexpr double LOOP_ICP_TRANSFORMATION_EPS = 1e-6;  // icp.setTransformationEpsilon(1e-6), :521
constexpr double LOOP_ICP_FITNESS_EPS = 1e-6;         // icp.setEuclideanFitnessEpsilon(1e-6), :522
constexpr float LOOP_LEAF = 0.4f;                     // filter_size of downSizeFilterScancontext and downSizeFilterICP, :890-892
constexpr int LOOP_SUBMAP_HALF = 25;                  // historyKeyframeSearchNum, :500
constexpr double LOOP_FITNESS_THRES = 0.3;            // loopFitnessScoreThreshold, :531

// What a verification needs besides the caller's arena and stream.  No stream of its own: every call takes the caller's (reloc's lane
// 0, the pipeline's lane 5) and the ICP context sits on the lane init() is told.  filter() and gather_filter() end in CloudFilter::wait,
// which synchronises the stream: behind them `raw` and the pinned table are free again.  They return the number of centroids or an error.
struct SubmapVerifier {
    float leaf = 0.f;
    const char* who = "";  // prefix of the filter's capacity error
    CloudFilter cf;
    DevBuf<float4> raw, ds_src, ds_tgt;
    DevBuf<GatherXf> d_xf;
    PinBuf<GatherXf> h_xf;  // filled by the caller: n_sel entries and the sentinel
    scal_icp_t* icp = nullptr;

    ~SubmapVerifier() { scal_icp_destroy(icp); }  // the caller has synchronised its stream
    // table_entries counts the sentinel; ic: the distance, the epsilons and the iteration cap (sizes and device are filled in here)
    int init(int device, int lane, int capacity, int table_entries, float leaf_m, scal_icp_config ic, const char* tag, const char* who_);
    // VoxelGrid(leaf) of the n > 0 records already loaded into cf, exactly as scal_voxel_downsample_device runs it, into d_out
    int filter(hipStream_t s, int n, float4* d_out);
    // the submap of h_xf's table out of `arena` into raw, then its filter into d_out; an empty one launches nothing
    int gather_filter(hipStream_t s, const float4* arena, int n_sel, float4* d_out);
    // d_src against ds_tgt; a null guess is scal_icp_align_device's path, launch for launch
    int align(const float4* d_src, int n_src, int n_tgt, const float* guess16, scal_icp_result* out) {
        return scal_icp_align_guess_device(icp, reinterpret_cast<const float*>(d_src), n_src, reinterpret_cast<const float*>(ds_tgt.p), n_tgt, guess16, out);
    }
};

}  // namespace scal
