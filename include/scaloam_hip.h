/*
 * scaloam_hip.h — C-ABI of libscaloam_hip.so: the MI355X (gfx950) implementation of SC-A-LOAM's
 * data-parallel hot path.  The reference (swoonge/SC-A-LOAM) has no plugin/FFI interface: its stages
 * are welded into ROS node main()s.  Each entry point below is therefore a *call-site cut*: it replaces
 * the cited lines of the reference, and INTEGRATION.md shows the few lines a maintainer changes in each
 * node to call it.  Plain C: opaque handles, raw pointers and sizes, int status codes; nothing throws
 * or aborts across this boundary.
 *
 * Conventions
 *  - Every context owns one HIP stream, its device buffers and pinned staging.  All arrays passed in or
 *    out are caller-owned and only need to stay valid for the duration of the call.  `_device` variants
 *    take pointers into GPU memory of the context's device instead of host memory.
 *  - Points are `PointXYZI` as the reference uses them (include/aloam_velodyne/common.h:43):
 *    4 packed floats x,y,z,intensity (16 B) on the host side.  On the device everything is SoA.
 *  - A context is single-caller (like the reference's node threads) except the ScanContext context,
 *    which serialises insert/detect internally (the reference calls them from two threads with no
 *    common lock: laserPosegraphOptimization.cpp:633-642 vs :718).
 *  - Status: 0 ok, <0 SCAL_E_*; scal_last_error() gives a message for the calling thread.
 */
#ifndef SCALOAM_HIP_H
#define SCALOAM_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ status */
enum {
    SCAL_OK = 0,
    SCAL_E_ARG = -1,          /* bad argument */
    SCAL_E_LIDAR_TYPE = -2,   /* unknown lidar_type (reference: ROS_BREAK, scanRegistration.cpp:214-218) */
    SCAL_E_SCAN_LINE = -3,    /* scan_line not 16/32/64 (reference exits, scanRegistration.cpp:486-490) */
    SCAL_E_TOO_MANY = -4,     /* more points than max_points (reference scratch is 400000, scanRegistration.cpp:68-71) */
    SCAL_E_EMPTY = -5,        /* no point survives the NaN / range filters (reference would read points[0]) */
    SCAL_E_HIP = -6,          /* HIP runtime error */
    SCAL_E_NO_DEVICE = -7,    /* no gfx950 device / code object missing: the product never falls back to a CPU path */
    SCAL_E_CAPACITY = -8,     /* a device-side capacity was exceeded (segment longer than the LDS sort, map pool full) */
    SCAL_E_STATE = -9         /* call order violated (e.g. fetch before run) */
};
const char* scal_last_error(void);
/* number of visible HIP devices, -1 if the runtime cannot initialise */
int scal_device_count(void);
const char* scal_version(void);
/* 0 (default): the stages of a scan share one in-order stream per device (plus the optional side streams).  1: every stage
 * context created afterwards gets its own stream, so that consecutive scans overlap the way the reference's four ROS nodes do
 * (A of scan k+1 during C of scan k ...); hand-overs between contexts are ordered by events.  Four streams carry the work (A + stage
 * C's gather and corner filter; B + ScanContext's descriptor and search; C; one side stream for stage C's surf filter and
 * ScanContext's keyframe filter), split so that the four chains are about equally long.  Use two or more features contexts
 * alternately in that mode: a context's outputs are rewritten by its next run, which waits for all their readers. */
int scal_set_stream_mode(int mode);
/* Optional per-kernel timing (HIP events on the launching stream), used by bench.py's roofline leg.
 * No counterpart in the reference: its TicToc phase timers print nothing. */
int scal_prof_enable(int on);
int scal_prof_filter(const char* kernel_name); /* time only this kernel (NULL/"" = all instrumented kernels) */
int scal_prof_reset(void);
int scal_prof_read(const char* kernel_name, double* total_ms, long* count);
int scal_prof_names(char* buf, int cap);
/* development aid: while on (together with scal_prof_enable), every timed dispatch is also kept as (kernel, start ms, stop ms)
 * relative to one base event; scal_prof_timeline_dump writes them as CSV and clears the list */
int scal_prof_timeline(int on);
int scal_prof_timeline_dump(const char* path);

/* ------------------------------------------------------------------ ordering against the caller's own streams
 * Every `_device` entry point reads (and writes) the caller's device memory on the CONTEXT'S stream, which is not ordered against
 * any stream of the caller: device inputs must be complete before the call, unless the caller orders the context's stream behind
 * its producer itself.  These accessors return that stream (a hipStream_t) for exactly that: hipStreamWaitEvent(ctx_stream, ev)
 * in front of the call, hipEventRecord(ev, ctx_stream) behind it (torch: torch.cuda.ExternalStream(ptr).wait_stream(...)).
 * Typical producer: an RCCL collective on the caller's stream (sharded map filter, sharded ScanContext exchange). */
typedef struct scal_features scal_features_t;
typedef struct scal_voxel scal_voxel_t;
typedef struct scal_sc scal_sc_t;
typedef struct scal_map scal_map_t;
typedef struct scal_odom scal_odom_t;
void* scal_features_stream(scal_features_t* ctx);
void* scal_voxel_stream(scal_voxel_t* ctx);
void* scal_sc_stream(scal_sc_t* ctx); /* the stream of descriptors, keys, database and searches (in stream mode 1 the keyframe filter of
                                       * the *_features entry points runs on a second, internal stream that this one waits for) */
void* scal_map_stream(scal_map_t* ctx);
void* scal_odom_stream(scal_odom_t* ctx);

/* ------------------------------------------------------------------ stage A: feature extraction
 * Replaces laserCloudHandler, src/scanRegistration.cpp:134-421 (NaN/range filter, ring id + relative
 * time, ring-major reorder, curvature, per-(ring,sixth) sort + greedy sharp/lessSharp/flat picks,
 * lessFlat + per-ring 0.2 m voxel grid).  The five output clouds are what the node publishes at :426-454. */
enum { SCAL_VLP16 = 0, SCAL_HDL32 = 1, SCAL_HDL64 = 2, SCAL_OS1_64 = 3 };

typedef struct {
    int lidar_type;        /* SCAL_*  (rosparam lidar_type, scanRegistration.cpp:481) */
    int n_scans;           /* rosparam scan_line (:480) */
    double minimum_range;  /* rosparam minimum_range (:482) */
    int max_points;        /* capacity; <= 400000 */
    int float_math;        /* 0: atan/sqrt of :168 promote to double (the pinned GCC 5 toolchain); 1: float overloads */
    int check_finite;      /* 1: drop non-finite points (pcl::removeNaNFromPointCloud on a non-dense cloud, :138) */
    int device;            /* HIP device ordinal */
} scal_features_config;

typedef struct {
    /* caller-owned host arrays; capacities in points unless noted; NULL = not wanted */
    float* cloud;      /* [max_points][4] ordered cloud, intensity = scanID + 0.1*relTime (/velodyne_cloud_2) */
    int* src_index;    /* [max_points] input index of every ordered point */
    float* curvature;  /* [max_points] cloudCurvature */
    int* label;        /* [max_points] cloudLabel */
    int* ring_start;   /* [n_scans] scanStartInd */
    int* ring_end;     /* [n_scans] scanEndInd */
    int* sharp;        /* [2*6*n_scans]  indices into `cloud`, reference emission order */
    int* less_sharp;   /* [20*6*n_scans] */
    int* flat;         /* [4*6*n_scans] */
    float* less_flat;  /* [max_points][4] downsampled lessFlat cloud */
    /* filled by the call */
    int n_kept, n_sharp, n_less_sharp, n_flat, n_less_flat;
    int n_tied_segments; /* segments whose sort met equal curvatures (std::sort order is unspecified there) */
} scal_features_out;

int scal_features_create(const scal_features_config* cfg, scal_features_t** ctx);
void scal_features_destroy(scal_features_t* ctx);
/* host input: xyz at xyz + i*stride_bytes (PointCloud2 layout). Synchronous. */
int scal_features_run(scal_features_t* ctx, const void* xyz, int n, int stride_bytes, scal_features_out* out);
/* host input, asynchronous: the scan is copied into pinned staging (the caller's buffer is free on return), uploaded and
 * processed on the context's stream; results stay on the GPU as with scal_features_run_device (the PointCloud2 callback of
 * scanRegistration.cpp:116 when the later stages consume the device-resident results) */
int scal_features_enqueue_host(scal_features_t* ctx, const void* xyz, int n, int stride_bytes);
/* device input (float*, stride in floats), asynchronous on the context's stream; results stay on the GPU
 * for scal_odom_step_features / scal_map_step_features / scal_sc_insert_features. */
int scal_features_run_device(scal_features_t* ctx, const float* d_xyz, int n, int stride_floats);
/* wait for the last run and copy results to the host */
int scal_features_fetch(scal_features_t* ctx, scal_features_out* out);
int scal_features_sync(scal_features_t* ctx);

/* ------------------------------------------------------------------ voxel grid
 * Replaces pcl::VoxelGrid<PointXYZI>::filter at scanRegistration.cpp:414-418,
 * laserMapping.cpp:543-551, :793-801 and laserPosegraphOptimization.cpp:629-631. */
int scal_voxel_create(int max_points, int device, scal_voxel_t** ctx);
void scal_voxel_destroy(scal_voxel_t* ctx);
int scal_voxel_downsample(scal_voxel_t* ctx, const float* xyzi, int n, float leaf, float* out_xyzi, int* n_out);
/* the same with the cloud and the output (room for n records; may not overlap the input) in device memory, e.g. between
 * scal_mapmerge_device_points and scal_icp_align_device: loopFindNearKeyframesCloud's VoxelGrid, :491-492; waits, *n_out on the host.
 * The input must be complete (or scal_voxel_stream ordered behind its producer) before the call. */
int scal_voxel_downsample_device(scal_voxel_t* ctx, const float* d_xyzi, int n, float leaf, float* d_out_xyzi, int* n_out);

/* ------------------------------------------------------------------ stage D: ScanContext
 * Replaces SCManager (include/scancontext/Scancontext.h:57-123, Scancontext.cpp), call sites
 * laserPosegraphOptimization.cpp:639 (insert) and :718 (detect). */
typedef struct {
    double max_radius;  /* PC_MAX_RADIUS, setMaximumRadius (Scancontext.cpp:267-270) */
    double dist_thres;  /* SC_DIST_THRES, setSCdistThres (:262-265) */
    int max_keyframes;  /* database capacity on this device */
    int float_math;     /* atan overload at Scancontext.cpp:26-35, as in scal_features_config */
    int device;
    /* sharding (multi-GPU): this context stores keyframes i with i % n_shards == shard; 1/0 = everything */
    int n_shards, shard;
    /* n > 0: run this context on the device's side stream n (1..5) so that insert/detect overlap with stages B and C of the
     * same scan; ordering against the features context (scal_sc_insert_features / scal_sc_make_features) is kept with events.
     * Two contexts on different lanes do not queue behind each other (descriptor builder: 1, sharded database: 5). */
    int side_stream;
} scal_sc_config;

typedef struct {
    int loop_id;      /* -1: no loop (Scancontext.cpp:338, :406-408) */
    float yaw_rad;    /* deg2rad(shift * 6 deg) (:422) */
    double min_dist;  /* best SC distance among the candidates */
    int nn_idx;       /* its keyframe index */
    int nn_shift;     /* its column shift */
    int cand_idx[3];  /* ring-key KNN candidates, ascending key distance */
    float cand_keydist[3];
    double cand_scdist[3];
    int cand_shift[3];
} scal_sc_result;

int scal_sc_create(const scal_sc_config* cfg, scal_sc_t** ctx);
void scal_sc_destroy(scal_sc_t* ctx);
int scal_sc_size(scal_sc_t* ctx);
/* makeAndSaveScancontextAndKeys(cloud) — cloud already downsampled by the caller as the reference does */
int scal_sc_insert_cloud(scal_sc_t* ctx, const float* xyzi, int n);
int scal_sc_insert_cloud_device(scal_sc_t* ctx, const float* d_x, const float* d_y, const float* d_z, const int* d_n, int n_max);
/* saveScancontextAndKeys(desc): 20x60 doubles, column-major */
int scal_sc_insert_descriptor(scal_sc_t* ctx, const double* desc_colmajor);
int scal_sc_get_descriptor(scal_sc_t* ctx, int idx, double* desc_colmajor, float* ringkey20);
/* keyframe cloud of a features context on the same device (its ordered full-resolution cloud, which is what
 * /velodyne_cloud_registered_local carries) -> VoxelGrid 0.4 m (laserPosegraphOptimization.cpp:629-631, :890-891)
 * -> makeAndSaveScancontextAndKeys (:639), nothing leaves the GPU. */
int scal_sc_insert_features(scal_sc_t* ctx, scal_features_t* feat);
/* same front end but the 20x60 descriptor is only written to d_desc (device memory, 1200 doubles, column-major)
 * and NOT inserted: the sharded search exchanges descriptors first. */
int scal_sc_make_features(scal_sc_t* ctx, scal_features_t* feat, double* d_desc);
/* the same without waiting: d_desc is valid after scal_sc_sync, or after scal_sc_wait_descriptor, which waits for the oldest
 * queued descriptor only (up to four may be in flight) */
int scal_sc_make_features_enqueue(scal_sc_t* ctx, scal_features_t* feat, double* d_desc);
int scal_sc_wait_descriptor(scal_sc_t* ctx);
int scal_sc_insert_descriptor_device(scal_sc_t* ctx, const double* d_desc_colmajor);
/* n (<= 64) device-resident descriptors in global order - the ranks' descriptors of one step after the all-gather - in one
 * launch and without a host synchronisation; every shard keeps the ones it owns */
int scal_sc_insert_descriptors_device(scal_sc_t* ctx, const double* d_descs_colmajor, int n);
/* waits for everything queued on the context's stream (before a collective on another stream reads its device outputs) */
int scal_sc_sync(scal_sc_t* ctx);
/* makeScancontext only (no insert) */
int scal_sc_make_descriptor(scal_sc_t* ctx, const float* xyzi, int n, double* desc_colmajor);
/* detectLoopClosureID(): query = newest keyframe; reproduces the >=31 gate, the 30-query tree period,
 * the exclusion of the newest 30 keys and the 3-candidate / 7-shift search (Scancontext.cpp:336-427). */
int scal_sc_detect(scal_sc_t* ctx, scal_sc_result* res);
/* the same in two halves: enqueue launches the search for the newest keyframe and returns, collect waits for the oldest search
 * not yet collected (its own event: nothing queued on the stream behind it is waited for).  scal_sc_detect = enqueue + collect.
 * Up to four searches may be in flight, each for the keyframe that was newest when it was enqueued. */
int scal_sc_detect_enqueue(scal_sc_t* ctx);
int scal_sc_detect_collect(scal_sc_t* ctx, scal_sc_result* res);
/* distanceBtnScanContext for descriptor pairs already in the database */
int scal_sc_distance_pairs(scal_sc_t* ctx, const int* idx_a, const int* idx_b, int n_pairs, double* dist, int* shift);
/* dense block of the pair grid (SURVEY.md 8d "D dense"; distDirectSC Scancontext.cpp:83-110 over every pair): queries [q0,q1) x
 * database [d0,d1), row-major [q][d].  mode 0 = the reference's 7-shift search around the sector-key alignment
 * (distanceBtnScanContext :113-148); 1 = exhaustive 60 shifts, column sums in the reference's order on the vector ALUs;
 * 2 = exhaustive 60 shifts on the matrix cores (v_mfma_f64_16x16x4_f64 over unit columns: same minimum and shift, distances
 * equal to mode 1 within a few ulp - the summation order differs); 3 = the same product on v_mfma_f32_16x16x4_f32 with the
 * unit columns rounded to f32 (twice the rate; distances within 2e-6 of mode 2 - inside the 1e-5 the path is held to - and the
 * shift can differ where two shifts are closer than that).  Unsharded contexts only. */
int scal_sc_distance_matrix(scal_sc_t* ctx, int q0, int q1, int d0, int d1, int mode, double* dist, int* shift);
/* the same with DEVICE outputs (nq*nd doubles / ints), enqueued on the context's stream: scal_sc_sync() before reading them */
int scal_sc_distance_matrix_device(scal_sc_t* ctx, int q0, int q1, int d0, int d1, int mode, double* d_dist, int* d_shift);
/* Batch loop search over a stored session (offline loop mining; the exhaustive counterpart of detectLoopClosureID's ring-key
 * prefilter + 7-shift search, Scancontext.cpp:336-427): for every query keyframe q in [q0, q1) the k (<= 16) smallest distances
 * among the keyframes d < q - exclude_recent (NUM_EXCLUDE_RECENT = 30, Scancontext.h:92), from the dense distance block of `mode`
 * (2 = all 60 shifts on the f64 matrix cores) with the top-k taken on the device.  Outputs [q1 - q0][k]: keyframe index (-1 =
 * fewer than k eligible), distance, column shift; ascending distance, ties to the lower index.  Unsharded contexts only. */
int scal_sc_batch_loop_search(scal_sc_t* ctx, int q0, int q1, int exclude_recent, int k, int mode, int* idx, double* dist, int* shift);
/* sharded search pieces (one context per GPU): local top-3 for the newest GLOBAL key, then a merge of the
 * gathered per-shard records (the all-gather itself is the caller's: RCCL via torch.distributed). */
typedef struct {
    float key_dist;
    int idx; /* global keyframe index, -1 = empty */
    double sc_dist;
    int shift;
    int pad;
} scal_sc_cand;
int scal_sc_shard_query(scal_sc_t* ctx, const double* query_desc_colmajor, int global_size_at_rebuild, scal_sc_cand out[3]);
/* batched form on device pointers: d_queries [nq][1200] doubles, d_out [nq][3] records; synchronous */
int scal_sc_shard_query_device(scal_sc_t* ctx, const double* d_queries, int nq, int global_size_at_rebuild, scal_sc_cand* d_out);
/* the same for a batch of nq (<= 64) queries, query q searched against the tree of size limits[q] (host array); three launches,
 * the 3 * nq records stay in device memory (d_out) and nothing is synchronised: follow with scal_sc_sync */
int scal_sc_shard_query_batch_device(scal_sc_t* ctx, const double* d_queries, int nq, const int* limits, scal_sc_cand* d_out);
int scal_sc_merge_candidates(const scal_sc_cand* gathered, int n_records, double dist_thres, scal_sc_result* res);
/* detectLoopClosureIDBetweenSession (Scancontext.cpp:272-333) for nq query descriptors (20x60 doubles, column-major, back to back)
 * that are NOT in the database: ring key of the query, KNN(3) over ALL keys of the database - no exclusion of recent keys, no >= 31
 * gate, no tree period -, distanceBtnScanContext(query, candidate) for the three, strict minimum, loop_id = nn_idx iff min_dist <
 * dist_thres, yaw_rad = deg2rad(shift * 6) as f32.  A database of one or two entries behaves as nanoflann does: unfilled KNN slots
 * keep index 0.  Queries run in chunks of 64, one launch set per chunk; a record depends neither on nq nor on the chunking.
 * Deviation: the reference builds its batch tree once, at the first call (is_tree_batch_made), and keeps searching that; this call
 * searches the database as it is at the call - the same whenever nothing was inserted in between.
 * SCAL_E_STATE: empty database.  SCAL_E_ARG: sharded context, NULL pointers, nq < 0. */
int scal_sc_detect_between(scal_sc_t* db, const double* query_descs_colmajor /* host [nq][1200] */, int nq, scal_sc_result* res /* [nq] */);
/* the same with the descriptors in device memory (complete before the call, or scal_sc_stream ordered behind their producer) */
int scal_sc_detect_between_device(scal_sc_t* db, const double* d_query_descs, int nq, scal_sc_result* res);
/* scal_sc_distance_matrix with the query rows taken from entries [q0, q1) of ANOTHER context on the same device (`queries` may also
 * be `db` itself): row-major [q][d] over database entries [d0, d1), modes 0-3 as above, bit-identical to the block a single context
 * holding both sets of descriptors would give.  The work is queued on db's stream behind everything queued on queries' stream
 * (an event); the call waits for it.  SCAL_E_ARG: a sharded context, different devices, a range outside either context. */
int scal_sc_cross_matrix(scal_sc_t* db, scal_sc_t* queries, int q0, int q1, int d0, int d1, int mode, double* dist, int* shift);
/* scal_sc_batch_loop_search with the query rows from another context: for every query entry q in [q0, q1) of `queries` the k (<= 16)
 * smallest distances over ALL entries of db (no entry is "too recent" for a query from another session).  Outputs [q1 - q0][k]:
 * database index (-1 = fewer than k entries), distance, column shift; ascending distance, ties to the lower index. */
int scal_sc_cross_search(scal_sc_t* db, scal_sc_t* queries, int q0, int q1, int k, int mode, int* idx, double* dist, int* shift);

/* ------------------------------------------------------------------ stage C: scan-to-map
 * Replaces process(), src/laserMapping.cpp:310-802 and :845-849. */
typedef struct {
    float line_res, plane_res; /* rosparams mapping_line_resolution / mapping_plane_resolution (:915-916) */
    int max_scan_points;       /* capacity of one full-resolution scan */
    int max_map_points;        /* capacity of the rolling 21x21x11 cube window, per feature class */
    int device;
} scal_map_config;

typedef struct {
    int n_corner_stack, n_surf_stack, n_corner_map, n_surf_map;
    int n_edge[2], n_plane[2];      /* residual blocks per outer iteration (:563) */
    int lm_iters[2], lm_success[2]; /* LM iterations / accepted steps per outer iteration */
    double cost_init[2], cost_final[2];
    int solved;                     /* 0: map too small (:555, :731-734), pose = prior */
    int n_map_corner_total, n_map_surf_total;
    int insert_path;                /* how :738-802 ran: 0 = full sort of the map pool, 1 = merge of the scan's points into the sorted map */
} scal_map_stats;

int scal_map_create(const scal_map_config* cfg, scal_map_t** ctx);
void scal_map_destroy(scal_map_t* ctx);
/* one process() pass.  corner_last / surf_last / full_res: PointXYZI host arrays (full_res may be NULL).
 * q_wodom (x,y,z,w), t_wodom: /laser_odom_to_init pose.  Outputs: q_w_curr, t_w_curr (/aft_mapped_to_init),
 * registered (full_res transformed, :845-849; may be NULL). */
int scal_map_step(scal_map_t* ctx, const float* corner_last, int n_corner, const float* surf_last, int n_surf,
                  const float* full_res, int n_full, const double* q_wodom, const double* t_wodom, double* q_w_curr,
                  double* t_w_curr, float* registered, scal_map_stats* stats);
/* same, inputs taken from a features context on the same device (lessSharp / lessFlat / ordered cloud) */
int scal_map_step_features(scal_map_t* ctx, scal_features_t* feat, const double* q_wodom, const double* t_wodom,
                           double* q_w_curr, double* t_w_curr, scal_map_stats* stats);
/* Optional: start the pose-independent part of the next scal_map_step_features(ctx, feat, ...) - input gather and the stack
 * downsample (:543-551) - on the device's side stream, so that it overlaps with stage B.  Returns immediately.  Up to three
 * prefetches may be queued ahead of their steps (rotating input sets); steps consume them in order.  `feat` must not be run again
 * before its step has been enqueued: the step would mix the prefetched inputs of one scan with the full-resolution cloud of the
 * next; the step entry points check the features context's run counter and return SCAL_E_STATE in that case. */
int scal_map_prefetch_features(scal_map_t* ctx, scal_features_t* feat);
/* The same in two halves, for a host that issues them from different threads (scal_pipeline does): begin queues the input gather and
 * the corner stack filter on the features context's stream, right behind stage A; finish queues the surf stack filter on the side
 * stream.  Halves are finished in the order they were begun; a step consumes its prefetch once both halves have been queued. */
int scal_map_prefetch_begin(scal_map_t* ctx, scal_features_t* feat);
int scal_map_prefetch_finish(scal_map_t* ctx, scal_features_t* feat);
/* scal_map_step_features in two halves.  enqueue queues the whole pass; collect returns the oldest uncollected pose as soon as it
 * is on the host, while the map insertion (:738-802) and the registration (:845-849) still run behind it.  Up to four steps may
 * be queued before the first is collected: transformAssociateToMap / transformUpdate (:143-153), the rolling-window decision
 * (:313-508) and the map sizes live on the device, so a step is queued right behind the previous one with nothing read back.
 * Such a step is speculative: it assumes the cube window of the previous step and the merge insert; when that does not hold the
 * device stops the chain, and collect / finish redo the step on the general path (window shift, full-sort insertion) and replay
 * the steps queued behind it - results are identical either way.  A features context handed to enqueue must not be run again
 * before its step has been collected; once the pose is collected it may be, even when the step's insertion is still to be redone
 * (that redo reads only what the step copied out of the context).  scal_map_export and scal_map_finish wait for all queued insertions (and report a
 * capacity error of an insertion).  The map sizes in the statistics of collect are those before this scan's insertion,
 * insert_path is -1. */
int scal_map_enqueue_features(scal_map_t* ctx, scal_features_t* feat, const double* q_wodom, const double* t_wodom);
int scal_map_collect(scal_map_t* ctx, double* q_w_curr, double* t_w_curr, scal_map_stats* stats);
int scal_map_finish(scal_map_t* ctx);
/* current map points of the 5x5x3 window (laserCloudCornerFromMap / SurfFromMap content); returns count */
int scal_map_export(scal_map_t* ctx, int which /*0 corner, 1 surf*/, float* out_xyzi, int cap);
/* every point of the 21x21x11 cube grid, one feature class: the content of /laser_cloud_map (laserMapping.cpp:824-837 adds the corner
 * and surf clouds of all 4,851 cubes every 20 frames); out_xyzi NULL or cap 0: only the count.  Returns the number of points written. */
int scal_map_export_all(scal_map_t* ctx, int which /*0 corner, 1 surf*/, float* out_xyzi, int cap);
int scal_map_get_wmap_wodom(scal_map_t* ctx, double* q_xyzw, double* t);
/* enable (default) / disable the merge insert; both give identical maps, the switch exists for tests and measurements */
int scal_map_set_merge_insert(scal_map_t* ctx, int enable);
/* how the steps ran so far: out4 = {queued speculatively, run on the general path, redone from the start after a stopped chain
 * (window moved), insertion redone with the full sort after a stopped chain}; for tests and measurements */
int scal_map_get_path_counters(scal_map_t* ctx, int* out4);
/* test hook: poll budget of the LM solve's partial-sum exchange between its workgroups (default 2^22).  With 0 every solve of this library's stage C gives up at
 * its first exchange: collect / step return SCAL_E_HIP ("LM solve abandoned"), the pose of that step is its prior, and the context
 * must keep working afterwards.  Exercises the bounded-wait path that would otherwise need a machine hogged by another process. */
int scal_map_debug_set_lm_polls(scal_map_t* ctx, int polls);
/* test hook: entries per 1 m cell of the one-launch neighbour-grid build of the queued steps (default: the number of filter voxels
 * that can intersect a cell - 27 corner / 8 surf at the reference's 0.4 / 0.8 m; values above that are clamped).  A cell that
 * receives more points stops the queued chain, and the step is redone with the general three-launch build: with 1 / 1 every
 * queued step takes that route (path counter 3 counts them) and the poses must not change. */
int scal_map_debug_set_grid_cap(scal_map_t* ctx, int cap_corner, int cap_surf);
/* 1 (default): every enqueue first looks (without waiting) whether queued steps have finished or stopped; 0: a stopped chain is
 * only noticed by collect / finish, so that steps really get queued behind it (test switch for the replay path) */
int scal_map_set_poll(scal_map_t* ctx, int enable);

/* ---- Ceres-adapter mode of stage C: the host keeps ceres::Problem / ceres::Solve exactly as
 * laserMapping.cpp:563-728 builds them; the device does what surrounds the solve and evaluates the residual blocks in batches.
 *   scal_map_adapter_begin   :310-560  transformAssociateToMap, window shift, submap (cell grids), stack downsample; returns the prior pose
 *   per outer iteration (:563):
 *     scal_map_associate     :578-688  kNN + PCA / plane fit at the caller's current pose -> residual blocks, in the order the reference adds
 *                                      them (corner stack points, then surf stack points); n_residuals = 3 per edge block + 1 per plane block
 *     scal_map_get_blocks              the blocks as records (to construct the reference's own LidarEdgeFactor / LidarPlaneNormFactor objects), or
 *     scal_map_eval_blocks             residuals [n_residuals] and ambient Jacobians [n_residuals][7] (qx qy qz qw tx ty tz, row-major) of all
 *                                      blocks at x7, without loss function or local parameterisation (Ceres applies its HuberLoss(0.1) and
 *                                      EigenQuaternionParameterization itself): what a ceres::EvaluationCallback + thin per-block CostFunction serves from
 *   scal_map_adapter_finish  :735-802, :845-849  transformUpdate with the solved pose, map insertion + re-filter, registration
 * kind: 0 LidarEdgeFactor(curr_point = cp, last_point_a = pa, last_point_b = pb, s = 1), 2 LidarPlaneNormFactor(curr_point = cp,
 * plane_unit_norm = pa, negative_OA_dot_norm = pb[0]); (1 = LidarPlaneFactor(cp, j = pa, unit normal = pb) in the odometry's blocks). */
typedef struct {
    int kind, pad;
    double cp[3], pa[3], pb[3];
} scal_block;
int scal_map_adapter_begin(scal_map_t* ctx, const float* corner_last, int n_corner, const float* surf_last, int n_surf, const float* full_res,
                           int n_full, const double* q_wodom, const double* t_wodom, double* q_w_curr, double* t_w_curr);
int scal_map_associate(scal_map_t* ctx, const double* q_w_curr, const double* t_w_curr, int* n_blocks, int* n_residuals);
int scal_map_get_blocks(scal_map_t* ctx, scal_block* out, int cap); /* returns the number of records written */
int scal_map_eval_blocks(scal_map_t* ctx, const double* x7, int want_jac, double* residuals, double* jacobians);
int scal_map_adapter_finish(scal_map_t* ctx, const double* q_w_curr, const double* t_w_curr, float* registered, scal_map_stats* stats);

/* ------------------------------------------------------------------ stage B: scan-to-scan odometry
 * Replaces the main loop body of src/laserOdometry.cpp:267-291, :299-506, :554-568. */
typedef struct {
    int max_points; /* capacity of the lessFlat cloud */
    int device;
} scal_odom_config;
typedef struct {
    int n_edge[2], n_plane[2];
    int lm_iters[2], lm_success[2];
    double cost_init[2], cost_final[2];
} scal_odom_stats;
int scal_odom_create(const scal_odom_config* cfg, scal_odom_t** ctx);
void scal_odom_destroy(scal_odom_t* ctx);
int scal_odom_step(scal_odom_t* ctx, const float* sharp, int n_sharp, const float* less_sharp, int n_less_sharp,
                   const float* flat, int n_flat, const float* less_flat, int n_less_flat, double* q_last_curr,
                   double* t_last_curr, double* q_w_curr, double* t_w_curr, scal_odom_stats* stats);
int scal_odom_step_features(scal_odom_t* ctx, scal_features_t* feat, double* q_last_curr, double* t_last_curr,
                            double* q_w_curr, double* t_w_curr, scal_odom_stats* stats);
/* the same in two halves (= enqueue + collect): the caller can queue other work while the step runs.  Up to four steps may be
 * queued before the first is collected (a step only needs its predecessor's device state: the last clouds and the pose increment
 * of :97-101); collect returns them in order and integrates the pose (:504-505) on the host. */
int scal_odom_enqueue_features(scal_odom_t* ctx, scal_features_t* feat);
int scal_odom_collect(scal_odom_t* ctx, double* q_last_curr, double* t_last_curr, double* q_w_curr, double* t_w_curr,
                      scal_odom_stats* stats);

/* Ceres-adapter mode of stage B (laserOdometry.cpp:278-501 with the host's own ceres::Problem / ceres::Solve), the counterpart of
 * scal_map_adapter_*: begin uploads the four clouds and returns the initial guess (para_q / para_t persist across scans, :97-101)
 * and whether this frame is solved at all (the first one is not, :267-271); per outer iteration scal_odom_associate runs the
 * correspondence search of :299-483 at the solver's current increment, scal_odom_get_blocks / scal_odom_eval_blocks are as for
 * stage C (kind 0 LidarEdgeFactor, kind 1 LidarPlaneFactor given as (j, unit normal)); finish integrates the pose (:504-505) and
 * hands the clouds over (:554-568). */
int scal_odom_adapter_begin(scal_odom_t* ctx, const float* sharp, int n_sharp, const float* less_sharp, int n_less_sharp, const float* flat,
                            int n_flat, const float* less_flat, int n_less_flat, double* q_last_curr, double* t_last_curr, int* need_solve);
int scal_odom_associate(scal_odom_t* ctx, const double* q_last_curr, const double* t_last_curr, int* n_blocks, int* n_residuals);
int scal_odom_get_blocks(scal_odom_t* ctx, scal_block* out, int cap);
int scal_odom_eval_blocks(scal_odom_t* ctx, const double* x7, int want_jac, double* residuals, double* jacobians);
int scal_odom_adapter_finish(scal_odom_t* ctx, const double* q_last_curr, const double* t_last_curr, double* q_w_curr, double* t_w_curr);

/* ------------------------------------------------------------------ offline dense map merge
 * Replaces the loop body of utils/python/makeMergedMap.py:83-133: keyframe cloud x SE(3) pose -> global frame (f64), removal of
 * points whose LOCAL range is <= near_thres (:109-116, 2 m in the script), concatenation in keyframe order, f32 xyzi out
 * (:145-147).  In-process analogues: local2global (laserPosegraphOptimization.cpp:338-359), transformPointCloud (:446-470). */
typedef struct {
    long long max_points;  /* capacity of the merged map */
    int max_frame_points;  /* largest keyframe given to scal_mapmerge_add */
    int device;
} scal_mapmerge_config;
typedef struct scal_mapmerge scal_mapmerge_t;
int scal_mapmerge_create(const scal_mapmerge_config* cfg, scal_mapmerge_t** ctx);
void scal_mapmerge_destroy(scal_mapmerge_t* ctx);
int scal_mapmerge_reset(scal_mapmerge_t* ctx);
/* one keyframe: xyzi host records, pose12 = one line of optimized_poses.txt (row-major top 3x4 of the SE(3) matrix, :48-56) */
int scal_mapmerge_add(scal_mapmerge_t* ctx, const float* xyzi, int n, const double* pose12, double near_thres);
/* n_frames keyframes already in device memory, back to back: frame f = records [offsets[f], offsets[f+1]) (host arrays) */
int scal_mapmerge_add_batch_device(scal_mapmerge_t* ctx, const float* d_xyzi, const int* offsets, const double* poses12,
                                   int n_frames, double near_thres);
long long scal_mapmerge_size(scal_mapmerge_t* ctx);                                 /* points merged so far (waits), <0 = error */
int scal_mapmerge_download(scal_mapmerge_t* ctx, float* out_xyzi, long long cap_points);
/* pubMap's VoxelGrid over the merged map (laserPosegraphOptimization.cpp:810-834, leaf = mapviz_filter_size): *n_out centroids
 * in PCL order, the first cap_points of them written to out_xyzi (host).  The merged map itself is kept. */
int scal_mapmerge_downsample(scal_mapmerge_t* ctx, float leaf, float* out_xyzi, long long cap_points, long long* n_out);
const float* scal_mapmerge_device_points(scal_mapmerge_t* ctx);                     /* the merged xyzi records in device memory */

/* ------------------------------------------------------------------ loop-closure verification ICP
 * Replaces the pcl::IterativeClosestPoint call of doICPVirtualRelative, laserPosegraphOptimization.cpp:518-535.  The caller
 * builds the two clouds as the reference does (:504-507: keyframes moved by one root pose, VoxelGrid 0.4) with scal_mapmerge_*
 * and scal_voxel_*, and applies the acceptance test of :532 (converged && fitness <= 0.3) to the result. */
typedef struct {
    double max_corr_dist;           /* setMaxCorrespondenceDistance, 150 (:520) */
    double transformation_epsilon;  /* setTransformationEpsilon, 1e-6 (:522) */
    double fitness_epsilon;         /* setEuclideanFitnessEpsilon, 1e-6 (:523) */
    int max_iterations;             /* setMaximumIterations, 100 (:521) */
    int max_source, max_target;     /* capacities */
    int device;
} scal_icp_config;
typedef struct {
    int converged;          /* icp.hasConverged() */
    int iterations;
    int state;              /* 1 iteration cap, 2 transformation epsilon, 3 absolute MSE, 4 relative MSE, 5 too few correspondences */
    int n_correspondences;  /* of the last iteration */
    double fitness;         /* icp.getFitnessScore() */
    double T[16];           /* icp.getFinalTransformation(), row-major, f32 values */
} scal_icp_result;
typedef struct scal_icp scal_icp_t;
int scal_icp_create(const scal_icp_config* cfg, scal_icp_t** ctx);
void scal_icp_destroy(scal_icp_t* ctx);
/* icp.setInputSource(src); icp.setInputTarget(tgt); icp.align(): xyzi host records */
int scal_icp_align(scal_icp_t* ctx, const float* src_xyzi, int n_src, const float* tgt_xyzi, int n_tgt, scal_icp_result* res);
/* the same with both clouds already in HBM (16-byte xyzi records, e.g. scal_mapmerge_device_points / a device voxel output): the
 * source is copied into the context, the target is read in place and must stay valid until the call returns */
int scal_icp_align_device(scal_icp_t* ctx, const float* d_src_xyzi, int n_src, const float* d_tgt_xyzi, int n_tgt, scal_icp_result* res);
/* nearest-neighbour search: 1 (default) = cell grid over the target, exact, with the dense sweep for queries it cannot settle;
 * 0 = dense sweep only.  Both stand in for pcl::KdTreeFLANN::nearestKSearch(k=1) (pcl/registration/impl/icp.hpp) and give the
 * same correspondences, lowest target index on equal distances. */
int scal_icp_set_search(scal_icp_t* ctx, int mode);
/* icp.align(output, guess): pcl::Registration::align with an initial transformation (row-major 4x4, f32).  The working copy of the
 * source is moved once by the guess (the f32 arithmetic of every later increment) and the accumulated transformation starts at the
 * guess instead of the identity; iteration, convergence criteria and states are those of scal_icp_align.  T is the whole
 * transformation, guess included, and fitness is that of the ORIGINAL source moved by T.  guess == NULL or the identity matrix is
 * scal_icp_align launch for launch, with identical results.  SCAL_E_ARG: a guess that is not finite or whose last row is not
 * 0 0 0 1 (the context stays usable). */
int scal_icp_align_guess(scal_icp_t* ctx, const float* src_xyzi, int n_src, const float* tgt_xyzi, int n_tgt, const float guess[16],
                         scal_icp_result* res);
int scal_icp_align_guess_device(scal_icp_t* ctx, const float* d_src_xyzi, int n_src, const float* d_tgt_xyzi, int n_tgt, const float guess[16],
                                scal_icp_result* res);

/* ---- point-to-plane alignment on a scal_icp_t (an extension: the reference has no counterpart).
 * The target carries one normal per point, tgt_nc [n_tgt][4] f32 in exactly the layout scal_nbr_normals* writes: normal, then
 * curvature.  The curvature is ignored; the normal is used as stored, never re-normalised.  scal_icp_config, the search modes of
 * scal_icp_set_search and the guess (its rules and error codes those of scal_icp_align_guess, NULL or the identity: none) are
 * shared with the point-to-point calls, which are not changed by these.  The CPU restatement is scaloam/icp_plane.py; the device is
 * held to it bit for bit, so THE ORDER OF THE OPERATIONS BELOW IS PART OF THE INTERFACE.
 *
 * Correspondences are exactly those of scal_icp_align: the nearest target point by the f32 key (d, index) - d the f32 squared
 * distance dx dx + dy dy + dz dz summed left to right, the lowest index among equal d - within the cap `!(d > max2)`,
 * max2 = (float)(max_corr_dist^2); a source or target point that is not finite takes no part.  A correspondence whose target normal
 * has a component that is not finite (the NaN rows scal_nbr_normals writes for sparse neighbourhoods) is dropped: it still counts
 * for `fitness` and for nothing else.
 *
 * One row per remaining correspondence, everything f64 promoted from the f32 values, one rounding per operation (no FMA).  p the
 * moved source point, q the target point, n its normal:
 *     c0 = p.y n.z - p.z n.y,  c1 = p.z n.x - p.x n.z,  c2 = p.x n.y - p.y n.x          (c = p x n)
 *     a  = (c0, c1, c2, n.x, n.y, n.z)
 *     r  = ((q.x - p.x) n.x + (q.y - p.y) n.y) + (q.z - p.z) n.z
 * and the sweep minimises sum (a.x - r)^2 over x = (alpha, beta, gamma, tx, ty, tz).
 *
 * 32 sums per sweep (SCAL_ICP_PLANE_NSUM):
 *     [0]       number of rows (within the cap, finite normal)
 *     [1..21]   sum a_i a_j, i <= j, row-major: (0,0) (0,1) .. (0,5) (1,1) .. (5,5)
 *     [22..27]  sum a_i r
 *     [28]      sum r r
 *     [29]      sum d over the rows (d the f32 squared distance)
 *     [30]      number of source points with any nearest neighbour (no cap, no normal test)
 *     [31]      sum d over those
 * Source point i is lane i % 64 of wave (i / 64) % 4 of workgroup i / 256; a point without a term adds +0.  Every sum is reduced in
 * the order of the point-to-point sums: the 64 lanes of a wave by the xor butterfly v += v[lane ^ o] for o = 32, 16, 8, 4, 2, 1;
 * the four waves as ((r0 + r1) + r2) + r3; the workgroups sequentially, in workgroup order, from +0.
 *
 * Host step on the sums.  Fewer than 6 rows ([0] < 6): state 5, no increment.  Otherwise the 6x6 system A x = b (A from [1..21],
 * b from [22..27]) is solved by LDL^T without pivoting, in this order:
 *     for j = 0 .. 5:
 *         v_k = L_jk D_k                                       for k < j
 *         d   = A_jj;  d = d - L_jk v_k                        for k = 0 .. j-1 ascending
 *         degenerate unless  d > SCAL_ICP_PLANE_PIVOT_MIN A_jj
 *         D_j = d
 *         s = A_ij;  s = s - L_ik v_k  (k ascending);  L_ij = s / d        for i = j+1 .. 5
 *     y_i = b_i;  y_i = y_i - L_ik y_k  (k = 0 .. i-1 ascending)           for i = 0 .. 5
 *     z_i = y_i / D_i
 *     x_i = z_i;  x_i = x_i - L_ki x_k  (k = i+1 .. 5 ascending)           for i = 5 .. 0
 * A degenerate system (one plane, two planes, a line: the data do not fix all six freedoms) is state 6: not converged, no
 * increment, T keeps what has accumulated.  SCAL_ICP_PLANE_PIVOT_MIN is a setting, not a measurement: exactly singular systems
 * show pivot ratios d / A_jj of 0, -1.6e-16 or an A_jj of 0, three orthogonal planes 0.25, a pair of thinned street keyframes 0.87.
 *
 * The increment, without trigonometric functions: h = (alpha / 2, beta / 2, gamma / 2), m = sqrt(((1 + hx hx) + hy hy) + hz hz),
 * the unit quaternion (w, x, y, z) = (1 / m, hx / m, hy / m, hz / m), the rotation
 *     1 - 2 (y y + z z)    2 (x y - z w)        2 (x z + y w)
 *     2 (x y + z w)        1 - 2 (x x + z z)    2 (y z - x w)
 *     2 (x z - y w)        2 (y z + x w)        1 - 2 (x x + y y)
 * and the translation (tx, ty, tz), all stored as f32.  It is applied to the working cloud and taken up as F = T F in the f32
 * arithmetic of scal_icp_align, and the convergence criteria and states 1 - 4 are scal_icp_align's with mse = [29] / [0].
 *
 * The final sweep moves the ORIGINAL source by the final T and sums with the same cap: fitness = [31] / [30] (uncapped, the value
 * scal_icp_result::fitness has for this T, so the reference's 0.3 gate stays comparable), plane_fitness = [28] / [0],
 * normal_eq = [1..27].  first_eq = [1..27] of the first sweep (the source as given, or moved by the guess). */
#define SCAL_ICP_PLANE_NSUM 32
#define SCAL_ICP_PLANE_PIVOT_MIN 1e-10
typedef struct {
    int converged, iterations, state, n_correspondences; /* as scal_icp_result; n_correspondences counts rows; state 6: degenerate normal equations */
    double fitness;       /* as scal_icp_result: uncapped mean d of the ORIGINAL source moved by T; DBL_MAX without a neighbour */
    double plane_fitness; /* mean r^2 over the final sweep's rows; DBL_MAX without one */
    double T[16];         /* row-major, f32 values, guess included */
    double normal_eq[27]; /* upper triangle of A^T A (21, row-major) and A^T b (6) of the FINAL sweep: the 6x6 information of the alignment */
    double first_eq[27];  /* the same of the FIRST sweep */
} scal_icp_plane_result;
/* xyzi host records and host normals.  Empty clouds: state 5, T the identity.  SCAL_E_ARG / SCAL_E_TOO_MANY as scal_icp_align for
 * the same arguments (tgt_nc == NULL with n_tgt > 0 is SCAL_E_ARG); the context stays usable.  The first plane call on a context
 * allocates what only these calls need (normals staging, 32-wide partials, pinned sums); they are released with the context. */
int scal_icp_align_plane(scal_icp_t* ctx, const float* src_xyzi, int n_src, const float* tgt_xyzi, const float* tgt_nc, int n_tgt,
                         const float guess[16], scal_icp_plane_result* res);
/* all three arrays already in HBM; target and normals are read in place and must stay valid until the call returns */
int scal_icp_align_plane_device(scal_icp_t* ctx, const float* d_src_xyzi, int n_src, const float* d_tgt_xyzi, const float* d_tgt_nc, int n_tgt,
                                const float guess[16], scal_icp_plane_result* res);

/* ------------------------------------------------------------------ multiview refine (BASELINE.json config #5, "global ICP refine")
 * An extension: the reference has no counterpart.  All K keyframes of a session are aligned at once, in Jacobi rounds.  One round:
 *  1. every frame f is moved by its pose with the map merge's arithmetic and near-range rule (the bits of a one-frame
 *     scal_mapmerge_add + download); the union of the moved frames, in frame order, is the round's fixed target;
 *  2. every non-fixed frame is aligned by point-to-point ICP - iteration, increment, convergence criteria and states exactly those
 *     of scal_icp_align - against the points of ALL OTHER frames: a point's own frame is never a candidate (a frame matched
 *     against a target that contains itself does not move);
 *  3. fitness = sum d^2 / n over the correspondences within max_corr_dist of a last sweep of the source moved by the final T.
 *     This deviates on purpose from scal_icp_result::fitness, which is PCL's uncapped getFitnessScore(): an uncapped score needs an
 *     exact neighbour for every far point that no other keyframe saw - at the scale of a session a dense sweep of millions of
 *     queries.  Where every point has a neighbour within max_corr_dist the two are the same number;
 *  4. frame f is accepted iff converged and fitness <= fitness_gate (the reference's loop test, :532, 0.3 there): pose <- T * pose
 *     in f64 (T's f32 values promoted; ((T[r][0] P[0][c] + T[r][1] P[1][c]) + T[r][2] P[2][c]) (+ T[r][3] for c = 3), no
 *     re-orthonormalisation).  Rejected and fixed frames keep their pose and still serve as targets;
 *  5. the next round moves the LOCAL clouds by the new poses (no f32 error accumulates) and the rounds stop early once a round
 *     accepts no increment other than the identity.
 * max_corr_dist: the reference's ICP uses 150 m (:520) because it verifies ONE loop candidate against a submap; across a whole
 * session that cap pairs every point of a frame with something, however far.  A CPU prototype on the golden KAIST03 keyframes
 * 0 / 7 / 20 (0.4 m leaf, golden poses, each against the other two) moved the outer frames' clean poses by 0.30-0.90 m with the
 * 150 m cap and by 0.08-0.17 m with a 2 m cap; the middle frame displaced by (0.3, -0.2, 0.05) m and 0.02 rad of yaw came back
 * from 0.471 m / 1.146 deg to 0.062 m / 0.068 deg of its golden pose with the 2 m cap.  The Python wrapper defaults to 2 m.
 * The neighbour search is exact for any cap: a sparse 1 m cell index (sorted cell keys behind a hash table) whose cell width does
 * not grow with the map's extent, searched ring by ring, with a dense sweep for the queries it cannot settle when the cap asks
 * for neighbours beyond the last ring. */
typedef struct {
    double max_corr_dist;           /* as scal_icp_config */
    double transformation_epsilon;
    double fitness_epsilon;
    double fitness_gate;            /* accept iff converged && fitness <= fitness_gate */
    int max_iterations;
    int max_frames;                 /* capacities: keyframes per call ... */
    int max_points;                 /* ... and points of all of them together */
    int device;
} scal_refine_config;
typedef struct {
    int converged, iterations, state, n_correspondences;  /* of the last round, as scal_icp_result (state 0: fixed frame) */
    int accepted;           /* the last round's T went into the pose */
    double fitness;         /* capped at max_corr_dist (see above); DBL_MAX without a correspondence */
    double T[16];           /* the last round's transformation, row-major, f32 values */
} scal_refine_frame_result;
typedef struct scal_refine scal_refine_t;
int scal_refine_create(const scal_refine_config* cfg, scal_refine_t** ctx);   /* SCAL_E_NO_DEVICE without a gfx950 device */
void scal_refine_destroy(scal_refine_t* ctx);
/* n_frames keyframes in their LOCAL frames, 16-byte xyzi records back to back in device memory: frame f = records [offsets[f],
 * offsets[f+1]) (host array, offsets[0] = 0, non-decreasing), as scal_mapmerge_add_batch_device takes them; thin them first
 * (scal_voxel_downsample_device, 0.4 m in the reference's ICP, :491-492).  poses12: rows of optimized_poses.txt, refined in place.
 * fixed: one byte per frame, non-zero = the pose is held (NULL: none).  res[n_frames], *rounds_run: the rounds executed.
 * SCAL_E_ARG: a NULL pointer, n_frames < 0, rounds < 1, bad offsets, near_thres not finite; SCAL_E_TOO_MANY: more frames or points
 * than the context holds.  Arguments are checked before the device is touched and the context stays usable after any error.  An
 * empty frame and a frame with fewer than 3 correspondences end in state 5, not accepted, pose kept. */
int scal_refine_run_device(scal_refine_t* ctx, const float* d_xyzi, const int* offsets, int n_frames, double* poses12,
                           const unsigned char* fixed, double near_thres, int rounds, scal_refine_frame_result* res, int* rounds_run);
/* the same with the records in host memory (staged into the context) */
int scal_refine_run(scal_refine_t* ctx, const float* xyzi, const int* offsets, int n_frames, double* poses12,
                    const unsigned char* fixed, double near_thres, int rounds, scal_refine_frame_result* res, int* rounds_run);

/* ---- the multiview refine with the point-to-plane metric (an extension)
 * The same context, the same scal_refine_config, the same rounds; what differs from scal_refine_run* is the metric of step 2, which
 * is scal_icp_align_plane's, and what it needs.  The CPU restatement is scaloam/refine_plane.py; the device is held to it bit for
 * bit, so THE ORDER OF THE OPERATIONS BELOW IS PART OF THE INTERFACE.
 *
 * Input normals.  nc [offsets[n_frames]][4] f32, one record per input record: the normal and the curvature of that point among the
 * points of ITS OWN frame in the frame's LOCAL coordinates, in the layout scal_nbr_normals_self writes, NaN rows included.  Local
 * normals do not depend on the poses being refined: the caller computes them once per frame and every round reuses them.  The sign
 * of a normal does not matter (a row and its residual flip together); the curvature is carried along and otherwise ignored.
 *
 * One round is the point refine's round with three differences.
 *  1. The move.  A kept point goes through exactly what step 1 above does (same bits, same near-range rule
 *     sqrt((x x + y y) + z z) > near_thres, same stable compaction) and its normal is written to the same position of the union as
 *         N.x = (float)((P[0] n.x + P[1] n.y) + P[2]  n.z)
 *         N.y = (float)((P[4] n.x + P[5] n.y) + P[6]  n.z)
 *         N.z = (float)((P[8] n.x + P[9] n.y) + P[10] n.z)        N.w = n.w
 *     with P the frame's pose12, every operation in f64 on the promoted f32 components, one rounding each, no translation.  A NaN
 *     component makes the moved normal non-finite, and the sums drop such a correspondence as scal_icp_align_plane does.
 *  2. The sweep.  The neighbour search is the point refine's, untouched.  The sums are scal_icp_align_plane's 32, with the moved
 *     normals of the whole union as the target's normals: source point i of frame f (counted from the frame's first kept point) is
 *     lane i % 64 of wave (i / 64) % 4 of the frame's workgroup i / 256, the frame's workgroups are summed in workgroup order from
 *     +0.  The host step is scal_icp_align_plane's: fewer than 6 rows is state 5, degenerate normal equations state 6; both end the
 *     frame unconverged and not accepted, its pose kept.
 *  3. The result, scal_refine_plane_frame_result: plane_fitness = [28] / [0] and normal_eq = [1..27] of the final sweep (the moved
 *     frame by the whole T, same cap), first_eq = [1..27] of the first sweep.  fitness = [29] / [0] of the final sweep: the mean f32
 *     d over the rows, that is within the cap AND with a finite normal.  This deviates from scal_icp_plane_result::fitness, which is
 *     [31] / [30], uncapped: the refine does not settle far queries when the cap is below the last ring of the search, so [30] and
 *     [31] are no defined quantity here - the reasoning of step 3 above.  Where every source point has its neighbour within the cap
 *     and that neighbour's normal is finite, the two are the same number bit for bit.
 * Acceptance (converged and fitness <= fitness_gate), pose <- T pose, Jacobi rounds, `fixed` and the early stop are the point
 * refine's.
 *
 * The equality held: for every cap, sums [0..29] of every frame in every sweep are those of
 * scal_icp_align_plane(G_f, concat(G_g, g != f), concat(N_g, g != f)), G and N the moved points and normals; therefore T,
 * iterations, state, converged, n_correspondences, plane_fitness, normal_eq and first_eq equal it bit for bit.  Leaving the own
 * frame out keeps the index order among the other frames, so equal distances resolve alike.
 *
 * The first plane call on a context allocates what only these calls need (the moved normals, the 32-wide partials, the pinned
 * [max_frames][32] sums; the normals staging by the first call with host arrays); they are released with the context.  The point
 * refine's results on the same context are not changed by these calls. */
typedef struct {
    int converged, iterations, state, n_correspondences;  /* as scal_refine_frame_result; n_correspondences counts rows; state 6: degenerate */
    int accepted;
    double fitness;         /* mean d over the final sweep's rows (see above); DBL_MAX without one */
    double T[16];
    double plane_fitness;   /* mean r^2 over the final sweep's rows; DBL_MAX without one */
    double normal_eq[27];   /* upper triangle of A^T A (21, row-major) and A^T b (6) of the FINAL sweep: the frame's 6x6 information */
    double first_eq[27];    /* the same of the FIRST sweep */
} scal_refine_plane_frame_result;
/* arguments, checks and error codes as scal_refine_run_device; d_nc == NULL with any point present is SCAL_E_ARG.  Everything is
 * checked before the device is touched and the context stays usable after any error. */
int scal_refine_run_plane_device(scal_refine_t* ctx, const float* d_xyzi, const float* d_nc, const int* offsets, int n_frames,
                                 double* poses12, const unsigned char* fixed, double near_thres, int rounds,
                                 scal_refine_plane_frame_result* res, int* rounds_run);
/* the same with records and normals in host memory (staged into the context) */
int scal_refine_run_plane(scal_refine_t* ctx, const float* xyzi, const float* nc, const int* offsets, int n_frames, double* poses12,
                          const unsigned char* fixed, double near_thres, int rounds, scal_refine_plane_frame_result* res, int* rounds_run);

/* ------------------------------------------------------------------ the four stages as ONE pipelined object
 * The reference runs scanRegistration, laserOdometry, laserMapping and laserPosegraphOptimization as four processes that work on
 * different scans at the same time (node main()s: scanRegistration.cpp:475-517, laserOdometry.cpp:186-600, laserMapping.cpp:909-952,
 * laserPosegraphOptimization.cpp:874-906; hand-over by ROS topics with queue size 100).  scal_pipeline is that arrangement inside one
 * process and one GPU: it owns a ring of features contexts, one odometry, one mapping and one ScanContext context, puts each stage on
 * its own stream (scal_set_stream_mode(1) semantics) and keeps the schedule - which scan each stage may start, when a features
 * context may be rewritten, how many stage-C steps are queued on the device - on five internal host threads (stage A + the first half of
 * stage C's prefetch; its second half + ScanContext's filter, insert and search; stage B; stage C; ScanContext's answers).  Scans go in with push, poses come out IN ORDER with pop; every scan passes through
 * A -> B -> C and A -> D with the reference's data dependencies, and the poses are bit-identical to calling the four stage APIs one
 * scan at a time.  A C++ host (host/replay_main.cpp) and bench.py drive the same object. */
enum {
    SCAL_PIPE_SC_OFF = 0,        /* stages A-C only */
    SCAL_PIPE_SC_EVERY_SCAN = 1, /* makeAndSaveScancontextAndKeys + detectLoopClosureID for every scan (BASELINE config #2's "SC loop search" per scan) */
    SCAL_PIPE_SC_DESCRIPTOR = 2, /* only build each scan's descriptor into device memory (sharded search: the caller exchanges it over RCCL) */
    /* the pose-graph node's keyframe path (laserPosegraphOptimization.cpp:598-639, :713-730, :472-548): stage D gates the stage-C poses
     * into keyframes (scal_keyframe_gate), keeps each keyframe's 0.4 m cloud and pose, inserts only keyframes into ScanContext, searches
     * from the newest keyframe once 30 of the pipeline's own keyframes exist (:715), and verifies every detected loop with ICP between
     * the current keyframe and the loop keyframe's +-25 neighbours, all moved by the loop keyframe's pose and downsampled at 0.4 m
     * (:472-548).  Verified / rejected loops come out with scal_pipeline_pop_loop.  Deviation: the search runs for every keyframe (the
     * project's per-keyframe detect convention), not on the reference's 1 Hz timer (:735-745).  One sequence only. */
    SCAL_PIPE_SC_KEYFRAME = 3
};
typedef struct {
    int lidar_type, n_scans;      /* as scal_features_config */
    double minimum_range;
    int max_points;               /* capacity of one scan */
    int float_math, check_finite;
    float line_res, plane_res;    /* as scal_map_config */
    int max_map_points;
    double sc_max_radius, sc_dist_thres;
    int sc_max_keyframes;
    int sc_mode;                  /* SCAL_PIPE_SC_* */
    int device;
    int ring;                     /* features contexts used in turn: 4..16, 0 = 6 */
    int depth;                    /* stage-C steps queued on the device and not collected: 1..3, 0 = 2 */
    double* d_desc_ring;          /* sc_mode 2: caller-owned device memory for ring x 1200 doubles, scan k's descriptor at slot k % ring
                                   * (NULL: allocated by the pipeline) - so that an RCCL all-gather can read it in place */
    /* sc_mode 3 (0 = the reference's default everywhere) */
    double keyframe_meter_gap;    /* keyframe_meter_gap rosparam, 0 = 2.0 m (:874) */
    double keyframe_deg_gap;      /* keyframe_deg_gap rosparam, 0 = 10 deg (:875) */
    int kf_max_points;            /* keyframe cloud store, points over all keyframes; 0 = no clouds kept, no loop is verified */
    double loop_fitness_thres;    /* loopFitnessScoreThreshold, 0 = 0.3 (:531) */
    int pgo_map_max_points;       /* sc_mode 3: capacity of the pose-graph map in points before its filter; 0 = no map buffers */
} scal_pipeline_config;
typedef struct {
    long long seq;                        /* 0, 1, 2 ... in push order */
    double q_w_curr[4], t_w_curr[3];      /* /aft_mapped_to_init (laserMapping.cpp:861-876) */
    double q_odom[4], t_odom[3];          /* /laser_odom_to_init (laserOdometry.cpp:508-522) */
    scal_odom_stats odom;
    scal_map_stats map;
    int have_loop;                        /* sc_mode 1: `loop` is detectLoopClosureID's answer with this scan as the query */
    scal_sc_result loop;
    const double* d_descriptor;           /* sc_mode 2: this scan's 20x60 descriptor in device memory (valid until `ring` more scans were pushed) */
    /* sc_mode 3: `have_loop` / `loop` are the search with this keyframe as the query (have_loop = 0 while fewer than 30 keyframes
     * of the pipeline exist, and for scans that are not keyframes) */
    int is_keyframe;
    int keyframe_id;                      /* its ScanContext database index (pre-filled entries count), -1 = not a keyframe */
} scal_pipeline_result;
typedef struct scal_pipeline scal_pipeline_t;
int scal_pipeline_create(const scal_pipeline_config* cfg, scal_pipeline_t** p);
void scal_pipeline_destroy(scal_pipeline_t* p);
/* One scan, xyz in device memory (stride in floats); returns as soon as the scan is registered - the buffer must stay valid until the
 * scan's result has been popped.  Blocks only while `ring` scans are in flight; SCAL_E_STATE when 32 results wait to be popped. */
int scal_pipeline_push_device(scal_pipeline_t* p, const float* d_xyz, int n, int stride_floats);
/* The same from host memory (PointCloud2 layout, as scal_features_run): the scan is copied into pinned staging and uploaded on
 * stage A's stream; the caller's buffer is free when the call returns. */
int scal_pipeline_push_host(scal_pipeline_t* p, const void* xyz, int n, int stride_bytes);
/* Result of the oldest scan not yet popped; blocks until its mapping pose (and, in sc_mode 1 and 3, its loop answer) is on the host.
 * An error of any stage is returned here (and by every later call) with the failing stage's message in scal_last_error(). */
int scal_pipeline_pop(scal_pipeline_t* p, scal_pipeline_result* out);
/* waits until every pushed scan has its result ready AND the last scan's map insertion has finished (sc_mode 3: and every detected
 * loop has been verified); results stay queued for pop */
int scal_pipeline_drain(scal_pipeline_t* p);
/* scans pushed and not popped */
int scal_pipeline_in_flight(scal_pipeline_t* p);
/* the contexts inside (owned by the pipeline): pre-fill the ScanContext database, export the map, read statistics.  Only while the
 * pipeline is drained. */
scal_sc_t* scal_pipeline_sc(scal_pipeline_t* p);
scal_map_t* scal_pipeline_map(scal_pipeline_t* p);
scal_odom_t* scal_pipeline_odom(scal_pipeline_t* p);
scal_features_t* scal_pipeline_features(scal_pipeline_t* p, int i);

/* ---- sc_mode 3: loop candidates and keyframes
 * One detected loop (loop_id >= 0) and its ICP verification (doICPVirtualRelative, :500-548).  The source is the current keyframe's
 * cloud, the target the clouds of keyframes loop_kf-25 .. loop_kf+25 that have one, all moved by loop_kf's pose (local2global with the
 * root keyframe's pose, :479-486, a quirk of the reference kept here) and downsampled at 0.4 m (:491-492); ICP with :519-523's settings. */
typedef struct {
    long long seq;          /* the scan (push order) whose keyframe was the query */
    int curr_kf, loop_kf;   /* ScanContext database indices */
    float yaw_rad;          /* the search's yaw */
    double min_dist;        /* the search's SC distance */
    int verified;           /* 1 accepted (converged && fitness <= loop_fitness_thres), 0 rejected, -1 not verifiable: the current or
                             * the loop keyframe has no stored cloud (a pre-filled database entry, or kf_max_points == 0); no ICP ran */
    int converged, iterations, state; /* as scal_icp_result */
    double fitness;
    double T[16];           /* icp.getFinalTransformation(), row-major */
    int n_src, n_tgt;       /* cloud sizes after the 0.4 m filters */
    double q_rel[4];        /* poseFrom.between(poseTo) (:540-547), x y z w: getTranslationAndEulerAngles of T (f32), */
    double t_rel[3];        /* Rot3::RzRyRx, inverse - in double; set whenever ICP ran */
} scal_pipeline_loop;
/* the oldest loop record not yet popped, in detection order: 1 = *out filled; 0 = none is ready (wait = 0), or none is ready and no
 * verification is pending (wait = 1: blocks while one is); < 0 error.  Push returns SCAL_E_STATE while 64 records wait to be popped
 * (the pipeline itself never waits for this queue).  scal_pipeline_drain also waits for every pending verification. */
int scal_pipeline_pop_loop(scal_pipeline_t* p, scal_pipeline_loop* out, int wait);
/* keyframe kf (database index) of this pipeline, only while drained: pose6 = x y z roll pitch yaw (getOdom, :312-323) and its
 * stored 0.4 m cloud (the one keyframeLaserClouds holds, :629-634): *n = its size, the first min(*n, cap) xyzi records go to xyzi
 * (host; may be NULL with cap 0).  *n = 0 when no clouds are kept.  SCAL_E_ARG for a pre-filled entry or an unknown index. */
int scal_pipeline_keyframe(scal_pipeline_t* p, int kf, double pose6[6], float* xyzi, int cap, int* n);
/* updatePoses (:408-431): the caller's optimized poses for n keyframes of this pipeline, given by database index (as keyframe_id /
 * curr_kf / loop_kf); pose6 = x y z roll pitch yaw (keyframePosesUpdated's Pose6D, the layout scal_pipeline_keyframe returns).
 * Allowed at any time, drained or with scans in flight.  All or nothing: SCAL_E_ARG (and nothing changes) when an id is not a keyframe
 * stage D has assigned to this pipeline (pre-filled entries and unknown ids are refused) or a pose is not finite.  The latest update
 * of a keyframe wins; one never updated keeps its gated pose (:636).  The loop verification (loopFindNearKeyframesCloud, :479-486)
 * moves both ICP clouds by the loop keyframe's updated pose: a loop whose query scan was pushed after this call returned sees this
 * update, one whose query scan was pushed before sees the poses that held when that scan was pushed - whatever the device timing, the
 * schedule or a drain.  scal_pipeline_keyframe keeps returning the gated pose. */
int scal_pipeline_update_keyframe_poses(scal_pipeline_t* p, const int* kf, const double* pose6 /* [n][6] */, int n);
/* pubMap (:810-834) on the device: the pipeline's own keyframes with database index < kf_end, counted in their own order (node_idx),
 * every skip-th starting with the first (the reference: skip 2, kf_end = recentIdxUpdated), each moved by its current pose (the latest
 * update) with local2global's f32 arithmetic (:338-359), concatenated in keyframe order and filtered by pcl::VoxelGrid(leaf)
 * (mapviz_filter_size 0.4, :895-896; PCL's "leaf size too small" guard included: output = input), in PCL order.  *n_out = points of
 * the map; its first min(*n_out, cap) xyzi records go to out_xyzi (host; NULL with cap 0 allowed).  Allowed with scans in flight: it
 * never waits for stage D nor queues work on the pipeline's streams, and returns when the map is complete; concurrent calls run one
 * after the other.  SCAL_E_STATE: sc_mode is not 3, pgo_map_max_points is 0, or kf_end is beyond the keyframes whose append stage D
 * has confirmed (every keyframe_id popped so far is confirmed).  SCAL_E_CAPACITY: more selected points than pgo_map_max_points
 * (*n_out = the points needed, nothing runs), or a bounding box that needs more than 45 key bits.  SCAL_E_ARG: leaf not finite and
 * > 0, skip < 1, kf_end < 0. */
int scal_pipeline_pgo_map(scal_pipeline_t* p, int kf_end, int skip, float leaf, float* out_xyzi, long long cap, long long* n_out);
/* the last map scal_pipeline_pgo_map built: xyzi records in device memory, valid until the next call or destroy; NULL before the first */
const float* scal_pipeline_pgo_map_device(scal_pipeline_t* p, long long* n);

/* ---- sc_mode 3: the pose-graph optimisation itself (process_pg :644-690, process_icp :761-768, runISAM2opt :399-406, updatePoses
 * :408-431) over the pipeline's own keyframes with database index < kf_end (nodes in their own order, node_idx) and the pipeline's
 * accepted loops (verified == 1) whose curr_kf < kf_end - the pipeline keeps them itself, popped by the caller or not.  The graph is
 * the one of scal_posegraph below: prior on node 0 at its gated pose (variances 1e-12, :286-288), odometry edges (k-1, k) = between of the
 * GATED poses (variances 1e-6 x 3 rotation, 1e-4 x 3 translation, :292), one Cauchy(k = 1) loop edge (loop_kf, curr_kf) = (q_rel, t_rel)
 * with variances 0.5 (:295-300) per accepted loop; no GPS factors (:673-681: the pipeline has no GPS input).  Initial estimate: every
 * keyframe's current pose (its latest update, else its gated pose).  Deviation: the batch optimum over these factors, where the reference
 * runs iSAM2 once a second (:791-808).
 * The call waits until every keyframe < kf_end has passed stage D and every loop detected for one of them has been verified, so the
 * graph - and, the solver being deterministic, the result bit for bit - does not depend on device timing, ring, depth, the caller's
 * look-ahead or a drain.  It holds no stage's lock while it waits or solves and queues nothing on the pipeline's four busy streams: the
 * solver runs on the pose-graph map's stream, one map or optimisation at a time.  Its context is created by the first call.
 * Outputs: *res (may be NULL); the first min(n_nodes, cap) keyframe ids and poses (x y z roll pitch yaw with RzRyRx(roll, pitch, yaw) =
 * the optimized rotation, as updatePoses reads them) - SCAL_E_CAPACITY with res->n_nodes set and nothing else done when cap < n_nodes
 * (kf_ids / pose6 may be NULL with cap 0 to ask for the size that way).  apply = 1: the effect of
 * scal_pipeline_update_keyframe_poses(kf_ids, pose6, n_nodes) at the moment the call returns; apply = 0 changes nothing.
 * SCAL_E_STATE: sc_mode is not 3, or kf_end is beyond the keyframes whose append stage D has confirmed (as scal_pipeline_pgo_map).
 * SCAL_E_ARG: kf_end < 0.  A solve that does not converge is not an error: res->solver.converged = 0, the poses are the last accepted ones. */
typedef struct {
    int iterations;           /* Gauss-Newton iterations (linear solves), accepted or not */
    int converged;            /* 1: a step's max-norm fell below step_tol */
    double initial_cost, final_cost;
    int linear_iterations;    /* conjugate-gradient iterations over all solves */
    int linear_status;        /* of the last solve: 0 converged, 1 hit max_linear_iterations, 2 breakdown (system not positive definite) */
    double last_step_max;     /* max-norm of the last computed step [rad | m] */
} scal_posegraph_stats;
typedef struct {
    int n_nodes, n_odom_edges, n_loop_edges, applied;
    scal_posegraph_stats solver;
} scal_pipeline_pgo_result;
int scal_pipeline_optimize_keyframes(scal_pipeline_t* p, int kf_end, int apply, int* kf_ids /* [cap] */, double* pose6 /* [cap][6] */, int cap,
                                     scal_pipeline_pgo_result* res);

/* ---- the keyframe gate (:598-617 with getOdom :312-323 and diffTransformation :325-336), host only, no device needed.  The
 * accumulators start at 1e6 (:67-68), so the first pose is a keyframe; roll/pitch/yaw from tf's getRPY in double, the delta through
 * pcl::getTransformation / getTranslationAndEulerAngles in f32, the rotation summed naively. */
typedef struct {
    double meter_gap, rad_gap;
    double translation_accumulated, rotation_accumulated;
    double curr[6];         /* odom_pose_curr: x y z roll pitch yaw */
} scal_keyframe_gate_state;
int scal_keyframe_gate_init(scal_keyframe_gate_state* st, double meter_gap, double deg_gap);
int scal_keyframe_gate(scal_keyframe_gate_state* st, const double q_xyzw[4], const double t_xyz[3], int* is_keyframe);

/* ---- several independent sequences (sensor streams) on ONE GPU, their kernels sharing launches ("batched /
 * streamed numbers - several independent scans or sequences in flight").  One scan's kernels run on 1..50 workgroups of a 256-CU part
 * and the device advances only four dependent chains at full rate, so S sequences go faster only when their kernels share a launch:
 * every hot-path kernel takes up to 4 argument sets (blockIdx.z selects one), the per-stage calls of the S sequences are recorded and
 * merged position by position (csrc/batch.hpp).  The sequences step together: push one scan of EVERY sequence, pop their S results.
 * Each sequence has its own contexts (map, poses, ScanContext database), and its poses are bit-identical to running it alone. */
int scal_pipeline_create_multi(const scal_pipeline_config* cfg, int n_seqs /* 1..4 */, scal_pipeline_t** p);
int scal_pipeline_seqs(scal_pipeline_t* p);
int scal_pipeline_push_device_multi(scal_pipeline_t* p, const float* const* d_xyz /* [n_seqs] */, const int* n /* [n_seqs] */, int stride_floats);
int scal_pipeline_pop_multi(scal_pipeline_t* p, scal_pipeline_result* out /* [n_seqs] */);
scal_sc_t* scal_pipeline_sc_of(scal_pipeline_t* p, int seq);
scal_map_t* scal_pipeline_map_of(scal_pipeline_t* p, int seq);

/* ------------------------------------------------------------------ factor evaluation (Ceres adapter mode)
 * Batched residual / Jacobian / normal-equation evaluation of lidarFactor.hpp:12-138 blocks at a pose,
 * for a host that keeps ceres::Problem orchestration.  kind: 0 LidarEdgeFactor(a,b),
 * 1 LidarPlaneFactor(j, unit normal), 2 LidarPlaneNormFactor(n, d in pb[0]).  Arrays are [n][3] doubles. */
int scal_factors_eval(int device, int n, const int* kind, const double* cp, const double* pa, const double* pb,
                      const double* x7 /* qx qy qz qw tx ty tz */, double* cost, double* gradient6, double* hessian6x6);

/* ------------------------------------------------------------------ pose-graph optimisation (batch)
 * What the pose-graph node asks of GTSAM (laserPosegraphOptimization.cpp: initNoises :284-310, the factors of process_pg :644-690 and
 * process_icp :761-768, runISAM2opt :399-406), restated from the published algorithms - GTSAM / iSAM2 itself is third-party code and
 * parity with it is unpinned, like the Ceres and PCL restatements.  Nodes are SE(3) poses (pose7 = qx qy qz qw tx ty tz, the layout of
 * scal_factors_eval); one prior Log(P^-1 T) and between edges r = Log(Z^-1 Ti^-1 Tj), the full SE(3) logarithm in GTSAM's tangent order
 * (rotation, then translation), whitened by 1 / sqrt(variance); an edge with cauchy_k > 0 has the cost k^2/2 log(1 + |e|^2/k^2) and is
 * reweighted as gtsam::noiseModel::Robust does (w = k^2 / (k^2 + |e|^2), row block and right-hand side times sqrt(w)).  No GPS factors.
 * Deviation: batch Gauss-Newton over all factors (the optimum iSAM2's estimate approaches), not incremental updates.  A step that would
 * raise the cost is rejected and solved again with Levenberg damping.  Everything is f64 and stays in device memory; the normal
 * equations are solved by conjugate gradients preconditioned with an exact parallel solve of their block-tridiagonal part (the odometry
 * chain).  No float atomics: the result is bitwise reproducible.  scaloam.pgo.optimize_pose_graph is the CPU restatement it is held to. */
typedef struct {
    int device;
    int max_nodes, max_edges;   /* capacities (between edges; the prior is extra) */
} scal_posegraph_config;
typedef struct {                /* 0 = default */
    int max_iterations;         /* Gauss-Newton iterations, default 50 */
    double step_tol;            /* stop when a step's max-norm is below this, default 1e-8 */
    int max_linear_iterations;  /* conjugate-gradient iterations per solve, default 2000; a solve that hits it ends the optimisation */
    double linear_rtol;         /* relative residual (in the preconditioner's norm) of a solve, default 1e-12 */
} scal_posegraph_params;
typedef struct scal_posegraph scal_posegraph_t;
int scal_posegraph_create(const scal_posegraph_config* cfg, scal_posegraph_t** g);   /* SCAL_E_NO_DEVICE without a gfx950 device */
void scal_posegraph_destroy(scal_posegraph_t* g);
/* the estimate (quaternions are normalised); SCAL_E_ARG: n < 1, a pose that is not finite or has a zero quaternion; SCAL_E_CAPACITY: n > max_nodes */
int scal_posegraph_set_nodes(scal_posegraph_t* g, const double* pose7 /* [n][7] */, int n);
/* the one prior (a second call replaces it); SCAL_E_ARG: node outside the nodes set so far, pose not finite, a variance not finite and > 0 */
int scal_posegraph_set_prior(scal_posegraph_t* g, int node, const double* pose7, const double* variances6);
/* n more edges, all or nothing; SCAL_E_ARG: an index outside the nodes set so far, i == j, a pose not finite, a variance not finite and
 * > 0, cauchy_k negative or not finite (cauchy_k NULL = none robust); SCAL_E_CAPACITY: more than max_edges in all */
int scal_posegraph_add_between(scal_posegraph_t* g, int n, const int* i, const int* j, const double* pose7_rel /* [n][7] */,
                               const double* variances6 /* [n][6] */, const double* cauchy_k /* [n] */);
int scal_posegraph_clear_edges(scal_posegraph_t* g);   /* the between edges; nodes and prior stay */
/* SCAL_E_STATE: no nodes, no prior, or an edge / the prior names a node beyond the current nodes.  A solve that does not converge is not
 * an error (stats->converged = 0, the nodes are the last accepted estimate).  params and stats may be NULL. */
int scal_posegraph_optimize(scal_posegraph_t* g, const scal_posegraph_params* params, scal_posegraph_stats* stats);
int scal_posegraph_get_nodes(scal_posegraph_t* g, double* pose7 /* [n][7] */, int n);   /* SCAL_E_ARG unless n = the number of nodes */
/* robust weights of the between edges at the current estimate, in the order they were added (1 for edges that are not robust): which
 * loops were down-weighted.  SCAL_E_ARG unless n = the number of edges; SCAL_E_STATE before the first optimize on these edges. */
int scal_posegraph_get_edge_weights(scal_posegraph_t* g, double* w /* [n] */, int n);

/* ------------------------------------------------------------------ relocalisation against a stored session
 * An extension: the reference's README lists "SLAM with multi-session localization" as a TODO and ships its two hooks uncalled
 * (saveScancontextAndKeys, Scancontext.cpp:236-246; detectLoopClosureIDBetweenSession, :272-333).  A context holds one saved session -
 * per keyframe its Scans/NNNNNN.pcd cloud, its line of optimized_poses.txt and its descriptor - and answers "where is this scan in
 * it": scal_sc_detect_between finds the place, ICP against a submap around it verifies it and gives the pose.
 *
 * add_keyframe does what the node does before it stores a keyframe (laserPosegraphOptimization.cpp:629-639): VoxelGrid(leaf) of the
 * cloud (the device filter of scal_voxel_*), the filtered cloud into an xyzi arena in HBM, the descriptor from the filtered cloud
 * (makeAndSaveScancontextAndKeys) or as given by the caller (saveScancontextAndKeys of a reloaded SCDs/NNNNNN.scd).
 *
 * query, one launch chain on the context's stream (every part of the context runs on that one stream); the clouds never leave HBM:
 *  1. source = VoxelGrid(leaf) of the query cloud;
 *  2. its descriptor and keys (not inserted);
 *  3. scal_sc_detect_between; loop_id < 0: status 0, nothing more runs.  c = loop_id;
 *  4. target = the stored clouds of keyframes j in [c - h, c + h] (h = submap_half) that exist, in keyframe order, each brought into
 *     keyframe c's frame, then VoxelGrid(leaf).  Keyframe c's cloud is copied unchanged; every other j is moved by
 *     M_j = P_c^-1 P_j, computed in f64 with all sums left to right and then rounded to an f32 3x4:
 *         Ri = Rc^T,   ti[r] = -((Ri[r][0] tc[0] + Ri[r][1] tc[1]) + Ri[r][2] tc[2]),
 *         M[r][k] = (Ri[r][0] Pj[0][k] + Ri[r][1] Pj[1][k]) + Ri[r][2] Pj[2][k]   (+ ti[r] for k = 3),
 *     and applied with local2global's f32 arithmetic (:338-359), ((m0 x + m1 y) + m2 z) + m3 per coordinate.
 *     DEVIATION from loopFindNearKeyframesCloud (:472-494), which moves all 2h + 1 clouds by the ROOT keyframe's single pose (:482):
 *     inside one odometry frame that stack is what the reference verifies with, but against a stored session it would smear the
 *     submap over 2h keyframe gaps; here every cloud is moved by its own pose;
 *  5. guess G = Rz(-sc.yaw_rad): cos and sin of the f32 yaw taken in double and rounded to f32, G = [c s 0 0; -s c 0 0; 0 0 1 0;
 *     0 0 0 1].  The shift comes from distanceBtnScanContext(query, candidate), which turns the CANDIDATE onto the query, hence the
 *     sign.  no_yaw_guess = 1: the identity, as the reference's verification starts (it computes the yaw and drops it, :722).
 *     On the golden KAIST03 keyframes (CPU oracle) ICP from the identity fails for every heading
 *     difference of about 90 degrees or more and the guess repairs all of them;
 *  6. scal_icp_align_guess_device(source, target, G);
 *  7. status = 1 iff converged and fitness <= fitness_thres, else 2; pose12 = P_c T in f64 (T's f32 values promoted;
 *     (P[r][0] T[0][k] + P[r][1] T[1][k]) + P[r][2] T[2][k], + P[r][3] for k = 3): the query's pose in the session's frame.
 * Capacities: the arena holds max_points filtered records over all keyframes; the work buffers hold max_query_points records - one
 * query cloud BEFORE its filter, and one submap before its filter (the sum of the stored clouds of its keyframes). */
typedef struct {
    int max_keyframes, max_points;   /* stored session: keyframes, xyzi records over all stored (filtered) clouds */
    int max_query_points;            /* one query cloud before the filter (and one submap before its filter) */
    double sc_max_radius, sc_dist_thres;   /* 0 = 80, 0.2 */
    int float_math;
    float leaf;                      /* 0 = 0.4 (downSizeFilterScancontext / downSizeFilterICP) */
    int submap_half;                 /* 0 = 25 (historyKeyframeSearchNum); -1 = the candidate keyframe alone */
    double fitness_thres;            /* 0 = 0.3 */
    double max_corr_dist, transformation_epsilon, fitness_epsilon;   /* 0 = 150, 1e-6, 1e-6 */
    int max_iterations;              /* 0 = 100 */
    int no_yaw_guess;                /* 1 = start ICP from identity, as the reference's verification does */
    int device;
} scal_reloc_config;
typedef struct {
    scal_sc_result sc;       /* the between-session search */
    int status;              /* 0 no place found (sc.loop_id < 0), 1 accepted, 2 rejected by ICP (not converged or fitness > thres) */
    int n_src, n_tgt;        /* cloud sizes after the filters (status 0: n_tgt = 0) */
    scal_icp_result icp;     /* T: query frame -> candidate keyframe's frame, guess included; all zero for status 0 */
    double pose12[12];       /* status 1 or 2: P_candidate * T, the query's pose in the session's frame, row-major 3x4 */
} scal_reloc_result;
typedef struct scal_reloc scal_reloc_t;
int scal_reloc_create(const scal_reloc_config* cfg, scal_reloc_t** ctx);   /* SCAL_E_NO_DEVICE without a gfx950 device */
void scal_reloc_destroy(scal_reloc_t* ctx);
int scal_reloc_size(scal_reloc_t* ctx);   /* keyframes stored */
/* one keyframe of a saved session in its local frame, pose12 = its line of optimized_poses.txt; desc_colmajor NULL: the descriptor is
 * built from the filtered cloud.  Returns the keyframe index (>= 0).  SCAL_E_CAPACITY when the arena or the database is full - nothing
 * is stored -, SCAL_E_TOO_MANY for more than max_query_points points, SCAL_E_ARG for a pose that is not finite. */
int scal_reloc_add_keyframe(scal_reloc_t* ctx, const float* xyzi, int n, const double pose12[12], const double* desc_colmajor_or_NULL);
/* SCAL_E_STATE: no keyframe stored.  SCAL_E_TOO_MANY: more than max_query_points points.  SCAL_E_CAPACITY: the submap does not fit the
 * work buffers (or a voxel grid needs more than 45 key bits).  The context stays usable after any of them. */
int scal_reloc_query(scal_reloc_t* ctx, const float* xyzi, int n, scal_reloc_result* out);
/* nq queries, cloud q = records [offsets[q], offsets[q + 1]): steps 1-2 for all of them, one batched search per 64 queries, then steps
 * 4-7 per found candidate.  Every record equals the single call's bit for bit. */
int scal_reloc_query_batch(scal_reloc_t* ctx, const float* xyzi, const int* offsets /* [nq + 1] */, int nq, scal_reloc_result* out /* [nq] */);
scal_sc_t* scal_reloc_sc(scal_reloc_t* ctx);    /* the session's database (owned by the context), e.g. for scal_sc_cross_search between two sessions */

/* ------------------------------------------------------------------ dynamic-point removal from a merged keyframe map
 * An extension: the reference's README names the second offline use of a saved session (Scans/ + optimized_poses.txt) - "remove
 * dynamic points using these saved keyframe poses and scans ... see our Removert project" - and ships no code for it.  The semantics
 * are those of the CPU restatement python/scaloam/removert.py, which the device path equals bit for bit (DESIGN.md section 8.10 has
 * the differences from Removert itself).
 *
 * Projection of a point p from a pose [R|t] (sensor to world) at `res` degrees per pixel, H = max(1, lround((fov_up - fov_down) / res)),
 * W = lround(360 / res); all in f64, every operation rounded once (no fused multiply-add), in this order:
 *     d = p - t,   x = (R00 d0 + R10 d1) + R20 d2   (y, z: columns 1, 2),   r = (float)sqrt((x x + y y) + z z),
 *     az = atan2(y, x),   el = atan2(z, sqrt(x x + y y)),   u = (az + pi) / (2 pi) * W,   col = min((int)u, W - 1),
 *     v = (fu - el) / (fu - fd) * H   with fu = fov_up_deg * (pi / 180), fd likewise.
 * The point takes part iff min_range <= r <= max_range (both in f32) and 0 <= v < H; row = (int)v.  Scan points are projected from
 * the identity pose.  A scan's range image at `res` holds per pixel the smallest r of its points (empty where none falls).
 * Keyframe k HITS map point m at `res` iff m takes part in k's view, its pixel in k's image is not empty and (scan_r - r_m) >
 * diff_thres in f32: k's ray went through the place where m lies.  hits(m, res) = the number of keyframes that hit m, and
 *     dynamic(m) = [some remove resolution has hits >= min_hits] AND [every revert resolution has hits >= 1].
 * Pointwise: the result does not depend on the order of points or keyframes.  Hit counts saturate at 65535.
 *
 * Device memory comes from the config and does not grow with the session: a run of more than max_keyframes keyframes, or of more
 * than max_scan_points scan records, goes through the device in chunks of consecutive keyframes (hits add up, the result is the
 * same).  (point, keyframe) pairs are culled by XY cells of cell_size: a cell's points are tested against the keyframes within
 * max_range plus the cell's half diagonal of its centre, which drops no pair the range test would accept. */
typedef struct {
    int max_points;           /* map records (<= 2^30) */
    int max_keyframes;        /* keyframes resident at once */
    int max_scan_points;      /* scan records resident at once; no single scan may have more */
    int max_resolutions;      /* remove + revert resolutions of one run, 1 .. 8 */
    int min_hits;             /* >= 1 (and <= 65535) */
    int device;
    double fov_up_deg, fov_down_deg;          /* -90 <= fov_down < fov_up <= 90 */
    double min_range, max_range, diff_thres;  /* all > 0, min_range <= max_range */
    double min_res_deg;       /* the finest resolution a run may ask for (it sizes the images); 0 = 1.0 */
    double cell_size;         /* culling cells; 0 = max_range / 8 */
} scal_removert_config;
typedef struct {
    long long points, keyframes, dynamic;
    long long pairs_tested;       /* (point, keyframe) pairs that were projected */
    long long pairs_bruteforce;   /* points * keyframes */
} scal_removert_stats;
typedef struct scal_removert scal_removert_t;
/* SCAL_E_NO_DEVICE without a gfx950 device; SCAL_E_ARG (before any device work) for a NULL pointer, a capacity < 1, max_resolutions
 * > 8, a range, threshold, min_res_deg or cell_size that is NaN, infinite or negative (zero too where the config has no default for
 * it), fov_up <= fov_down or outside +-90, min_range > max_range, min_hits < 1 */
int scal_removert_create(const scal_removert_config* cfg, scal_removert_t** ctx);
void scal_removert_destroy(scal_removert_t* ctx);
/* the map: n xyzi records in the world frame, copied to the device and binned into cells.  Records that are not finite never take
 * part.  SCAL_E_TOO_MANY: n > max_points. */
int scal_removert_set_map(scal_removert_t* ctx, const float* xyzi, int n);
/* the same for records already in device memory, as scal_mapmerge_device_points returns them (wait for the merge first:
 * scal_mapmerge_size does).  Nothing is copied: the records must stay where they are until the next set_map. */
int scal_removert_set_map_device(scal_removert_t* ctx, const float* d_xyzi, int n);
/* K keyframes: scan k = host records [offsets[k], offsets[k + 1]) of scans_xyzi in its sensor frame (offsets[0] = 0, non-decreasing),
 * poses12 [K][12] as optimized_poses.txt has them.  dynamic_out [n] (host), hits_out [n] (host, may be NULL): hits at the finest
 * remove resolution (the first of the smallest).  SCAL_E_STATE: no map set.  SCAL_E_ARG: a NULL pointer, K < 0, n_remove < 1,
 * n_revert < 0, more than max_resolutions in all, a resolution that is NaN, below min_res_deg or above 360, bad offsets, a pose that
 * is not finite.  SCAL_E_TOO_MANY: one scan has more than max_scan_points records. */
int scal_removert_run(scal_removert_t* ctx, const float* scans_xyzi, const int* offsets, int K, const double* poses12,
                      const double* remove_res, int n_remove, const double* revert_res, int n_revert, unsigned char* dynamic_out,
                      unsigned short* hits_out_or_NULL, scal_removert_stats* stats);
/* the map records of the last run that are static (which = 0) or dynamic (which = 1), in input order: *n_out of them, the first cap
 * written to out_xyzi (host; may be NULL with cap 0).  SCAL_E_STATE before the first run on this map. */
int scal_removert_compact(scal_removert_t* ctx, int which, float* out_xyzi, int cap, int* n_out);
/* keyframe k's range image at resolution res_index (remove resolutions first, then revert) of the last run, +inf where empty: for
 * tracing a parity failure to the half of the algorithm that caused it.  SCAL_E_ARG unless H and W are that image's; SCAL_E_STATE
 * before the first run or for a keyframe that is not in the last chunk the run processed (its images are gone). */
int scal_removert_scan_image(scal_removert_t* ctx, int k, int res_index, float* out /* [H * W] */, int H, int W);

/* ------------------------------------------------------------------ radius neighbour index
 * An extension (no counterpart in the reference): how many records of an indexed cloud lie within a fixed radius of each query, and
 * how near the nearest of them is.  It is the primitive of the map diff between two sessions that share a frame and of a
 * RadiusOutlierRemoval-style noise filter (python/scaloam/nbr.py, which is also the CPU restatement the device equals bit for bit;
 * DESIGN.md section 8.11).
 *
 * Index set I and query set Q: xyzi records; intensity is carried along and never read.  r finite and > 0, r2 = (float)r * (float)r
 * rounded to f32.  For a query q and an index record p, both finite in x, y, z:
 *     d2 = ((qx - px)*(qx - px) + (qy - py)*(qy - py)) + (qz - pz)*(qz - pz)      f32, every operation rounded once (no FMA)
 * p is WITHIN q iff d2 <= r2.  count(q) = the number of index records within q, saturating at 65535; min_d2(q) = the smallest such
 * d2, or +inf when there is none.  A record that is not finite takes no part as an index record and gets count 0 and +inf as a
 * query.  In a self query (Q = I) a point counts itself, as PCL's radiusSearch does.  min and a saturating count do not depend on the
 * order of evaluation: the result is defined bit for bit, pointwise, with no margin condition.
 *
 * k nearest neighbours.  Call p a CANDIDATE of q iff both are finite and d2 <= r2, d2 and r2 as above.  The
 * candidates of q are ordered by the pair (d2, input position of p in I), ascending: a total order, so duplicates and equidistant
 * records have a defined place.  knn(q, k), 1 <= k <= SCAL_NBR_MAX_K, is the first k candidates: one row of idx (int32 input
 * positions) and one row of d2 (float32) per query.  A row with fewer than k candidates is padded with -1 in idx and +inf in d2; a
 * query that is not finite gets a fully padded row.  A self query returns the point itself first, or an exact duplicate of it with a
 * lower position (PCL's nearestKSearch behaviour).  The result is defined bit for bit, with no margin condition.
 * A full row is the k nearest of ALL of I: every record that is not a candidate has d2 > r2 >= the row's last d2, strictly, so no tie
 * crosses the bound.  Unbounded k-NN is therefore exact by asking the short rows again at twice the radius (scaloam.nbr.knn); the
 * device primitive is the bounded one and uses the index as it is.
 *
 * Device memory comes from the config and does not grow with the map, with one exception: the k-NN rows of scal_nbr_knn and
 * scal_nbr_knn_self are staged in 8 bytes x k x the queries of the call (4 for an output that is NULL), allocated at the first such
 * call and grown to the largest so far - 1.2 GB for a self query of 7.1 M points at k = 21.  A context that never asks for
 * neighbours pays nothing, and scal_nbr_knn_device writes to the caller's buffers and stages nothing.
 *
 * Normals and point-to-plane distances (scaloam.nbr.normals_within is the restatement).  The neighbourhood of
 * a query q is its knn(q, k) row exactly as defined above, 3 <= k <= SCAL_NBR_MAX_K; m is its number of entries, p_s its records in
 * row order.  Everything below is f64, every operation rounded once (no FMA), and every sum runs sequentially in row order from +0:
 * the order of the sums is part of the interface.
 *   centroid     c = (sum_s p_s) / m per axis, p_s converted exactly from f32.
 *   covariance   d_s = p_s - c; the six sums of dx dx, dx dy, dx dz, dy dy, dy dz, dz dz over a second pass, each divided by m.
 *   eigenvectors cyclic Jacobi on A = the covariance, V = identity, with + - * / sqrt, compares and selects only: up to 8 sweeps over
 *                the pairs (p, q) = (0, 1), (0, 2), (1, 2), r the third index.  A pair with a_pq == 0 leaves A and V untouched.
 *                Otherwise theta = (a_qq - a_pp) / (2 a_pq), t = 1 / (|theta| + sqrt(theta theta + 1)), negated where theta < 0,
 *                c = 1 / sqrt(t t + 1), s = t c, h = t a_pq; a_pp -= h, a_qq += h, a_pq = 0; (a_rp, a_rq) becomes
 *                (c a_rp - s a_rq, s a_rp + c a_rq), and so does (v_ip, v_iq) for every row i of V.
 *   normal       the column of V under the smallest diagonal entry lambda_min, the lowest column on ties.
 *   curvature    (lambda_min > 0 ? lambda_min : 0) / tr for tr = (a_00 + a_11) + a_22, and 0 where tr <= 0.
 *   viewpoint    three doubles, optional: with v = viewpoint - q, the normal is negated iff (nx vx + ny vy) + nz vz < 0.  Without a
 *                viewpoint the sign is what the rotations deliver - deterministic, not oriented.
 *   distance     (nx ex + ny ey) + nz ez for e = q - c, after the flip: the signed distance of q to the plane through c.
 * Outputs: nc [n][4] float32 - the normal's components rounded to f32, then the curvature - and dist [n] float32.  Where m < 3
 * (a query that is not finite has m = 0) all five values are the quiet NaN SCAL_NBR_NAN_BITS.  The host entry points stage nc and
 * dist in max(max_index_points, max_query_points) entries each, allocated when first asked for, and the first normals call of a
 * context allocates a position table of 4 bytes x max_index_points, refilled from the index's own records after every set_index. */
#define SCAL_NBR_MAX_K 64
#define SCAL_NBR_NAN_BITS 0x7fc00000u
typedef struct {
    int device;
    int max_index_points;     /* 1 .. 2^30 */
    int max_query_points;     /* 1 .. 2^30; queries of one call (a self query may have max_index_points) */
} scal_nbr_config;
typedef struct scal_nbr scal_nbr_t;
/* SCAL_E_NO_DEVICE without a gfx950 device; SCAL_E_ARG (before any device work) for a NULL pointer or a capacity < 1 */
int scal_nbr_create(const scal_nbr_config* cfg, scal_nbr_t** ctx);
void scal_nbr_destroy(scal_nbr_t* ctx);
/* the index: n xyzi records (host), n = 0 allowed (every later count is 0).  A second call replaces index and radius.
 * SCAL_E_ARG: a radius that is not finite and > 0 (as a double and as the float it is rounded to), n < 0, a NULL pointer with n > 0.
 * SCAL_E_CAPACITY: n > max_index_points. */
int scal_nbr_set_index(scal_nbr_t* ctx, const float* xyzi, int n, double radius);
/* the same for records in device memory, as scal_mapmerge_device_points returns them (wait for the merge first: scal_mapmerge_size
 * does).  The records are copied into the index's own order before the call returns. */
int scal_nbr_set_index_device(scal_nbr_t* ctx, const float* d_xyzi, int n, double radius);
/* n queries (host) -> count_u16 [n], min_d2 [n] (host; either may be NULL).  SCAL_E_STATE before any set_index; SCAL_E_CAPACITY:
 * n > max_query_points (nothing runs; callers split the set, the result does not depend on how). */
int scal_nbr_query(scal_nbr_t* ctx, const float* xyzi, int n, unsigned short* count_u16, float* min_d2);
/* queries and outputs in device memory; waits for the result */
int scal_nbr_query_device(scal_nbr_t* ctx, const float* d_xyzi, int n, unsigned short* d_count_u16, float* d_min_d2);
/* the index records themselves as the queries, outputs (host) in the order the index was given in */
int scal_nbr_query_self(scal_nbr_t* ctx, unsigned short* count_u16, float* min_d2);
/* n queries (host), 1 <= k <= SCAL_NBR_MAX_K -> idx [n][k], d2 [n][k] (host; either may be NULL), rows as defined above.
 * SCAL_E_ARG (before any device work): a NULL context, n < 0, a NULL query pointer with n > 0, k out of range.  SCAL_E_STATE: no index
 * set.  SCAL_E_CAPACITY: n > max_query_points.  SCAL_E_HIP: the staging could not be allocated; the context stays usable. */
int scal_nbr_knn(scal_nbr_t* ctx, const float* xyzi, int n, int k, int* idx, float* d2);
/* queries and outputs in device memory; waits for the result */
int scal_nbr_knn_device(scal_nbr_t* ctx, const float* d_xyzi, int n, int k, int* d_idx, float* d_d2);
/* the index records themselves as the queries, rows (host) in the order the index was given in */
int scal_nbr_knn_self(scal_nbr_t* ctx, int k, int* idx, float* d2);
/* n queries (host), 3 <= k <= SCAL_NBR_MAX_K, viewpoint3 three doubles or NULL -> nc [n][4], dist [n] (host; either may be NULL), as
 * defined above.  Error codes as scal_nbr_knn (k < 3 is SCAL_E_ARG). */
int scal_nbr_normals(scal_nbr_t* ctx, const float* xyzi, int n, int k, const double* viewpoint3, float* nc, float* dist);
/* queries and outputs in device memory (viewpoint3 stays a host pointer); waits for the result */
int scal_nbr_normals_device(scal_nbr_t* ctx, const float* d_xyzi, int n, int k, const double* viewpoint3, float* d_nc, float* d_dist);
/* the index records themselves as the queries, outputs (host) in the order the index was given in */
int scal_nbr_normals_self(scal_nbr_t* ctx, int k, const double* viewpoint3, float* nc, float* dist);
/* of the last query, radius, k-NN or normals: (query, record) pairs tested and work items (pieces of up to 64 queries of one cell) */
int scal_nbr_stats(scal_nbr_t* ctx, long long* pairs, int* work_items);

#ifdef __cplusplus
}
#endif
#endif /* SCALOAM_HIP_H */
