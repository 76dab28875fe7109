// scal_pipeline: the reference's four concurrently running nodes (scanRegistration.cpp:475-517, laserOdometry.cpp:186-600,
// laserMapping.cpp:909-952, laserPosegraphOptimization.cpp:874-906) as one object on one GPU.  See include/scaloam_hip.h.
//
// The schedule (what round 2 kept in bench.py's Python threads) lives here, on five host threads that only ever queue work:
//   front   stage A of scan k on features context k % ring, then the lane-0 half of stage C's pose-independent prefetch (input gather
//           + corner stack filter); a features context is rewritten only when the scan that used it last has left stage C (pose
//           collected), has been queued into stage B and has been handed to ScanContext (the library's reader events then order the
//           device side);
//   side    the side-lane half of the prefetch (surf stack filter) and ScanContext's keyframe filter + descriptor + insert + search;
//   odom    stage B is queued up to two scans ahead of the pose it hands to stage C, its poses are collected (the only thing this
//           thread ever waits for);
//   pose    a collected odometry pose goes straight into stage C's enqueue, which queues behind the stage-C steps still running on
//           the device (`depth` uncollected); finished steps are collected;
//   loop    ScanContext's answers, collected one scan behind their searches.
// sc_mode 3 (keyframes) moves ScanContext behind stage C, as the pose-graph node sits behind laserMapping: the side thread does only the
// prefetch half (as with ScanContext off); the loop thread becomes stage D - in scan order it waits for the scan's stage-C pose, runs
// the keyframe gate and, for a keyframe, queues the ScanContext insert with the keyframe store's append behind it and (30 keyframes
// on) the search, then collects the answer; a detected loop goes to a sixth thread that verifies it (keyframes.hip) on its own stream.
// Nothing here touches the device except through the per-stage C-ABI, so the poses are those of the per-stage calls.
#include "common.hpp"
#include "keyframes.hpp"
#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <deque>
#include <chrono>
#include <cstdlib>
#include <string>
#include <thread>

namespace scal {
void print_forced_flushes();
}
using namespace scal;

namespace {
constexpr int REC_N = 64;      // per-scan records (ring); at most 32 scans may be pushed and not popped
constexpr int MAX_UNPOPPED = 32;
constexpr int MAX_LOOPS_UNPOPPED = 64;  // sc_mode 3: loop records detected and not popped
// development knobs (environment), read once: how far the stages may run ahead of each other
int env_int(const char* name, int dflt, int lo, int hi) {
    const char* e = std::getenv(name);
    if (!e) return dflt;
    const int v = std::atoi(e);
    return v < lo ? lo : (v > hi ? hi : v);
}
const int B_AHEAD = env_int("SCALOAM_PIPE_B_AHEAD", 2, 1, 3);     // stage-B steps queued and not collected
const int PF_AHEAD = env_int("SCALOAM_PIPE_PF_AHEAD", 3, 1, 3);   // scal_map::MAX_PF: prefetches queued ahead of their steps

// SCALOAM_PIPE_TIMING=1: host time spent inside each stage call, printed per scan when the pipeline is destroyed (development aid)
const bool TIMING = env_int("SCALOAM_PIPE_TIMING", 0, 0, 1) != 0;
struct HostTimer {
    const char* name[12] = {};
    double total[12] = {};
    long calls[12] = {};
    template <class F>
    int run(int slot, const char* nm, F&& f) {
        if (!TIMING) return f();
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = f();
        name[slot] = nm;
        total[slot] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        calls[slot]++;
        return rc;
    }
    void print(const char* thread) const {
        for (int i = 0; i < 12; ++i)
            if (calls[i]) std::fprintf(stderr, "[scal_pipeline] %-6s %-28s %8.1f us/call x %ld\n", thread, name[i], total[i] / calls[i], calls[i]);
    }
};

constexpr int SMAX = scal::BATCH_MAX;  // sequences that share launches
struct Rec {
    const float* d_xyz[SMAX] = {};
    const void* h_xyz[SMAX] = {};
    int n[SMAX] = {};
    int stride = 0;
    bool host = false;
    scal_pipeline_result res[SMAX] = {};
};
}  // namespace

struct scal_pipeline {
    scal_pipeline_config cfg{};
    int ring = 6, depth = 2;
    int S = 1;  // independent sequences stepping together; S > 1: their per-stage calls are recorded and zipped (batch.hpp)
    std::vector<scal_features_t*> regs[SMAX];
    scal_odom_t* od[SMAX] = {};
    scal_map_t* mp[SMAX] = {};
    scal_sc_t* sc[SMAX] = {};
    double* d_desc = nullptr;  // sc_mode 2: ring x 1200 doubles (S = 1 only)
    bool own_desc = false;
    Rec rec[REC_N];
    std::mutex mu;
    std::condition_variable cv;
    // monotone counters, all guarded by mu: scan k is "done" for a stage when counter > k
    long long pushed = 0, a_run = 0, a_done = 0, pf_done = 0, b_enq = 0, b_coll = 0, c_enq = 0, c_coll = 0, d_ins = 0, d_coll = 0, popped = 0;
    int pop_waiting = 0;
    bool drain_req = false, drained = true;
    bool stop = false;
    int err = SCAL_OK;
    std::string errmsg;
    std::thread t_front, t_side, t_odom, t_pose, t_loop;
    HostTimer tm_front, tm_side, tm_odom, tm_pose, tm_loop;
    // sc_mode 3: keyframe gate and store (stage D's thread), loops waiting for verification / to be popped
    KeyframeStore* kf = nullptr;
    scal_keyframe_gate_state gate{};
    double fitness_thres = LOOP_FITNESS_THRES;
    std::deque<KfLoopJob> jobs;
    std::deque<scal_pipeline_loop> loops;
    bool verifying = false;
    long long verifying_seq = 0;  // the job being verified (verifying)
    long long loops_owed = 0;  // detected and not popped
    std::thread t_verify;
    // sc_mode 3, scal_pipeline_optimize_keyframes: the accepted loops in detection order (kept whether or not the caller pops them), how
    // far stage D has got in keyframes, and the optimizer (created by the first call, used under the keyframe store's map_mu)
    struct AcceptedLoop {
        int curr_kf, loop_kf;
        double q[4], t[3];
    };
    std::vector<AcceptedLoop> accepted;
    int verifying_kf = -1;   // curr_kf of the job being verified (verifying)
    int kf_passed_end = 0;   // database index + 1 of the newest own keyframe that has left stage D (its loop, if any, is in `jobs` or further)
    scal_posegraph_t* pg = nullptr;

    bool sc_on() const { return cfg.sc_mode != SCAL_PIPE_SC_OFF; }
    bool side_sc() const { return cfg.sc_mode == SCAL_PIPE_SC_EVERY_SCAN || cfg.sc_mode == SCAL_PIPE_SC_DESCRIPTOR; }  // ScanContext behind stage A
    bool kf_mode() const { return cfg.sc_mode == SCAL_PIPE_SC_KEYFRAME; }
    bool verify_idle() const { return jobs.empty() && !verifying; }
    Rec& r(long long k) { return rec[k % REC_N]; }
    // one per-stage call for every sequence.  S = 1: the call itself.  S > 1: each sequence's call runs under a recorder (nothing
    // reaches the device), then the S lists are zipped: same kernel, same shape -> one launch with gridDim.z = S.
    template <class F>
    int for_all(F&& f) {
        if (S == 1) return f(0);
        Recorder recs[SMAX];
        Recorder* ptr[SMAX];
        int rc = SCAL_OK;
        for (int q = 0; q < S && rc == SCAL_OK; ++q) {
            ptr[q] = &recs[q];
            g_recorder = &recs[q];
            rc = f(q);
            g_recorder = nullptr;
        }
        if (rc != SCAL_OK) {  // what the earlier sequences queued still has to run: their host state already counts on it
            for (int q = 0; q < S; ++q) (void)recs[q].flush();
            return rc;
        }
        if (zip_and_launch(ptr, S) != hipSuccess) {
            set_error("scal_pipeline: a batched launch failed: %s", hipGetErrorString(hipGetLastError()));
            return SCAL_E_HIP;
        }
        return SCAL_OK;
    }
    // calls that wait for the device: one after the other
    template <class F>
    int for_each(F&& f) {
        for (int q = 0; q < S; ++q) SCAL_TRY(f(q));
        return SCAL_OK;
    }
    void fail(int rc) {  // called with mu held, from the thread whose stage call failed
        if (err == SCAL_OK) {
            err = rc;
            errmsg = scal_last_error();
        }
        cv.notify_all();
    }
};

namespace {

// Lane 0's thread: stage A of scan k and, right behind it on the same stream, the first half of stage C's prefetch (input gather +
// corner stack filter).
void front_thread(scal_pipeline* p) {
    std::unique_lock<std::mutex> lk(p->mu);
    for (;;) {
        const long long k = p->a_done;
        p->cv.wait(lk, [&] {
            if (p->stop || p->err) return true;
            if (p->pushed <= k) return false;
            const long long old = k - p->ring;  // the scan that used this features context last
            if (old >= 0 && (p->c_coll <= old || p->b_enq <= old || (p->sc_on() && p->d_ins <= old))) return false;
            return k - p->c_enq < PF_AHEAD;     // prefetches queued ahead of their stage-C steps
        });
        if (p->stop || p->err) return;
        const Rec& rc = p->r(k);
        const int slot = static_cast<int>(k % p->ring);
        lk.unlock();
        int st = p->tm_front.run(0, "A: features_run", [&] {
            return p->for_all([&](int q) {
                scal_features_t* reg = p->regs[q][slot];
                return rc.host ? scal_features_enqueue_host(reg, rc.h_xyz[q], rc.n[q], rc.stride) : scal_features_run_device(reg, rc.d_xyz[q], rc.n[q], rc.stride);
            });
        });
        if (st == SCAL_OK) {
            lk.lock();
            p->a_run = k + 1;  // stage B may be queued behind stage A at once
            p->cv.notify_all();
            lk.unlock();
            st = p->tm_front.run(1, "C: prefetch, lane 0 half", [&] { return p->for_all([&](int q) { return scal_map_prefetch_begin(p->mp[q], p->regs[q][slot]); }); });
        }
        lk.lock();
        if (st != SCAL_OK) {
            p->fail(st);
            return;
        }
        p->a_done = k + 1;
        p->cv.notify_all();
    }
}

// The side lane's thread: everything else that only needs stage A - the second half of stage C's prefetch (surf stack filter) and
// ScanContext's keyframe filter + descriptor + insert + search.  The two big voxel filters - same kernels, same stream, different
// clouds - are recorded and SHARE their launches (zip_marked_and_launch): ~200 us of side-stream time per scan become ~110.  With
// several sequences all 2 S filter runs are merged the same way.  (One thread issued lane 0's and the side lane's launches until the
// chains got short enough for its 130-220 us of launch calls per scan to be the longest thing in the period.)
void side_thread(scal_pipeline* p) {
    std::unique_lock<std::mutex> lk(p->mu);
    const bool search = p->cfg.sc_mode == SCAL_PIPE_SC_EVERY_SCAN;
    for (;;) {
        const long long k = p->pf_done;
        p->cv.wait(lk, [&] {
            if (p->stop || p->err) return true;
            if (p->a_done <= k) return false;
            return !(p->side_sc() && k - p->d_coll >= 3);  // the ScanContext context holds four searches / descriptors in flight
        });
        if (p->stop || p->err) return;
        const int slot = static_cast<int>(k % p->ring);
        lk.unlock();
        double* dd = p->d_desc ? p->d_desc + static_cast<size_t>(slot) * 1200 : nullptr;
        int st = p->tm_side.run(1, "C: prefetch, side half + D: insert", [&]() -> int {
            if (!p->side_sc() && p->S == 1) return scal_map_prefetch_finish(p->mp[0], p->regs[0][slot]);
            Recorder recs[2 * SMAX];
            Recorder* ptr[2 * SMAX];
            int nr = 0, rc2 = SCAL_OK;
            rc2 = p->tm_side.run(3, "   record prefetch", [&] {
                int r3 = SCAL_OK;
                for (int q = 0; q < p->S && r3 == SCAL_OK; ++q) {
                    g_recorder = ptr[nr] = &recs[nr];
                    ++nr;
                    r3 = scal_map_prefetch_finish(p->mp[q], p->regs[q][slot]);
                    g_recorder = nullptr;
                }
                return r3;
            });
            if (rc2 == SCAL_OK && p->side_sc())
                rc2 = p->tm_side.run(4, "   record insert", [&] {
                    int r3 = SCAL_OK;
                    for (int q = 0; q < p->S && r3 == SCAL_OK; ++q) {
                        g_recorder = ptr[nr] = &recs[nr];
                        ++nr;
                        r3 = search ? scal_sc_insert_features(p->sc[q], p->regs[q][slot]) : scal_sc_make_features_enqueue(p->sc[q], p->regs[q][slot], dd);
                        g_recorder = nullptr;
                    }
                    return r3;
                });
            if (rc2 != SCAL_OK) {  // what was recorded still has to run: the contexts' host state already counts on it
                for (int i = 0; i < nr; ++i) (void)recs[i].flush();
                return rc2;
            }
            return p->tm_side.run(5, "   zip + launch", [&]() -> int {
                if (zip_marked_and_launch(ptr, nr) != hipSuccess) {
                    set_error("scal_pipeline: a batched launch failed: %s", hipGetErrorString(hipGetLastError()));
                    return SCAL_E_HIP;
                }
                return SCAL_OK;
            });
        });
        if (st == SCAL_OK && search) st = p->tm_side.run(2, "D: sc_detect_enqueue", [&] { return p->for_all([&](int q) { return scal_sc_detect_enqueue(p->sc[q]); }); });
        lk.lock();
        if (st != SCAL_OK) {
            p->fail(st);
            return;
        }
        p->r(k).res[0].d_descriptor = dd;
        p->pf_done = k + 1;
        if (p->side_sc()) p->d_ins = k + 1;
        p->cv.notify_all();
    }
}

// Stage B's thread: queues the odometry steps (up to B_AHEAD in front of the collected ones) and collects their poses.  It only ever
// waits for stage B: while the two stages shared a thread, the wait for a pose (100 us) kept finished stage-C steps from being collected
// and the caller's next push from starting.
void odom_thread(scal_pipeline* p) {
    std::unique_lock<std::mutex> lk(p->mu);
    for (;;) {
        enum { NONE, B_ENQ, B_COLL } what = NONE;
        p->cv.wait(lk, [&] {
            if (p->stop || p->err) return true;
            if (p->b_enq < p->a_run && p->b_enq - p->b_coll < B_AHEAD) { what = B_ENQ; return true; }
            // a pose is only collected when stage C has room to take it soon: the record of an uncollected step is not reused meanwhile
            if (p->b_coll < p->b_enq && p->b_coll - p->c_enq < 2) { what = B_COLL; return true; }
            return false;
        });
        if (p->stop || p->err) return;
        int st = SCAL_OK;
        if (what == B_ENQ) {
            const long long k = p->b_enq;
            const int slot = static_cast<int>(k % p->ring);
            lk.unlock();
            st = p->tm_odom.run(0, "B: odom_enqueue_features", [&] { return p->for_all([&](int q) { return scal_odom_enqueue_features(p->od[q], p->regs[q][slot]); }); });
            lk.lock();
            if (st == SCAL_OK) p->b_enq = k + 1;
        } else {
            const long long k = p->b_coll;
            scal_pipeline_result* R = p->r(k).res;
            lk.unlock();
            st = p->tm_odom.run(1, "B: odom_collect (wait)", [&] {
                return p->for_each([&](int q) {
                    double qlc[4], tlc[3];
                    return scal_odom_collect(p->od[q], qlc, tlc, R[q].q_odom, R[q].t_odom, &R[q].odom);
                });
            });
            lk.lock();
            if (st == SCAL_OK) p->b_coll = k + 1;
        }
        if (st != SCAL_OK) {
            p->fail(st);
            return;
        }
        p->cv.notify_all();
    }
}

// Stage C's thread: a collected stage-B pose goes straight into a stage-C step (at most depth + 1 of them in flight, scal_map allows 4),
// finished steps are collected.
void pose_thread(scal_pipeline* p) {
    std::unique_lock<std::mutex> lk(p->mu);
    for (;;) {
        enum { NONE, C_ENQ, C_COLL, FINISH } what = NONE;
        p->cv.wait(lk, [&] {
            if (p->stop || p->err) return true;
            const long long inflight = p->c_enq - p->c_coll;
            if (p->c_enq < p->b_coll && p->c_enq < p->pf_done && inflight <= p->depth) { what = C_ENQ; return true; }
            // A pose is collected when more than `depth` steps are queued on the device - or at once when the caller waits for it and
            // nothing more can be queued meanwhile (every pushed scan has its step queued): never at the price of an empty queue.
            if (inflight > p->depth || (inflight > 0 && (p->pop_waiting || p->drain_req) && p->c_enq == p->pushed)) { what = C_COLL; return true; }
            if (p->drain_req && p->c_coll == p->pushed) { what = FINISH; return true; }
            return false;
        });
        if (p->stop || p->err) return;
        int st = SCAL_OK;
        if (what == C_ENQ) {
            const long long k = p->c_enq;
            const int slot = static_cast<int>(k % p->ring);
            scal_pipeline_result* R = p->r(k).res;
            lk.unlock();
            st = p->tm_pose.run(2, "C: map_enqueue_features", [&] {
                return p->for_all([&](int q) { return scal_map_enqueue_features(p->mp[q], p->regs[q][slot], R[q].q_odom, R[q].t_odom); });
            });
            lk.lock();
            if (st == SCAL_OK) p->c_enq = k + 1;
        } else if (what == C_COLL) {
            const long long k = p->c_coll;
            scal_pipeline_result* R = p->r(k).res;
            lk.unlock();
            st = p->tm_pose.run(3, "C: map_collect (wait)", [&] {
                return p->for_each([&](int q) { return scal_map_collect(p->mp[q], R[q].q_w_curr, R[q].t_w_curr, &R[q].map); });
            });
            lk.lock();
            if (st == SCAL_OK) p->c_coll = k + 1;
        } else if (what == FINISH) {
            lk.unlock();
            st = p->for_each([&](int q) { return scal_map_finish(p->mp[q]); });  // the last scan's map insertion (:738-802) belongs to the work
            lk.lock();
            if (st == SCAL_OK) p->drain_req = false, p->drained = true;
        }
        if (st != SCAL_OK) {
            p->fail(st);
            return;
        }
        p->cv.notify_all();
    }
}

void loop_thread(scal_pipeline* p) {  // ScanContext's answers (the searches themselves are queued by the front thread)
    std::unique_lock<std::mutex> lk(p->mu);
    const bool search = p->cfg.sc_mode == SCAL_PIPE_SC_EVERY_SCAN;
    for (;;) {
        p->cv.wait(lk, [&] {
            if (p->stop || p->err) return true;
            // an answer is collected one scan behind its search - a whole period to finish - or as soon as somebody waits for it
            const long long infl = p->d_ins - p->d_coll;
            return infl >= 2 || (infl > 0 && (p->pop_waiting || p->drain_req));
        });
        if (p->stop || p->err) return;
        const long long k = p->d_coll;
        scal_pipeline_result* R = p->r(k).res;
        lk.unlock();
        int st;
        if (search) {
            st = p->tm_loop.run(2, "D: sc_detect_collect (wait)", [&] {
                return p->for_each([&](int q) {
                    const int rc = scal_sc_detect_collect(p->sc[q], &R[q].loop);
                    R[q].have_loop = rc == SCAL_OK;
                    return rc;
                });
            });
        } else {
            st = scal_sc_wait_descriptor(p->sc[0]);
        }
        lk.lock();
        if (st != SCAL_OK) {
            p->fail(st);
            return;
        }
        p->d_coll = k + 1;
        p->cv.notify_all();
    }
}

// sc_mode 3, stage D (laserPosegraphOptimization.cpp:590-639, :713-730): scan k's stage-C pose through the keyframe gate, in scan order.  A
// keyframe is inserted into ScanContext from its features context (keyframe filter 0.4 m + descriptor), its filtered cloud appended to the
// keyframe store behind the descriptor, and - once the pipeline has 30 keyframes of its own (:715) - searched for.  A scan that is not a
// keyframe passes at once.  The insert is queued before d_ins lets the front thread reuse the features context.
void keyframe_thread(scal_pipeline* p) {
    std::unique_lock<std::mutex> lk(p->mu);
    for (;;) {
        const long long k = p->d_coll;
        p->cv.wait(lk, [&] { return p->stop || p->err || p->c_coll > k; });
        if (p->stop || p->err) return;
        scal_pipeline_result& R = p->r(k).res[0];
        const int slot = static_cast<int>(k % p->ring);
        lk.unlock();
        int is_kf = 0;
        bool detect = false;
        int st = scal_keyframe_gate(&p->gate, R.q_w_curr, R.t_w_curr, &is_kf);
        R.is_keyframe = is_kf, R.keyframe_id = -1, R.have_loop = 0;
        if (st == SCAL_OK && is_kf) {
            const int id = scal_sc_size(p->sc[0]);
            double p6[6];
            pose6_from(R.q_w_curr, R.t_w_curr, p6);
            st = p->tm_loop.run(0, "D: insert + append", [&] { return p->kf->insert(p->sc[0], p->regs[0][slot], id, p6); });
            if (st == SCAL_OK) {
                R.keyframe_id = id;
                detect = p->kf->own_count() >= 30;  // performSCLoopClosure: keyframePoses.size() < NUM_EXCLUDE_RECENT -> no search
                if (detect) st = p->tm_loop.run(1, "D: sc_detect_enqueue", [&] { return scal_sc_detect_enqueue(p->sc[0]); });
            }
        }
        lk.lock();
        if (st != SCAL_OK) {
            p->fail(st);
            return;
        }
        p->d_ins = k + 1;
        p->cv.notify_all();
        lk.unlock();
        if (detect) {
            st = p->tm_loop.run(2, "D: sc_detect_collect (wait)", [&] { return scal_sc_detect_collect(p->sc[0], &R.loop); });
            R.have_loop = st == SCAL_OK;
        }
        if (st == SCAL_OK && is_kf) st = p->kf->check();  // the append has run: an overflowing store is reported with this scan
        lk.lock();
        if (st != SCAL_OK) {
            p->fail(st);
            return;
        }
        if (detect && R.loop.loop_id >= 0) {  // scLoopICPBuf (:726)
            p->jobs.push_back(KfLoopJob{k, R.keyframe_id, R.loop.loop_id, R.loop.yaw_rad, R.loop.min_dist});
            p->loops_owed++;
        }
        if (is_kf) p->kf_passed_end = R.keyframe_id + 1;
        p->d_coll = k + 1;
        p->cv.notify_all();
    }
}

// sc_mode 3: process_icp (:777-800) - every detected loop, oldest first, on the keyframe store's own stream
void verify_thread(scal_pipeline* p) {
    std::unique_lock<std::mutex> lk(p->mu);
    for (;;) {
        p->cv.wait(lk, [&] { return p->stop || p->err || !p->jobs.empty(); });
        if (p->stop || p->err) return;
        const KfLoopJob job = p->jobs.front();
        p->jobs.pop_front();
        p->verifying = true, p->verifying_seq = job.seq, p->verifying_kf = job.curr_kf;
        lk.unlock();
        scal_pipeline_loop rec;
        const int st = p->kf->verify(job, p->fitness_thres, &rec);
        lk.lock();
        p->verifying = false;
        if (st != SCAL_OK) {
            p->fail(st);
            return;
        }
        p->loops.push_back(rec);
        if (rec.verified == 1) {
            scal_pipeline::AcceptedLoop a{rec.curr_kf, rec.loop_kf, {rec.q_rel[0], rec.q_rel[1], rec.q_rel[2], rec.q_rel[3]}, {rec.t_rel[0], rec.t_rel[1], rec.t_rel[2]}};
            p->accepted.push_back(a);
        }
        p->cv.notify_all();
    }
}

int report(scal_pipeline* p) {  // mu held
    set_error("%s", p->errmsg.c_str());
    return p->err;
}

int push(scal_pipeline* p, const float* const* d_xyz, const void* const* h_xyz, const int* n, int stride, bool host) {
    std::unique_lock<std::mutex> lk(p->mu);
    if (p->err) return report(p);
    if (p->pushed - p->popped >= MAX_UNPOPPED) {
        set_error("scal_pipeline_push: %d results wait to be popped", MAX_UNPOPPED);
        return SCAL_E_STATE;
    }
    if (p->loops_owed >= MAX_LOOPS_UNPOPPED) {
        set_error("scal_pipeline_push: %d loop records wait to be popped (scal_pipeline_pop_loop)", MAX_LOOPS_UNPOPPED);
        return SCAL_E_STATE;
    }
    const long long k = p->pushed;
    Rec& rc = p->r(k);
    rc = Rec();
    for (int q = 0; q < p->S; ++q) {
        rc.d_xyz[q] = d_xyz ? d_xyz[q] : nullptr, rc.h_xyz[q] = h_xyz ? h_xyz[q] : nullptr, rc.n[q] = n[q];
        rc.res[q].seq = k;
    }
    rc.stride = stride, rc.host = host;
    p->pushed = k + 1;
    p->drained = false;
    p->cv.notify_all();
    // a host buffer belongs to the caller again when this returns: wait until stage A has staged it.  A device buffer is only
    // registered; the call blocks while `ring` scans are in flight (back-pressure instead of an unbounded queue).
    p->cv.wait(lk, [&] { return p->err || (host ? p->a_done > k : p->a_done + p->ring > k); });
    if (p->err) return report(p);
    return SCAL_OK;
}

int pop(scal_pipeline* p, scal_pipeline_result* out) {
    std::unique_lock<std::mutex> lk(p->mu);
    if (p->popped >= p->pushed && !p->err) {
        set_error("scal_pipeline_pop: nothing pushed");
        return SCAL_E_STATE;
    }
    const long long k = p->popped;
    p->pop_waiting++;
    p->cv.notify_all();
    p->cv.wait(lk, [&] { return p->err || (p->c_coll > k && (!p->sc_on() || p->d_coll > k)); });
    p->pop_waiting--;
    if (p->err) return report(p);
    for (int q = 0; q < p->S; ++q) out[q] = p->r(k).res[q];
    p->popped = k + 1;
    p->cv.notify_all();
    return SCAL_OK;
}

int create(const scal_pipeline_config* cfg, int n_seqs, scal_pipeline_t** out) {
    if (!cfg || !out) {
        set_error("scal_pipeline_create: null argument");
        return SCAL_E_ARG;
    }
    *out = nullptr;
    const int ring = cfg->ring == 0 ? 6 : cfg->ring, depth = cfg->depth == 0 ? 2 : cfg->depth;
    if (ring < 4 || ring > 16 || depth < 1 || depth > 3 || cfg->sc_mode < 0 || cfg->sc_mode > 3) {
        set_error("scal_pipeline_create: ring must be 4..16, depth 1..3, sc_mode 0..3");
        return SCAL_E_ARG;
    }
    if (n_seqs < 1 || n_seqs > SMAX || (n_seqs > 1 && (cfg->sc_mode == SCAL_PIPE_SC_DESCRIPTOR || cfg->sc_mode == SCAL_PIPE_SC_KEYFRAME))) {
        set_error("scal_pipeline_create_multi: 1..%d sequences (sc_mode 2 and 3 only with one)", SMAX);
        return SCAL_E_ARG;
    }
    scal_keyframe_gate_state gate{};
    if (cfg->sc_mode == SCAL_PIPE_SC_KEYFRAME) {  // zero: the reference's defaults (:874-876, :531)
        if (cfg->kf_max_points < 0 || !(cfg->loop_fitness_thres >= 0) || cfg->sc_max_keyframes <= 0 ||
            scal_keyframe_gate_init(&gate, cfg->keyframe_meter_gap == 0 ? 2.0 : cfg->keyframe_meter_gap,
                                    cfg->keyframe_deg_gap == 0 ? 10.0 : cfg->keyframe_deg_gap) != SCAL_OK) {
            set_error("scal_pipeline_create: sc_mode 3 needs keyframe gaps >= 0, kf_max_points >= 0, loop_fitness_thres >= 0, sc_max_keyframes > 0");
            return SCAL_E_ARG;
        }
    }
    if (cfg->pgo_map_max_points < 0 || (cfg->pgo_map_max_points > 0 && (cfg->sc_mode != SCAL_PIPE_SC_KEYFRAME || cfg->kf_max_points == 0))) {
        set_error("scal_pipeline_create: pgo_map_max_points must be >= 0, and > 0 only in sc_mode 3 with kf_max_points > 0");
        return SCAL_E_ARG;
    }
    SCAL_TRY(select_device(cfg->device));
    auto* p = new scal_pipeline();
    p->cfg = *cfg, p->ring = ring, p->depth = depth, p->S = n_seqs;
    p->gate = gate;
    p->fitness_thres = cfg->loop_fitness_thres == 0 ? LOOP_FITNESS_THRES : cfg->loop_fitness_thres;
    int rc = SCAL_OK;
    if (p->kf_mode()) {
        p->kf = new KeyframeStore();
        rc = p->kf->init(cfg->device, cfg->kf_max_points, cfg->sc_max_keyframes, cfg->pgo_map_max_points);
    }
    scal_features_config fc{};
    fc.lidar_type = cfg->lidar_type, fc.n_scans = cfg->n_scans, fc.minimum_range = cfg->minimum_range, fc.max_points = cfg->max_points;
    fc.float_math = cfg->float_math, fc.check_finite = cfg->check_finite, fc.device = cfg->device;
    for (int q = 0; q < n_seqs && rc == SCAL_OK; ++q) {
        for (int i = 0; i < ring && rc == SCAL_OK; ++i) {
            scal_features_t* f = nullptr;
            rc = scal_features_create(&fc, &f);
            if (rc == SCAL_OK) p->regs[q].push_back(f);
        }
        if (rc == SCAL_OK) {
            scal_odom_config oc{};
            oc.max_points = cfg->max_points, oc.device = cfg->device;
            rc = odom_create(&oc, StreamLayout::PerStage, &p->od[q]);  // one stream per stage
        }
        if (rc == SCAL_OK) {
            scal_map_config mc{};
            mc.line_res = cfg->line_res, mc.plane_res = cfg->plane_res, mc.max_scan_points = cfg->max_points, mc.max_map_points = cfg->max_map_points;
            mc.device = cfg->device;
            rc = map_create(&mc, StreamLayout::PerStage, &p->mp[q]);
        }
        if (rc == SCAL_OK && p->sc_on()) {
            scal_sc_config sc{};
            sc.max_radius = cfg->sc_max_radius, sc.dist_thres = cfg->sc_dist_thres, sc.max_keyframes = cfg->sc_max_keyframes;
            sc.float_math = cfg->float_math, sc.device = cfg->device, sc.n_shards = 1, sc.shard = 0, sc.side_stream = env_int("SCALOAM_PIPE_SC_LANE", 1, 0, 5);
            // ScanContext entirely on the side stream it shares with stage C's surf filter (keyframe filter, descriptor, search: one in-order
            // chain, no cross-stream wait).  With the descriptor + search behind stage B instead (the per-stage layout's own split, lane 0
            // here) stage B's chain queues behind a search that waits for the keyframe filter on the other stream: 3250-3360 scans/s against
            // 3660 on one box (tools/gpu_pipe_knobs.sh).
            rc = sc_create(&sc, StreamLayout::PerStage, &p->sc[q]);
            if (rc == SCAL_OK && cfg->sc_mode == SCAL_PIPE_SC_DESCRIPTOR) {
                if (cfg->d_desc_ring) {
                    p->d_desc = cfg->d_desc_ring;
                } else if (hipMalloc(reinterpret_cast<void**>(&p->d_desc), sizeof(double) * 1200 * ring) != hipSuccess) {
                    set_error("scal_pipeline_create: hipMalloc of the descriptor ring failed");
                    rc = SCAL_E_HIP;
                } else {
                    p->own_desc = true;
                }
            }
        }
    }
    if (rc != SCAL_OK) {
        const std::string keep = scal_last_error();
        scal_pipeline_destroy(p);
        set_error("%s", keep.c_str());
        return rc;
    }
    p->t_front = std::thread(front_thread, p);
    p->t_side = std::thread(side_thread, p);
    p->t_odom = std::thread(odom_thread, p);
    p->t_pose = std::thread(pose_thread, p);
    if (p->side_sc()) p->t_loop = std::thread(loop_thread, p);
    if (p->kf_mode()) p->t_loop = std::thread(keyframe_thread, p), p->t_verify = std::thread(verify_thread, p);
    *out = p;
    return SCAL_OK;
}

}  // namespace

extern "C" int scal_pipeline_create(const scal_pipeline_config* cfg, scal_pipeline_t** out) { return create(cfg, 1, out); }
extern "C" int scal_pipeline_create_multi(const scal_pipeline_config* cfg, int n_seqs, scal_pipeline_t** out) { return create(cfg, n_seqs, out); }
extern "C" int scal_pipeline_seqs(scal_pipeline_t* p) { return p ? p->S : 0; }

extern "C" void scal_pipeline_destroy(scal_pipeline_t* p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(p->mu);
        p->stop = true;
        p->cv.notify_all();
    }
    if (p->t_front.joinable()) p->t_front.join();
    if (p->t_side.joinable()) p->t_side.join();
    if (p->t_odom.joinable()) p->t_odom.join();
    if (p->t_pose.joinable()) p->t_pose.join();
    if (p->t_loop.joinable()) p->t_loop.join();
    if (p->t_verify.joinable()) p->t_verify.join();
    if (TIMING) {
        p->tm_front.print("front"), p->tm_side.print("side"), p->tm_odom.print("odom"), p->tm_pose.print("pose"), p->tm_loop.print("loop");
        std::fprintf(stderr, "[scal_pipeline] sequences %d, recorded lists flushed in the middle of an entry point: %ld\n", p->S, g_forced_flushes);
        print_forced_flushes();
    }
    (void)hipSetDevice(p->cfg.device);
    // consumers first: their destructors wait for the streams that still read the features contexts
    for (int q = 0; q < SMAX; ++q) {
        if (p->sc[q]) scal_sc_destroy(p->sc[q]);
        if (p->mp[q]) scal_map_destroy(p->mp[q]);
        if (p->od[q]) scal_odom_destroy(p->od[q]);
    }
    for (int q = 0; q < SMAX; ++q)
        for (auto* f : p->regs[q]) scal_features_destroy(f);
    if (p->pg) scal_posegraph_destroy(p->pg);
    delete p->kf;  // after the ScanContext context, whose stream appended to it
    if (p->d_desc && p->own_desc) (void)hipFree(p->d_desc);
    delete p;
}

static int check_scan(scal_pipeline_t* p, const void* ptr, int n) {
    if ((!ptr && n > 0) || n < 0) {
        set_error("scal_pipeline_push: bad argument");
        return SCAL_E_ARG;
    }
    if (n > p->cfg.max_points) {
        set_error("scan has %d points, capacity is %d", n, p->cfg.max_points);
        return SCAL_E_TOO_MANY;
    }
    return SCAL_OK;
}

extern "C" int scal_pipeline_push_device(scal_pipeline_t* p, const float* d_xyz, int n, int stride_floats) {
    if (!p || stride_floats < 3 || p->S != 1) {
        set_error("scal_pipeline_push_device: bad argument (a pipeline of several sequences takes scal_pipeline_push_device_multi)");
        return SCAL_E_ARG;
    }
    SCAL_TRY(check_scan(p, d_xyz, n));
    return push(p, &d_xyz, nullptr, &n, stride_floats, false);
}

extern "C" int scal_pipeline_push_device_multi(scal_pipeline_t* p, const float* const* d_xyz, const int* n, int stride_floats) {
    if (!p || !d_xyz || !n || stride_floats < 3) {
        set_error("scal_pipeline_push_device_multi: bad argument");
        return SCAL_E_ARG;
    }
    for (int q = 0; q < p->S; ++q) SCAL_TRY(check_scan(p, d_xyz[q], n[q]));
    return push(p, d_xyz, nullptr, n, stride_floats, false);
}

extern "C" int scal_pipeline_push_host(scal_pipeline_t* p, const void* xyz, int n, int stride_bytes) {
    if (!p || stride_bytes < 12 || (stride_bytes % 4) != 0 || stride_bytes > 32 || p->S != 1) {
        set_error("scal_pipeline_push_host: bad argument (stride_bytes must be a multiple of 4 in [12, 32]; one sequence)");
        return SCAL_E_ARG;
    }
    SCAL_TRY(check_scan(p, xyz, n));
    return push(p, nullptr, &xyz, &n, stride_bytes, true);
}

extern "C" int scal_pipeline_pop(scal_pipeline_t* p, scal_pipeline_result* out) {
    if (!p || !out || p->S != 1) {
        set_error("scal_pipeline_pop: bad argument (a pipeline of several sequences takes scal_pipeline_pop_multi)");
        return SCAL_E_ARG;
    }
    return pop(p, out);
}

extern "C" int scal_pipeline_pop_multi(scal_pipeline_t* p, scal_pipeline_result* out) {
    if (!p || !out) {
        set_error("scal_pipeline_pop_multi: null argument");
        return SCAL_E_ARG;
    }
    return pop(p, out);
}

extern "C" int scal_pipeline_drain(scal_pipeline_t* p) {
    if (!p) return SCAL_E_ARG;
    std::unique_lock<std::mutex> lk(p->mu);
    if (p->err) return report(p);
    if (p->drained) return SCAL_OK;
    p->drain_req = true;
    p->pop_waiting++;  // the loop thread collects its last answer, the pose thread every queued pose
    p->cv.notify_all();
    p->cv.wait(lk, [&] { return p->err || (p->drained && (!p->sc_on() || p->d_coll == p->pushed) && p->verify_idle()); });
    p->pop_waiting--;
    if (p->err) return report(p);
    return SCAL_OK;
}

extern "C" int scal_pipeline_pop_loop(scal_pipeline_t* p, scal_pipeline_loop* out, int wait) {
    if (!p || !out) {
        set_error("scal_pipeline_pop_loop: null argument");
        return SCAL_E_ARG;
    }
    std::unique_lock<std::mutex> lk(p->mu);
    if (!p->kf_mode()) {
        set_error("scal_pipeline_pop_loop: only in sc_mode 3");
        return SCAL_E_STATE;
    }
    for (;;) {
        if (p->err) return report(p);
        if (!p->loops.empty()) {
            *out = p->loops.front();
            p->loops.pop_front();
            p->loops_owed--;
            return 1;
        }
        if (!wait || p->verify_idle()) return 0;
        p->cv.wait(lk);
    }
}

extern "C" int scal_pipeline_keyframe(scal_pipeline_t* p, int kf, double pose6[6], float* xyzi, int cap, int* n) {
    if (!p || !pose6 || !n || cap < 0 || (cap > 0 && !xyzi)) {
        set_error("scal_pipeline_keyframe: bad argument");
        return SCAL_E_ARG;
    }
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->err) return report(p);
    if (!p->kf_mode() || !p->drained || p->d_coll != p->pushed || !p->verify_idle()) {
        set_error("scal_pipeline_keyframe: only in sc_mode 3, while the pipeline is drained");
        return SCAL_E_STATE;
    }
    return p->kf->read(kf, pose6, xyzi, cap, n);
}

static int update_poses_locked(scal_pipeline_t* p, const int* kf, const double* pose6, int n);

extern "C" int scal_pipeline_update_keyframe_poses(scal_pipeline_t* p, const int* kf, const double* pose6, int n) {
    if (!p || n < 0 || (n > 0 && (!kf || !pose6))) {
        set_error("scal_pipeline_update_keyframe_poses: bad argument");
        return SCAL_E_ARG;
    }
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->err) return report(p);
    if (!p->kf_mode()) {
        set_error("scal_pipeline_update_keyframe_poses: only in sc_mode 3");
        return SCAL_E_STATE;
    }
    return update_poses_locked(p, kf, pose6, n);
}

static int update_poses_locked(scal_pipeline_t* p, const int* kf, const double* pose6, int n) {  // mu held
    // Stamped with the push counter: the loops of scans pushed from now on see this version.  A loop still to be verified belongs to a
    // queued job, the one being verified, or a scan stage D has not passed yet (seq >= d_coll).
    long long floor = p->d_coll;
    if (!p->jobs.empty()) floor = std::min(floor, p->jobs.front().seq);
    if (p->verifying) floor = std::min(floor, p->verifying_seq);
    return p->kf->update_poses(kf, pose6, n, p->pushed, floor);
}

static int pgo_map_state(scal_pipeline_t* p) {
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->err) return report(p);
    if (!p->kf_mode() || p->cfg.pgo_map_max_points == 0) {
        set_error("scal_pipeline_pgo_map: only in sc_mode 3 with pgo_map_max_points > 0");
        return SCAL_E_STATE;
    }
    return SCAL_OK;
}

extern "C" int scal_pipeline_pgo_map(scal_pipeline_t* p, int kf_end, int skip, float leaf, float* out_xyzi, long long cap, long long* n_out) {
    if (!p || !n_out || cap < 0 || (cap > 0 && !out_xyzi)) {
        set_error("scal_pipeline_pgo_map: bad argument");
        return SCAL_E_ARG;
    }
    *n_out = 0;
    SCAL_TRY(pgo_map_state(p));
    if (!(leaf > 0.f) || !std::isfinite(leaf) || skip < 1 || kf_end < 0) {
        set_error("scal_pipeline_pgo_map: leaf must be finite and > 0, skip >= 1, kf_end >= 0");
        return SCAL_E_ARG;
    }
    return p->kf->pgo_map(kf_end, skip, leaf, out_xyzi, cap, n_out);  // p->mu is not held: the map never waits for the stages
}

extern "C" const float* scal_pipeline_pgo_map_device(scal_pipeline_t* p, long long* n) {
    if (n) *n = 0;
    if (!p || !n || !p->kf_mode() || p->cfg.pgo_map_max_points == 0) return nullptr;
    return p->kf->pgo_map_device(n);
}

namespace {
// Pose6DtoGTSAMPose3 (:193-196): Rot3::RzRyRx(roll, pitch, yaw) as a quaternion + translation -> pose7 (qx qy qz qw tx ty tz)
void pose7_from6(const double* p6, double* p7) {
    const double cr = std::cos(p6[3] / 2), sr = std::sin(p6[3] / 2), cp = std::cos(p6[4] / 2), sp = std::sin(p6[4] / 2);
    const double cy = std::cos(p6[5] / 2), sy = std::sin(p6[5] / 2);
    p7[0] = sr * cp * cy - cr * sp * sy, p7[1] = cr * sp * cy + sr * cp * sy, p7[2] = cr * cp * sy - sr * sp * cy, p7[3] = cr * cp * cy + sr * sp * sy;
    p7[4] = p6[0], p7[5] = p6[1], p7[6] = p6[2];
}
// poseFrom.between(poseTo) (:664-671): a^-1 b
void pose7_between(const double* a, const double* b, double* o) {
    const double x = -a[0], y = -a[1], z = -a[2], w = a[3];  // a's rotation inverted
    o[0] = w * b[0] + x * b[3] + y * b[2] - z * b[1];
    o[1] = w * b[1] - x * b[2] + y * b[3] + z * b[0];
    o[2] = w * b[2] + x * b[1] - y * b[0] + z * b[3];
    o[3] = w * b[3] - x * b[0] - y * b[1] - z * b[2];
    const double d[3] = {b[4] - a[4], b[5] - a[5], b[6] - a[6]};
    const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)},
                            {2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)},
                            {2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)}};
    for (int r = 0; r < 3; ++r) o[4 + r] = (R[r][0] * d[0] + R[r][1] * d[1]) + R[r][2] * d[2];
}
}  // namespace

extern "C" int scal_pipeline_optimize_keyframes(scal_pipeline_t* p, int kf_end, int apply, int* kf_ids, double* pose6, int cap, scal_pipeline_pgo_result* res) {
    if (res) std::memset(res, 0, sizeof *res);
    if (!p || cap < 0 || (cap > 0 && (!kf_ids || !pose6))) {
        set_error("scal_pipeline_optimize_keyframes: bad argument");
        return SCAL_E_ARG;
    }
    {
        std::lock_guard<std::mutex> lk(p->mu);
        if (p->err) return report(p);
        if (!p->kf_mode()) {
            set_error("scal_pipeline_optimize_keyframes: only in sc_mode 3");
            return SCAL_E_STATE;
        }
    }
    if (kf_end < 0) {
        set_error("scal_pipeline_optimize_keyframes: kf_end must be >= 0");
        return SCAL_E_ARG;
    }
    std::vector<int> ids;
    std::vector<std::array<double, 6>> gated, current;
    SCAL_TRY(p->kf->pgo_snapshot(kf_end, &ids, &gated, &current));
    const int n = static_cast<int>(ids.size());
    if (res) res->n_nodes = n;
    if (cap < n) {
        set_error("scal_pipeline_optimize_keyframes: %d keyframes, room for %d", n, cap);
        return SCAL_E_CAPACITY;
    }
    if (n == 0) return SCAL_OK;
    // every keyframe of the graph has left stage D and every loop detected for one of them is verified: the graph no longer depends on timing
    std::vector<scal_pipeline::AcceptedLoop> loops;
    {
        std::unique_lock<std::mutex> lk(p->mu);
        const int need = ids.back() + 1;
        auto pending = [&] {
            if (p->verifying && p->verifying_kf < kf_end) return true;
            for (const KfLoopJob& j : p->jobs)
                if (j.curr_kf < kf_end) return true;
            return false;
        };
        p->cv.wait(lk, [&] { return p->err || p->stop || (p->kf_passed_end >= need && !pending()); });
        if (p->err) return report(p);
        if (p->stop) {  // the pipeline is being destroyed under the call: the graph may be incomplete
            set_error("scal_pipeline_optimize_keyframes: the pipeline is being destroyed");
            return SCAL_E_STATE;
        }
        for (const auto& a : p->accepted)
            if (a.curr_kf < kf_end) loops.push_back(a);
    }
    // Solved on the pose-graph map's lane (2), which carries none of the pipeline's four busy chains, under the map builder's mutex: a map
    // and an optimisation would only queue behind each other on that stream, and the optimizer is one object.  p->mu is not held.
    std::vector<double> x7(7 * static_cast<size_t>(n)), g7(7 * static_cast<size_t>(n));
    scal_posegraph_stats st{};
    {
        std::lock_guard<std::mutex> map_lk(p->kf->map_mu);
        // The poses as they stand now.  The node set is the one of the first snapshot: kf_end lies within the confirmed keyframes, and
        // keyframes are only ever appended behind those, so the own keyframes below kf_end (and n) cannot change.
        SCAL_TRY(p->kf->pgo_snapshot(kf_end, &ids, &gated, &current));
        for (int k = 0; k < n; ++k) pose7_from6(gated[static_cast<size_t>(k)].data(), &g7[7 * static_cast<size_t>(k)]), pose7_from6(current[static_cast<size_t>(k)].data(), &x7[7 * static_cast<size_t>(k)]);
        if (!p->pg) {
            scal_posegraph_config pc{};
            pc.device = p->cfg.device, pc.max_nodes = p->cfg.sc_max_keyframes, pc.max_edges = 2 * p->cfg.sc_max_keyframes;  // a chain + at most one loop per keyframe
            SCAL_TRY(posegraph_create_on_lane(&pc, 2, &p->pg));
        }
        const double var_prior[6] = {1e-12, 1e-12, 1e-12, 1e-12, 1e-12, 1e-12};  // :286-288
        const double var_odom[6] = {1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4};         // :292
        const double var_loop[6] = {0.5, 0.5, 0.5, 0.5, 0.5, 0.5};               // :295
        const size_t m = static_cast<size_t>(n - 1) + loops.size();
        std::vector<int> ei(m), ej(m);
        std::vector<double> ez(7 * m), ev(6 * m), ek(m);
        for (int k = 1; k < n; ++k) {
            const size_t e = static_cast<size_t>(k - 1);
            ei[e] = k - 1, ej[e] = k, ek[e] = 0.0;
            pose7_between(&g7[7 * e], &g7[7 * (e + 1)], &ez[7 * e]);
            std::memcpy(&ev[6 * e], var_odom, sizeof var_odom);
        }
        size_t e = static_cast<size_t>(n - 1);
        for (const auto& a : loops) {
            const auto node = [&](int db) { return static_cast<int>(std::lower_bound(ids.begin(), ids.end(), db) - ids.begin()); };
            ei[e] = node(a.loop_kf), ej[e] = node(a.curr_kf), ek[e] = 1.0;  // Cauchy(1), :297
            std::memcpy(&ez[7 * e], a.q, sizeof a.q), std::memcpy(&ez[7 * e + 4], a.t, sizeof a.t);
            std::memcpy(&ev[6 * e], var_loop, sizeof var_loop);
            ++e;
        }
        SCAL_TRY(scal_posegraph_set_nodes(p->pg, x7.data(), n));
        SCAL_TRY(scal_posegraph_clear_edges(p->pg));
        SCAL_TRY(scal_posegraph_set_prior(p->pg, 0, g7.data(), var_prior));
        SCAL_TRY(scal_posegraph_add_between(p->pg, static_cast<int>(m), ei.data(), ej.data(), ez.data(), ev.data(), ek.data()));
        SCAL_TRY(scal_posegraph_optimize(p->pg, nullptr, &st));
        SCAL_TRY(scal_posegraph_get_nodes(p->pg, x7.data(), n));
    }
    for (int k = 0; k < n; ++k) {
        kf_ids[k] = ids[static_cast<size_t>(k)];
        pose6_from(&x7[7 * static_cast<size_t>(k)], &x7[7 * static_cast<size_t>(k) + 4], pose6 + 6 * static_cast<size_t>(k));
    }
    if (res) res->n_odom_edges = n - 1, res->n_loop_edges = static_cast<int>(loops.size()), res->solver = st;
    if (apply) {
        std::lock_guard<std::mutex> lk(p->mu);
        if (p->err) return report(p);
        SCAL_TRY(update_poses_locked(p, kf_ids, pose6, n));
        if (res) res->applied = 1;
    }
    return SCAL_OK;
}

extern "C" int scal_pipeline_in_flight(scal_pipeline_t* p) {
    if (!p) return 0;
    std::lock_guard<std::mutex> lk(p->mu);
    return static_cast<int>(p->pushed - p->popped);
}

static bool seq_ok(scal_pipeline_t* p, int q) { return p && q >= 0 && q < p->S; }
extern "C" scal_sc_t* scal_pipeline_sc(scal_pipeline_t* p) { return p ? p->sc[0] : nullptr; }
extern "C" scal_map_t* scal_pipeline_map(scal_pipeline_t* p) { return p ? p->mp[0] : nullptr; }
extern "C" scal_odom_t* scal_pipeline_odom(scal_pipeline_t* p) { return p ? p->od[0] : nullptr; }
extern "C" scal_features_t* scal_pipeline_features(scal_pipeline_t* p, int i) {
    return (p && i >= 0 && i < static_cast<int>(p->regs[0].size())) ? p->regs[0][i] : nullptr;
}
extern "C" scal_sc_t* scal_pipeline_sc_of(scal_pipeline_t* p, int seq) { return seq_ok(p, seq) ? p->sc[seq] : nullptr; }
extern "C" scal_map_t* scal_pipeline_map_of(scal_pipeline_t* p, int seq) { return seq_ok(p, seq) ? p->mp[seq] : nullptr; }
