"""scal_pipeline - what bench.py measures and the C++ host ships - against the oracle chain over a long stream.

The other pipeline tests compare it with the per-stage HIP calls over 12-18 scans, and the oracle comparisons of the split entry
points stop at 50 scans.  Here 150 scans of the seeded HDL-64 sequence (BASELINE config #2, seed 205, about 1 m per scan) go
through S.Pipeline: the centre cube of the map window changes several times inside the stream, so speculative stage-C steps are
stopped on the device, redone on the general path and the steps behind them queued again, while later scans are in flight.
Every scan is held to O.features -> O.Odometry -> O.Mapper(0.4, 0.8) -> the oracle ScanContext manager, with the bars of the
50-scan tests (test_long_stream_parity_device_pipeline, test_odometry_stream, test_sc_detect_stream)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 150
LOOP_STRETCH = range(60, 91)   # scans whose oracle descriptors are in both databases before the stream starts
MERGE_MAX = 16384              # csrc/mapping.hip: new points one merge insert takes; the queue's room check counts it per step


def _sorted_rows(a):
    v = np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1, 4)
    return v[np.lexsort((v[:, 3], v[:, 2], v[:, 1], v[:, 0]))]


@pytest.fixture(scope="module")
def scans(hdl64_stream):
    return [hdl64_stream(k) for k in range(N)]


@pytest.fixture(scope="module")
def oracle(O, scans):
    """The oracle chain over the stream, once per module.  The databases are pre-filled with the oracle's own descriptors of
    LOOP_STRETCH (random ones give no loops on this trajectory), so the searches of those scans find real loops."""
    oo, om = O.Odometry(), O.Mapper(0.4, 0.8, voxel_order=1, knn_mode=0)
    per, keyframes = [], []
    for xyz in scans:
        f = O.features(xyz, O.HDL64, 5.0)
        c = f["cloud"]
        a = oo.step(c[f["sharp"]], c[f["less_sharp"]], c[f["flat"]], f["less_flat"])
        q, t, st, _ = om.step(c[f["less_sharp"]], f["less_flat"], c, a[2], a[3])
        per.append(dict(q=q, t=t, q_odom=a[2].copy(), t_odom=a[3].copy(), odom=a[4], n_edge=list(st.n_edge), n_plane=list(st.n_plane),
                        lm_iters=list(st.lm_iters), lm_success=list(st.lm_success), solved=st.solved))
        keyframes.append(O.voxel_grid(c, 0.4)[0])
    maker = O.SCManager(dist_thres=0.4)
    prefill = [maker.makeScancontext(keyframes[k]) for k in LOOP_STRETCH]
    osc = O.SCManager(dist_thres=0.4)
    for d in prefill:
        osc.saveScancontextAndKeys(d)
    for k in range(N):
        osc.makeAndSaveScancontextAndKeys(keyframes[k])
        per[k]["loop"] = osc.detectLoopClosureID()
    maps = [_sorted_rows(om.export(w)) for w in (0, 1)]
    maps_all = [_sorted_rows(om.export_all(w)) for w in (0, 1)]
    return dict(per=per, prefill=prefill, maps=maps, maps_all=maps_all)


def _run_pipeline(S, scans, prefill, ring, ahead, depth, max_map_points=3000000):
    cap = max(s.shape[0] for s in scans) + 1024
    p = S.Pipeline(S.HDL64, 5.0, max_points=cap, max_map_points=max_map_points, sc_mode=S.SC_EVERY_SCAN, sc_dist_thres=0.4,
                   sc_max_keyframes=len(prefill) + len(scans) + 8, ring=ring, depth=depth)
    for d in prefill:
        p.sc.saveScancontextAndKeys(d)
    got = []
    for k in range(len(scans)):
        p.push(scans[k])
        while p.in_flight() > ahead:
            got.append(p.pop())
    p.drain()
    while p.in_flight():
        got.append(p.pop())
    return p, got


def _check_against_oracle(p, got, oracle):
    """the per-scan bars of the 50-scan oracle tests, and the final maps bit for bit; returns the worst pose differences (map,
    odometry) and the number of loop hits"""
    per = oracle["per"]
    assert [g["seq"] for g in got] == list(range(N))
    worst = worst_odom = 0.0
    hits = 0
    for k in range(N):
        g, r = got[k], per[k]
        ms, os_ = g["map"], g["odom"]
        d_odom = max(np.abs(g["q_odom"] - r["q_odom"]).max(), np.abs(g["t_odom"] - r["t_odom"]).max())
        worst_odom = max(worst_odom, d_odom)
        assert d_odom <= 1e-7, (k, d_odom)
        assert list(os_.n_edge) == list(r["odom"].n_edge) and list(os_.n_plane) == list(r["odom"].n_plane), k
        assert list(os_.lm_iters) == list(r["odom"].lm_iters), k
        assert ms.solved == r["solved"], k
        assert list(ms.n_edge) == r["n_edge"] and list(ms.n_plane) == r["n_plane"], (k, list(ms.n_plane), r["n_plane"])
        assert list(ms.lm_iters) == r["lm_iters"] and list(ms.lm_success) == r["lm_success"], k
        d = max(np.abs(g["q"] - r["q"]).max(), np.abs(g["t"] - r["t"]).max())
        worst = max(worst, d)
        assert d <= 1e-6, (k, d)
        gl, ol = g["loop"], r["loop"]
        assert gl["loop_id"] == ol["loop_id"], (k, gl["loop_id"], ol["loop_id"])
        # the database holds the 31 pre-filled descriptors before the first search: every search is past the >= 31 gate
        assert np.array_equal(gl["cand"], ol["cand"]), (k, gl["cand"], ol["cand"])
        assert gl["nn_idx"] == ol["nn_idx"] and gl["yaw"] == ol["yaw"], k   # the oracle reports the best shift as its yaw
        assert abs(gl["min_dist"] - ol["min_dist"]) <= 1e-12 or (np.isnan(gl["min_dist"]) and np.isnan(ol["min_dist"])), k
        hits += ol["loop_id"] >= 0
    for w in (0, 1):
        gm, ga = _sorted_rows(p.map.export(w)), _sorted_rows(p.map.export_all(w))
        assert gm.shape == oracle["maps"][w].shape and np.array_equal(gm, oracle["maps"][w]), (w, gm.shape, oracle["maps"][w].shape)
        assert ga.shape == oracle["maps_all"][w].shape and np.array_equal(ga, oracle["maps_all"][w]), (w, ga.shape, oracle["maps_all"][w].shape)
    return worst, worst_odom, hits


@pytest.mark.parametrize("ring,ahead,depth", [(6, 4, 2), (4, 3, 3), (4, 0, 1)])
def test_pipeline_long_stream_matches_oracle(S, scans, oracle, ring, ahead, depth):
    """(6, 4, 2): bench.py's schedule.  (4, 3, 3): the smallest ring with the deepest stage-C queue - a features context is rerun
    as soon as its pose is collected, while its step's insertion may still have to be redone.  (4, 0, 1): nothing overlaps."""
    p, got = _run_pipeline(S, scans, oracle["prefill"], ring, ahead, depth)
    try:
        worst, worst_odom, hits = _check_against_oracle(p, got, oracle)
        cnt = p.map.path_counters()
        print(f"ring {ring} ahead {ahead} depth {depth}: worst pose difference {worst:.3g}, odometry {worst_odom:.3g}, loop hits {hits}, "
              f"path counters (speculative, general, window redo, insertion redo) {cnt}")
        assert cnt[2] >= 2, cnt     # the centre cube changed at least twice: speculative steps stopped and redone on the general path
        assert cnt[1] <= 12, cnt    # first scan and the window redos: everything else stays on the speculative chain
        assert hits >= 10, hits
    finally:
        p.close()


def test_pipeline_switches_to_the_general_path_when_the_map_pool_fills(S, scans, oracle):
    """map_enqueue queues a step speculatively only while every queued step could still merge MERGE_MAX new points into the pool
    (map.n + queued * MERGE_MAX <= max_map_points).  The pool here holds the stream's final map plus one MERGE_MAX - the room
    the general path's insertion needs - so the speculative chain is turned off 20 to 45 scans before the end (two or three steps
    queued), while the map never overflows.  Same oracle bars."""
    n_final = max(oracle["maps_all"][0].shape[0], oracle["maps_all"][1].shape[0])
    cap = n_final + MERGE_MAX
    p, got = _run_pipeline(S, scans, oracle["prefill"], 6, 4, 2, max_map_points=cap)
    try:
        worst, worst_odom, hits = _check_against_oracle(p, got, oracle)
        cnt = p.map.path_counters()
        # scans whose map (before their insertion) leaves no room for two queued steps: the schedule keeps two or three steps in
        # the queue, so about these take the general path (the host's map size lags the device's by the unconfirmed steps)
        tight = sum(g["map"].n_map_corner_total + 2 * MERGE_MAX > cap for g in got)
        print(f"max_map_points {cap}: worst pose difference {worst:.3g}, odometry {worst_odom:.3g}, loop hits {hits}, "
              f"scans without room for two queued steps {tight}, path counters {cnt}")
        assert tight >= 15, tight
        assert cnt[1] >= 20, cnt   # the general path took over (at most 12 without the switch, test above)
        assert cnt[0] + cnt[1] >= N, cnt
    finally:
        p.close()
