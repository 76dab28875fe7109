"""scal_pipeline sc_mode 3: the pose-graph node's keyframe path (laserPosegraphOptimization.cpp:598-639, :713-730, :472-548) inside the
pipeline - keyframe gate, keyframe cloud store, ScanContext on keyframes, ICP verification of every detected loop.

The stream is an out-and-back OS1-64 drive through the seeded config #3 world (seed 301): 40 scans at 0.5 m, a ramp to a stop, and the
same path backwards (reverse gear, same heading), so that keyframes more than 30 positions later revisit the early places.  The gate
runs at 0.4 m / 10 deg, so almost every scan is a keyframe: enough of them for ScanContext's tree (rebuilt every 30 searches, newest 30
excluded) to reach the early keyframes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GAP_M, GAP_DEG = 0.4, 10.0
KF_POINTS = 6000000
STEPS = [0.5] * 40 + [0.35, 0.2, 0.1, 0.0, -0.1, -0.2, -0.35] + [-0.5] * 42


@pytest.fixture(scope="module")
def stream(worlds, O):
    w = worlds(O.OS1_64, 301)
    q0, t0 = w.pose(0)
    _, t1 = w.pose(10)
    d = t1 - t0
    d[2] = 0
    d /= np.linalg.norm(d)
    x = np.concatenate([[0.0], np.cumsum(STEPS)])
    truth = [t0 + d * xi for xi in x]
    scans = [w.scan_pose(q0, t, 1000 + k) for k, t in enumerate(truth)]
    return scans, [t - t0 for t in truth]


@pytest.fixture(scope="module")
def oracle(O, stream):
    """features -> odometry -> mapper -> KeyframeGate -> voxel_grid(0.4) -> SCManager with performSCLoopClosure's 30-keyframe guard"""
    from scaloam.pgo import KeyframeGate
    scans, truth = stream
    oo, om = O.Odometry(), O.Mapper(0.4, 0.8)
    gate = KeyframeGate(GAP_M, GAP_DEG)
    osc = O.SCManager(max_radius=80.0, dist_thres=0.2)
    per, clouds, err = [], [], 0.0
    for k, xyz in enumerate(scans):
        f = O.features(xyz, O.OS1_64, 0.5)
        c = f["cloud"]
        a = oo.step(c[f["sharp"]], c[f["less_sharp"]], c[f["flat"]], f["less_flat"])
        q, t, _, _ = om.step(c[f["less_sharp"]], f["less_flat"], c, a[2], a[3])
        err = max(err, float(np.linalg.norm(t - truth[k])))
        r = dict(q=q.copy(), t=t.copy(), is_kf=bool(gate(q, t)), kf=-1, loop=None)
        if r["is_kf"]:
            r["kf"] = len(clouds)
            clouds.append(O.voxel_grid(c, 0.4)[0])
            osc.makeAndSaveScancontextAndKeys(clouds[-1])
            if len(clouds) >= 30:
                r["loop"] = osc.detectLoopClosureID()
        per.append(r)
    return dict(per=per, clouds=clouds, err=err)


def _pipeline(S, scans, ring=6, ahead=4, depth=2, kf_max_points=KF_POINTS, prefill=(), **kw):
    cap = max(s.shape[0] for s in scans) + 1024
    p = S.Pipeline(S.OS1_64, 0.5, max_points=cap, line_res=0.4, plane_res=0.8, max_map_points=2000000, sc_mode=S.SC_KEYFRAME,
                   sc_max_radius=80.0, sc_dist_thres=kw.pop("sc_dist_thres", 0.2), sc_max_keyframes=512, ring=ring, depth=depth,
                   keyframe_meter_gap=GAP_M, keyframe_deg_gap=GAP_DEG, kf_max_points=kf_max_points, **kw)
    for d in prefill:
        p.sc.saveScancontextAndKeys(d)
    return p


def _run(S, scans, **kw):
    ahead = kw.pop("ahead", 4)
    p = _pipeline(S, scans, **kw)
    got = []
    for xyz in scans:
        p.push(xyz)
        while p.in_flight() > ahead:
            got.append(p.pop())
    p.drain()
    while p.in_flight():
        got.append(p.pop())
    loops = []
    while True:
        r = p.pop_loop(wait=True)
        if r is None:
            break
        loops.append(r)
    return p, got, loops


def _check_oracle(p, got, loops, oracle, n_prefill=0):
    per = oracle["per"]
    assert [g["seq"] for g in got] == list(range(len(per)))
    worst, n_loops = 0.0, 0
    for k, (g, o) in enumerate(zip(got, per)):
        worst = max(worst, np.abs(g["q"] - o["q"]).max(), np.abs(g["t"] - o["t"]).max())
        assert g["is_keyframe"] == o["is_kf"], k
        assert g["keyframe_id"] == (o["kf"] + n_prefill if o["is_kf"] else -1), k
        assert (g["loop"] is None) == (o["loop"] is None), k
        if o["loop"] is not None:
            a, b = g["loop"], o["loop"]
            assert (a["loop_id"], a["nn_idx"], a["yaw"]) == (b["loop_id"], b["nn_idx"], b["yaw"]), k
            assert abs(a["min_dist"] - b["min_dist"]) <= 1e-5, k
            n_loops += a["loop_id"] >= 0
    assert worst <= 1e-5, worst
    # one record per detected loop, in detection order
    det = [(g["seq"], g["keyframe_id"], g["loop"]["loop_id"]) for g in got if g["loop"] is not None and g["loop"]["loop_id"] >= 0]
    assert [(r["seq"], r["curr_kf"], r["loop_kf"]) for r in loops] == det
    return n_loops


@pytest.fixture(scope="module")
def main_run(S, stream, oracle):
    p, got, loops = _run(S, stream[0], ahead=4)
    kfs = [p.keyframe(i) for i in range(len(oracle["clouds"]))]
    p.close()
    return got, loops, kfs


def test_oracle_tracks_the_out_and_back_stream(oracle):
    assert oracle["err"] < 2.0, oracle["err"]
    n = sum(1 for o in oracle["per"] if o["loop"] is not None and o["loop"]["loop_id"] >= 0)
    assert n >= 3 and len(oracle["clouds"]) >= 62


def test_keyframe_mode_matches_oracle_chain(S, stream, oracle, main_run):
    got, loops, kfs = main_run
    assert _check_oracle(None, got, loops, oracle) >= 3
    assert sum(r["verified"] == 1 for r in loops) >= 1
    from scaloam.pgo import rpy_from_quat
    kf_scans = [g for g in got if g["is_keyframe"]]
    for i, (pose, cloud) in enumerate(kfs):
        assert np.array_equal(cloud.view(np.uint32), oracle["clouds"][i].view(np.uint32)), i
        g = kf_scans[i]
        assert np.array_equal(pose[:3], g["t"]) and np.abs(pose[3:] - np.array(rpy_from_quat(g["q"]))).max() <= 1e-12, i


@pytest.mark.parametrize("ring,ahead,depth", [(6, 0, 2), (4, 4, 3)])
def test_keyframe_mode_schedules(S, stream, oracle, main_run, ring, ahead, depth):
    p, got, loops = _run(S, stream[0], ring=ring, ahead=ahead, depth=depth)
    p.close()
    _check_oracle(None, got, loops, oracle)
    ref = main_run[1]
    assert len(loops) == len(ref)
    for a, b in zip(loops, ref):
        assert a["verified"] == b["verified"] and a["fitness"] == b["fitness"] and np.array_equal(a["T"], b["T"])


def test_loop_verification(S, O, main_run):
    """every record against the same chain built in numpy: local2global with the loop keyframe's pose, VoxelGrid 0.4, ICP"""
    from scaloam.pgo import local2global_f32, relative_pose_from_icp
    _, loops, kfs = main_run
    vg = S.VoxelGrid(max_points=4000000)
    icp = S.LoopICP(max_source=400000, max_target=4000000)
    n_oracle = 0
    for r in loops:
        c, l = r["curr_kf"], r["loop_kf"]
        root = kfs[l][0]
        src = local2global_f32(kfs[c][1], root)
        tgt = np.concatenate([local2global_f32(kfs[j][1], root) for j in range(max(0, l - 25), min(l + 25, c) + 1)])
        so, to = O.voxel_grid(src, 0.4)[0], O.voxel_grid(tgt, 0.4)[0]
        assert (r["n_src"], r["n_tgt"]) == (so.shape[0], to.shape[0]), r
        if n_oracle < 4:
            n_oracle += 1
            ro = O.icp_align(so, to)
            assert (r["converged"], r["state"], r["iterations"]) == (int(ro["converged"]), ro["state"], ro["iterations"]), r
            assert np.abs(r["T"] - ro["T"]).max() <= 1e-9
            assert abs(r["fitness"] - ro["fitness"]) <= 1e-9 * max(1.0, ro["fitness"])
        else:
            rs = icp.align(vg.filter(src, 0.4), vg.filter(tgt, 0.4))
            assert (r["converged"], r["state"], r["iterations"]) == (int(rs["converged"]), rs["state"], rs["iterations"]), r
            assert np.array_equal(r["T"], rs["T"]) and r["fitness"] == rs["fitness"]
        assert r["verified"] == int(bool(r["converged"]) and r["fitness"] <= 0.3)
        q, t = relative_pose_from_icp(r["T"])
        assert np.abs(r["q_rel"] - q).max() <= 1e-6 and np.abs(r["t_rel"] - t).max() <= 1e-6
    vg.close()
    icp.close()


def test_keyframe_mode_equals_per_stage_calls(S, stream, main_run):
    """the serial per-stage HIP calls with the Python gate: the same poses, keyframes and loop answers, bit for bit"""
    from scaloam.pgo import KeyframeGate
    scans = stream[0]
    got = main_run[0]
    cap = max(s.shape[0] for s in scans) + 1024
    reg = S.ScanRegistration(S.OS1_64, 0.5, max_points=cap)
    od = S.LaserOdometry(max_points=cap)
    mp = S.LaserMapping(0.4, 0.8, max_scan_points=cap, max_map_points=2000000)
    sc = S.SCManager(max_radius=80.0, dist_thres=0.2)
    gate = KeyframeGate(GAP_M, GAP_DEG)
    n_kf = 0
    for k, xyz in enumerate(scans):
        reg.laserCloudHandler(xyz)
        _, _, qw, tw, _ = od.step_features(reg)
        qm, tm, _ = mp.process_features(reg, qw, tw)
        g = got[k]
        assert np.array_equal(g["q"], qm) and np.array_equal(g["t"], tm), k
        kf = gate(qm, tm)
        assert g["is_keyframe"] == kf, k
        if kf:
            sc.insert_features(reg)
            n_kf += 1
            if n_kf >= 30:
                r = sc.detectLoopClosureID()
                a = g["loop"]
                assert (a["loop_id"], a["nn_idx"], a["yaw"], a["min_dist"]) == (r["loop_id"], r["nn_idx"], r["yaw"], r["min_dist"]), k
            else:
                assert g["loop"] is None
    for x in (reg, od, mp, sc):
        x.close()


def test_tiny_fitness_threshold_rejects_every_loop(S, stream, main_run):
    p, got, loops = _run(S, stream[0], loop_fitness_thres=1e-30)
    p.close()
    ref = main_run[1]
    assert len(loops) == len(ref) and all(r["verified"] == 0 for r in loops)
    assert [r["fitness"] for r in loops] == [r["fitness"] for r in ref]


def test_prefilled_database(S, O, stream, oracle):
    """pre-filled entries shift keyframe_id; a loop onto one of them cannot be verified (no cloud)"""
    n_pre = 40
    mk = O.SCManager(max_radius=80.0, dist_thres=0.2)
    prefill = [mk.makeScancontext(c) for c in oracle["clouds"][:n_pre]]
    p, got, loops = _run(S, stream[0], prefill=prefill)
    p.close()
    ids = [g["keyframe_id"] for g in got]
    assert ids == [o["kf"] + n_pre if o["is_kf"] else -1 for o in oracle["per"]]
    onto_pre = [r for r in loops if r["loop_kf"] < n_pre]
    onto_own = [r for r in loops if r["loop_kf"] >= n_pre]
    assert onto_pre and all(r["verified"] == -1 and r["iterations"] == 0 and r["n_src"] == 0 for r in onto_pre)
    assert all(r["verified"] in (0, 1) and r["n_src"] > 0 for r in onto_own)


def test_no_cloud_store(S, stream, oracle):
    p, got, loops = _run(S, stream[0], kf_max_points=0)
    det = [g for g in got if g["loop"] is not None and g["loop"]["loop_id"] >= 0]
    assert len(det) >= 3 and len(loops) == len(det)
    assert all(r["verified"] == -1 and r["iterations"] == 0 and r["n_src"] == 0 and r["n_tgt"] == 0 for r in loops)
    pose, cloud = p.keyframe(0)
    assert cloud.shape[0] == 0 and np.array_equal(pose[:3], got[0]["t"])
    p.close()


def test_store_overflow_is_reported(S, stream):
    p = _pipeline(S, stream[0], kf_max_points=60000)
    with pytest.raises(S.ScalError) as e:
        for xyz in stream[0]:
            p.push(xyz)
            while p.in_flight() > 2:
                p.pop()
        p.drain()
    assert e.value.code == S.E_CAPACITY
    p.close()


def test_keyframe_mode_rejects_several_sequences(S):
    with pytest.raises(S.ScalError) as e:
        S.Pipeline(S.OS1_64, 0.5, max_points=100000, sc_mode=S.SC_KEYFRAME, n_seqs=2)
    assert e.value.code == S.E_ARG


def test_loop_queue_limit(S, stream):
    """a search that always answers (SC threshold 100) and nothing popped from the loop queue: push refuses at 64 records and takes
    scans again once they are popped; the pipeline itself never waits for the queue"""
    scans = stream[0] + stream[0]  # back at the start: drive the loop twice
    p = _pipeline(S, scans, kf_max_points=0, sc_dist_thres=100.0)
    refused_at = None
    for k, xyz in enumerate(scans):
        try:
            p.push(xyz)
        except S.ScalError as e:
            assert e.code == S.E_STATE
            refused_at = k
            break
        while p.in_flight() > 2:
            assert p.pop()["seq"] >= 0
    assert refused_at is not None
    p.drain()
    while p.in_flight():
        p.pop()
    n = 0
    while p.pop_loop(wait=False) is not None:
        n += 1
    assert n >= 64
    for xyz in scans[refused_at:refused_at + 3]:
        p.push(xyz)
    p.drain()
    p.close()
