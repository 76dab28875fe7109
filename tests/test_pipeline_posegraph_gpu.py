"""scal_pipeline_optimize_keyframes (sc_mode 3): the pose graph of the pipeline's own keyframes and accepted loops, optimised on the
device, against scaloam.pgo.optimize_pose_graph(build_pipeline_graph(...)); its result fed into the loop verification and the
pose-graph map; its independence of device timing.

The stream is test_pipeline_pgo_map_gpu.py's out-and-back OS1-64 drive (seed 301, gate 0.4 m / 10 deg), built the same way here."""
import ctypes

import numpy as np
import pytest

from scaloam import pgo as G

pytestmark = pytest.mark.gpu

GAP_M, GAP_DEG = 0.4, 10.0
KF_POINTS = 6000000
MAP_POINTS = 6000000
STEPS = [0.5] * 40 + [0.35, 0.2, 0.1, 0.0, -0.1, -0.2, -0.35] + [-0.5] * 42
DELTA = np.array([0.002, -0.001, 0.0, 0.0, 0.0, np.deg2rad(0.02)])   # test_pipeline_pgo_map_gpu.py's stand-in drift per keyframe
REC_KEYS = ("seq", "curr_kf", "loop_kf", "verified", "converged", "iterations", "state", "fitness", "n_src", "n_tgt")
POSE_BAR = 1e-5


@pytest.fixture(scope="module")
def stream(worlds, O):
    w = worlds(O.OS1_64, 301)
    q0, t0 = w.pose(0)
    _, t1 = w.pose(10)
    d = t1 - t0
    d[2] = 0
    d /= np.linalg.norm(d)
    x = np.concatenate([[0.0], np.cumsum(STEPS)])
    return [w.scan_pose(q0, t0 + d * xi, 1000 + k) for k, xi in enumerate(x)]


def _pipeline(S, scans, ring=6, depth=2, kf_max_points=KF_POINTS, pgo_map_max_points=MAP_POINTS, sc_mode=None):
    cap = max(s.shape[0] for s in scans) + 1024
    return S.Pipeline(S.OS1_64, 0.5, max_points=cap, line_res=0.4, plane_res=0.8, max_map_points=2000000,
                      sc_mode=S.SC_KEYFRAME if sc_mode is None else sc_mode, sc_max_radius=80.0, sc_dist_thres=0.2, sc_max_keyframes=512,
                      ring=ring, depth=depth, keyframe_meter_gap=GAP_M, keyframe_deg_gap=GAP_DEG, kf_max_points=kf_max_points,
                      pgo_map_max_points=pgo_map_max_points)


def _run(S, scans, M=None, at_M=None, ahead=4, on_pop=None, keep=False, **kw):
    """push every scan; with M: drain and pop everything right before scan M is pushed, then at_M(p, got)"""
    p = _pipeline(S, scans, **kw)
    got, extra = [], None

    def take():
        got.append(p.pop())
        if on_pop:
            on_pop(p, got[-1])

    for k, xyz in enumerate(scans):
        if k == M:
            p.drain()
            while p.in_flight():
                take()
            extra = at_M(p, got)
        p.push(xyz)
        while p.in_flight() > ahead:
            take()
    p.drain()
    while p.in_flight():
        take()
    loops = []
    while True:
        r = p.pop_loop(wait=True)
        if r is None:
            break
        loops.append(r)
    kfs = [p.keyframe(g["keyframe_id"]) for g in got if g["is_keyframe"]]
    if not keep:
        p.close()
        p = None
    return p, got, loops, kfs, extra


def _same_record(a, b):
    return (all(a[k] == b[k] for k in REC_KEYS) and np.array_equal(a["T"], b["T"]) and np.array_equal(a["q_rel"], b["q_rel"])
            and np.array_equal(a["t_rel"], b["t_rel"]))


def _same_poses(ga, gb):
    return len(ga) == len(gb) and all(np.array_equal(a["q"], b["q"]) and np.array_equal(a["t"], b["t"]) and a["keyframe_id"] == b["keyframe_id"]
                                      for a, b in zip(ga, gb))


def _pose_diff(a6, b6):
    a, b = G.pose7_from_pose6(a6), G.pose7_from_pose6(b6)
    d = G.se3_log(G.se3_between(a, b))
    return max(np.abs(a[:, 4:] - b[:, 4:]).max(), np.abs(d[:, :3]).max())


def _restatement(kfs, loops, kf_end):
    gated = np.array([pose for pose, _ in kfs[:kf_end]])
    prior, edges = G.build_pipeline_graph(gated, [r for r in loops if r["curr_kf"] < kf_end])
    x, st = G.optimize_pose_graph(G.pose7_from_pose6(gated), prior, edges)
    return gated, edges, G.pose6_from_pose7(x), st


@pytest.fixture(scope="module")
def base(S, stream):
    """a pipeline that never makes the call, drained at the end; then the drained results of the call for several kf_end.  This
    drive's loops are accepted ones (asserted here), so the 280-scan drive of tools/bench_keyframe_stream.py is not needed."""
    p, got, loops, kfs, _ = _run(S, stream, keep=True)
    n_kf = len(kfs)
    acc = sorted(r["curr_kf"] for r in loops if r["verified"] == 1)
    assert n_kf >= 62 and len(loops) >= 3 and len(acc) >= 1, "the drive yields no accepted loop"
    seqs = sorted(r["seq"] for r in loops)
    M = seqs[len(seqs) // 2]
    ends = sorted({acc[0] + 1, acc[len(acc) // 2] + 1, n_kf - 3, n_kf})
    drained = {e: p.optimize_keyframes(kf_end=e, apply=False) for e in ends}
    again = p.optimize_keyframes(kf_end=n_kf, apply=False)
    p.close()
    return dict(got=got, loops=loops, kfs=kfs, M=M, n_kf=n_kf, acc=acc, ends=ends, drained=drained, again=again)


def test_drained_against_the_restatement(S, base):
    for e in base["ends"]:
        ids, poses, st = base["drained"][e]
        gated, edges, ref, rs = _restatement(base["kfs"], base["loops"], e)
        n_loops = int((edges["k"] > 0).sum())
        dp = _pose_diff(ref, poses)
        print("kf_end", e, "loops", n_loops, "pose diff", dp, "moved by", _pose_diff(gated, poses), "cost", st["initial_cost"], "->", st["final_cost"],
              "restatement", rs["costs"][0], "->", rs["final_cost"], "iterations", st["iterations"], rs["iterations"], "linear", st["linear_iterations"])
        assert ids.tolist() == list(range(e)) and st["n_nodes"] == e and st["n_odom_edges"] == e - 1 and st["n_loop_edges"] == n_loops
        assert n_loops >= 1 and st["applied"] == 0
        assert st["converged"] == 1 and rs["converged"] == 1
        assert dp <= POSE_BAR
        assert st["final_cost"] < st["initial_cost"] and _pose_diff(gated, poses) > 1e-6, "the loop edges moved nothing"
        assert abs(st["final_cost"] - rs["final_cost"]) <= max(1e-9 * rs["final_cost"], 1e-12)
    # bit for bit the same when asked again
    a, b = base["drained"][base["n_kf"]], base["again"]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_never_called_changes_nothing(S, stream, base):
    """no map buffers, no call (nothing of the optimizer is ever created): the stream's results are those of the fixture's pipeline, which
    made its calls only after the last scan"""
    _, got, loops, _, _ = _run(S, stream, pgo_map_max_points=0)
    assert _same_poses(got, base["got"])
    assert len(loops) == len(base["loops"]) and all(_same_record(a, b) for a, b in zip(loops, base["loops"]))


def test_apply_reaches_map_and_verification(S, O, stream, base):
    """apply=True right before scan M: the pose-graph map and the loops of scans pushed afterwards use the returned poses (the checks
    test_pipeline_pgo_map_gpu.py makes for caller-supplied poses); keyframe() still returns the gated pose.
    On an out-and-back drive the root keyframe of every later loop lies before all keyframes the earlier loops can move, so the optimum
    leaves those roots where the gate put them and by itself changes no later record.  To give the check something to find, the caller
    first updates every popped keyframe to that file's drifting stand-in estimate (which does change later records, as that file
    asserts): the call then starts from those poses (the current ones), must come back to the optimum, and its apply must replace
    them - the later records must follow the RETURNED root poses and differ from a run that only made the stand-in update."""
    from scaloam.pgo import local2global_f32, pgo_map_cloud, relative_pose_from_icp, rpy_from_quat
    M = base["M"]

    def drift(p, got):
        kf = [g for g in got if g["is_keyframe"]]
        p.update_keyframe_poses([g["keyframe_id"] for g in kf],
                                [np.concatenate([g["t"], rpy_from_quat(g["q"])]) + g["keyframe_id"] * DELTA for g in kf])

    _, _, loops_drift, _, _ = _run(S, stream, M=M, at_M=drift)

    def at_M(p, got):
        n_before = sum(g["is_keyframe"] for g in got)
        drift(p, got)
        ids, poses, st = p.optimize_keyframes(apply=True)   # kf_end = the keyframes popped so far
        assert ids.tolist() == list(range(n_before)) and st["applied"] == 1 and st["n_loop_edges"] >= 1
        m = p.pgo_map(skip=2, leaf=0.4)
        return dict(ids=ids, poses=poses, st=st, map=m)

    p, got, loops, kfs, x = _run(S, stream, M=M, at_M=at_M, keep=True)
    upd = {int(i): x["poses"][k] for k, i in enumerate(x["ids"])}
    n_upd = len(upd)
    # the same as the drained call with that kf_end made after the last scan (the graph holds only loops with curr_kf < kf_end)
    _, _, ref, _ = _restatement(base["kfs"], base["loops"], n_upd)
    assert _pose_diff(ref, x["poses"]) <= POSE_BAR
    assert _same_poses(got, base["got"])
    for (pose, cloud), (pose_b, cloud_b) in zip(kfs, base["kfs"]):
        assert np.array_equal(pose, pose_b) and np.array_equal(cloud.view(np.uint32), cloud_b.view(np.uint32))   # keyframe(): the gated pose
    # the map built right after the call, and one over all keyframes at the end: optimized poses where there are any, gated ones behind
    clouds = [c for _, c in kfs]
    for kf_end, m in ((n_upd, x["map"]), (len(kfs), p.pgo_map(kf_end=len(kfs), skip=2, leaf=0.4))):
        poses = [upd.get(i, kfs[i][0]) for i in range(len(kfs))]
        ref_map, guard = O.voxel_grid(pgo_map_cloud(clouds, poses, kf_end, 2), 0.4)
        assert guard == 0 and m.shape == ref_map.shape and np.array_equal(m.view(np.uint32), ref_map.view(np.uint32)), kf_end
    p.close()
    # loop records: before M unchanged, after M the numpy chain with the RETURNED root pose
    ref_loops = base["loops"]
    assert [(r["seq"], r["curr_kf"], r["loop_kf"]) for r in loops] == [(r["seq"], r["curr_kf"], r["loop_kf"]) for r in ref_loops]
    vg = S.VoxelGrid(max_points=4000000)
    icp = S.LoopICP(max_source=400000, max_target=4000000)
    n_oracle, n_changed, n_after = 0, 0, 0
    assert len(loops_drift) == len(loops)
    for r, b, f in zip(loops, ref_loops, loops_drift):
        if r["seq"] < M:
            assert _same_record(r, b), r["seq"]
            continue
        n_after += 1
        n_changed += not _same_record(r, f)
        c, l = r["curr_kf"], r["loop_kf"]
        assert l in upd
        root = upd[l]
        src = local2global_f32(kfs[c][1], root)
        tgt = np.concatenate([local2global_f32(kfs[j][1], root) for j in range(max(0, l - 25), min(l + 25, c) + 1)])
        so, to = O.voxel_grid(src, 0.4)[0], O.voxel_grid(tgt, 0.4)[0]
        assert (r["n_src"], r["n_tgt"]) == (so.shape[0], to.shape[0]), r["seq"]
        if n_oracle < 1:
            n_oracle += 1
            ro = O.icp_align(so, to)
            assert (r["converged"], r["state"], r["iterations"]) == (int(ro["converged"]), ro["state"], ro["iterations"]), r["seq"]
            assert np.abs(r["T"] - ro["T"]).max() <= 1e-9
            assert abs(r["fitness"] - ro["fitness"]) <= 1e-9 * max(1.0, ro["fitness"])
        else:
            rs = icp.align(vg.filter(src, 0.4), vg.filter(tgt, 0.4))
            assert (r["converged"], r["state"], r["iterations"]) == (int(rs["converged"]), rs["state"], rs["iterations"]), r["seq"]
            assert np.array_equal(r["T"], rs["T"]) and r["fitness"] == rs["fitness"]
        assert r["verified"] == int(bool(r["converged"]) and r["fitness"] <= 0.3)
        q, t = relative_pose_from_icp(r["T"])
        assert np.abs(r["q_rel"] - q).max() <= 1e-6 and np.abs(r["t_rel"] - t).max() <= 1e-6
    vg.close()
    icp.close()
    assert n_after >= 1 and n_changed >= 1, "the applied poses changed no loop record against the stand-in update alone"


@pytest.mark.parametrize("ring,ahead,depth", [(6, 4, 2), (6, 0, 2), (4, 4, 3)])
def test_in_flight_is_deterministic(S, stream, base, ring, ahead, depth):
    """the call between pops, scans in flight, kf_end = the keyframes popped so far (the newest one's loop may still be in verification:
    the call waits for it): ids and poses bit-identical to the drained call with the same kf_end; with apply=False every popped pose
    and every loop record of the stream is bit-identical to the run that never makes the call"""
    calls = {}
    want = set(base["ends"])

    def on_pop(p, r):
        if r["is_keyframe"] and r["keyframe_id"] + 1 in want:
            calls[r["keyframe_id"] + 1] = p.optimize_keyframes(apply=False)

    _, got, loops, _, _ = _run(S, stream, ahead=ahead, on_pop=on_pop, ring=ring, depth=depth)
    assert sorted(calls) == base["ends"]
    for e, (ids, poses, st) in calls.items():
        d = base["drained"][e]
        assert np.array_equal(ids, d[0]) and np.array_equal(poses, d[1]) and st == d[2], e
    assert _same_poses(got, base["got"])
    assert len(loops) == len(base["loops"]) and all(_same_record(a, b) for a, b in zip(loops, base["loops"]))


def test_errors(S, stream):
    L = S.lib()
    scans = stream[:8]
    p = _pipeline(S, scans, pgo_map_max_points=0)
    res = S.PipelinePgoResult()
    i32p, f64p = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    ids, P = np.zeros(64, np.int32), np.zeros((64, 6))

    def call(kf_end, cap, apply=0):
        return L.scal_pipeline_optimize_keyframes(p.h, kf_end, apply, ids.ctypes.data_as(i32p), P.ctypes.data_as(f64p), cap, ctypes.byref(res))

    assert call(0, 64) == S.OK and res.n_nodes == 0        # nothing pushed yet: an empty graph
    assert call(1, 64) == S.E_STATE
    got = []
    for xyz in scans:
        p.push(xyz)
        while p.in_flight() > 2:
            got.append(p.pop())
    p.drain()
    while p.in_flight():
        got.append(p.pop())
    kf = [g["keyframe_id"] for g in got if g["is_keyframe"]]
    n = len(kf)
    assert n >= 4 and kf == list(range(n))
    assert call(n + 1, 64) == S.E_STATE                    # beyond the confirmed keyframes
    assert call(-1, 64) == S.E_ARG
    assert call(n, n - 1) == S.E_CAPACITY and res.n_nodes == n
    assert L.scal_pipeline_optimize_keyframes(p.h, n, 0, None, None, 0, ctypes.byref(res)) == S.E_CAPACITY and res.n_nodes == n
    assert L.scal_pipeline_optimize_keyframes(p.h, n, 0, None, None, 4, None) == S.E_ARG
    # no loops: the gated poses come back (within the step tolerance), nothing applied
    assert call(n, 64) == S.OK and res.n_nodes == n and res.n_odom_edges == n - 1 and res.n_loop_edges == 0 and res.applied == 0
    assert res.solver.converged == 1 and res.solver.iterations <= 1
    gated = np.array([p.keyframe(i)[0] for i in kf])
    assert ids[:n].tolist() == kf and _pose_diff(gated, P[:n]) <= 1e-8
    i2, p2, st = p.optimize_keyframes()                    # kf_end = popped so far, apply
    assert i2.tolist() == kf and st["applied"] == 1 and np.array_equal(p2, P[:n])
    p.close()
    for mode in (S.SC_OFF, S.SC_EVERY_SCAN):
        p = _pipeline(S, scans, sc_mode=mode, kf_max_points=0, pgo_map_max_points=0)
        assert L.scal_pipeline_optimize_keyframes(p.h, 0, 0, None, None, 0, ctypes.byref(res)) == S.E_STATE
        with pytest.raises(S.ScalError) as e:
            p.optimize_keyframes(kf_end=0)
        assert e.value.code == S.E_STATE
        p.close()
