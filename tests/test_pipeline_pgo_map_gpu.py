"""scal_pipeline sc_mode 3: the caller's optimized keyframe poses in (updatePoses, laserPosegraphOptimization.cpp:408-431), the pose-graph
map out (pubMap, :810-834).

The stream is test_pipeline_keyframes_gpu.py's out-and-back OS1-64 drive (seed 301, gate 0.4 m / 10 deg), whose stored keyframe clouds
that file holds to the oracle.  As a stand-in for an iSAM2 estimate, own keyframe j is updated to its gated pose6 + j * (2 mm, -1 mm,
0, 0, 0, 0.02 deg): enough to change the rebuilt submaps and the ICP results."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GAP_M, GAP_DEG = 0.4, 10.0
KF_POINTS = 6000000
MAP_POINTS = 6000000
STEPS = [0.5] * 40 + [0.35, 0.2, 0.1, 0.0, -0.1, -0.2, -0.35] + [-0.5] * 42
DELTA = np.array([0.002, -0.001, 0.0, 0.0, 0.0, np.deg2rad(0.02)])
REC_KEYS = ("seq", "curr_kf", "loop_kf", "verified", "converged", "iterations", "state", "fitness", "n_src", "n_tgt")


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


def _pipeline(S, scans, ring=6, depth=2, kf_max_points=KF_POINTS, pgo_map_max_points=MAP_POINTS, prefill=(), sc_mode=None):
    cap = max(s.shape[0] for s in scans) + 1024
    p = S.Pipeline(S.OS1_64, 0.5, max_points=cap, line_res=0.4, plane_res=0.8, max_map_points=2000000,
                   sc_mode=S.SC_KEYFRAME if sc_mode is None else sc_mode, sc_max_radius=80.0, sc_dist_thres=0.2, sc_max_keyframes=512,
                   ring=ring, depth=depth, keyframe_meter_gap=GAP_M, keyframe_deg_gap=GAP_DEG, kf_max_points=kf_max_points,
                   pgo_map_max_points=pgo_map_max_points)
    for d in prefill:
        p.sc.saveScancontextAndKeys(d)
    return p


def _estimate(g, n_pre=0):
    """the stand-in estimate of the keyframe of popped result g"""
    from scaloam.pgo import rpy_from_quat
    return np.concatenate([g["t"], rpy_from_quat(g["q"])]) + (g["keyframe_id"] - n_pre) * DELTA


def _update_popped(p, got):
    """update every keyframe popped so far; {id: pose6}"""
    upd = {g["keyframe_id"]: _estimate(g) for g in got if g["is_keyframe"]}
    ids = sorted(upd)
    p.update_keyframe_poses(ids, [upd[i] for i in ids])
    return upd


def _run(S, scans, M=None, drain_at_M=True, ahead=4, on_pop=None, **kw):
    """push every scan; with M: update the keyframes popped so far right before scan M is pushed (after a drain with drain_at_M)"""
    p = _pipeline(S, scans, **kw)
    got, upd = [], None

    def take():
        got.append(p.pop())
        if on_pop:
            on_pop(p, got[-1], upd)

    for k, xyz in enumerate(scans):
        if k == M:
            if drain_at_M:
                p.drain()
                while p.in_flight():
                    take()
            upd = _update_popped(p, got)
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
    return p, got, loops, upd, kfs


def _same_record(a, b):
    return (all(a[k] == b[k] for k in REC_KEYS) and np.array_equal(a["T"], b["T"]) and np.array_equal(a["q_rel"], b["q_rel"])
            and np.array_equal(a["t_rel"], b["t_rel"]))


def _same_poses(ga, gb):
    return all(np.array_equal(a["q"], b["q"]) and np.array_equal(a["t"], b["t"]) and a["keyframe_id"] == b["keyframe_id"] for a, b in zip(ga, gb))


def _download(ptr, n):
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    out = np.zeros((n, 4), np.float32)
    if n:
        assert hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0
    return out


def _expected_map(O, kfs, poses, kf_end, skip, leaf):
    from scaloam.pgo import pgo_map_cloud
    cloud = pgo_map_cloud([c for _, c in kfs], poses, kf_end, skip)
    ref, guard = O.voxel_grid(cloud, leaf)
    return cloud, ref, guard


@pytest.fixture(scope="module")
def base(S, stream):
    """no map buffers, no update"""
    p, got, loops, _, kfs = _run(S, stream, pgo_map_max_points=0)
    p.close()
    n_kf = sum(g["is_keyframe"] for g in got)
    seqs = sorted(r["seq"] for r in loops)
    assert n_kf >= 62 and len(seqs) >= 3
    M = seqs[len(seqs) // 2]  # after the first detected loops, before the last
    assert seqs[0] < M <= seqs[-1]
    return dict(got=got, loops=loops, kfs=kfs, M=M)


@pytest.fixture(scope="module")
def run_a(S, stream, base):
    """drain after scan M - 1, update every own keyframe, push the rest"""
    p, got, loops, upd, kfs = _run(S, stream, M=base["M"])
    p.close()
    assert len(upd) == sum(g["is_keyframe"] for g in got if g["seq"] < base["M"])
    return dict(got=got, loops=loops, upd=upd, kfs=kfs)


def test_map_buffers_change_nothing(S, stream, base):
    """pgo_map_max_points > 0 and no update: poses, keyframes and loop records bit-identical to a pipeline without map buffers"""
    p, got, loops, _, _ = _run(S, stream)
    p.close()
    assert _same_poses(got, base["got"])
    assert len(loops) == len(base["loops"]) and all(_same_record(a, b) for a, b in zip(loops, base["loops"]))


def test_map_parity_and_pcl_guard(S, O, stream, base):
    p, got, _, _, kfs = _run(S, stream)
    n_kf = len(kfs)
    poses = [pose for pose, _ in kfs]  # the gated poses (keyframePosesUpdated's start, :636)
    cases = [(2, 0.8, False), (2, 0.4, True), (1, 0.4, True), (3, 0.2, True)]
    updated = False
    for skip, leaf, upd in cases:
        if upd and not updated:
            est = _update_popped(p, got)
            poses = [est[i] for i in range(n_kf)]
            updated = True
        for kf_end in (n_kf, n_kf // 2 + 1):
            _, ref, guard = _expected_map(O, kfs, poses, kf_end, skip, leaf)
            assert guard == 0
            m = p.pgo_map(kf_end=kf_end, skip=skip, leaf=leaf)
            assert m.shape == ref.shape and np.array_equal(m.view(np.uint32), ref.view(np.uint32)), (skip, leaf, upd, kf_end)
            ptr, n = p.pgo_map_device()
            assert n == m.shape[0] and np.array_equal(_download(ptr, n).view(np.uint32), m.view(np.uint32))
    # kf_end=None: 1 + the largest keyframe_id popped
    assert np.array_equal(p.pgo_map(skip=2, leaf=0.4).view(np.uint32), _expected_map(O, kfs, poses, n_kf, 2, 0.4)[1].view(np.uint32))
    # PCL's "leaf size too small" guard: the output is the concatenated input
    cloud, ref, guard = _expected_map(O, kfs, poses, n_kf, 2, 0.005)
    assert guard == 1 and np.array_equal(ref.view(np.uint32), cloud.view(np.uint32))
    m = p.pgo_map(kf_end=n_kf, skip=2, leaf=0.005)
    assert np.array_equal(m.view(np.uint32), cloud.view(np.uint32))
    p.close()


def test_updates_reach_verification(S, O, base, run_a):
    """loops of scans pushed after the update: the chain rebuilt in numpy with the UPDATED loop keyframe pose; before: unchanged"""
    from scaloam.pgo import local2global_f32, relative_pose_from_icp
    M, upd, kfs = base["M"], run_a["upd"], run_a["kfs"]
    assert _same_poses(run_a["got"], base["got"])
    ref = base["loops"]
    assert [(r["seq"], r["curr_kf"], r["loop_kf"]) for r in run_a["loops"]] == [(r["seq"], r["curr_kf"], r["loop_kf"]) for r in ref]
    vg = S.VoxelGrid(max_points=4000000)
    icp = S.LoopICP(max_source=400000, max_target=4000000)
    n_oracle, n_changed, n_after = 0, 0, 0
    for r, b in zip(run_a["loops"], ref):
        if r["seq"] < M:
            assert _same_record(r, b), r["seq"]
            continue
        n_after += 1
        n_changed += not _same_record(r, b)
        c, l = r["curr_kf"], r["loop_kf"]
        root = upd[l]
        src = local2global_f32(kfs[c][1], root)
        tgt = np.concatenate([local2global_f32(kfs[j][1], root) for j in range(max(0, l - 25), min(l + 25, c) + 1)])
        so, to = O.voxel_grid(src, 0.4)[0], O.voxel_grid(tgt, 0.4)[0]
        assert (r["n_src"], r["n_tgt"]) == (so.shape[0], to.shape[0]), r["seq"]
        if n_oracle < 2:
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
    assert n_after >= 1 and n_changed >= 1, "the update changed no loop record"


@pytest.mark.parametrize("ring,ahead,depth", [(6, 4, 2), (6, 0, 2), (4, 4, 3)])
def test_update_in_flight_is_deterministic(S, O, stream, base, run_a, ring, ahead, depth):
    """the update right after the push of scan M - 1 returns, without a drain: the same loop records as run A.  In the first schedule
    pgo_map runs with scans in flight, after the pops of two keyframes (one before the update, one after): each map is the drained
    computation with the poses of that moment, and the stream is not disturbed."""
    maps = []
    K = (10, len(base["kfs"]) - 3)

    def on_pop(p, r, upd):
        if ahead == 4 and ring == 6 and r["is_keyframe"] and r["keyframe_id"] in K:
            maps.append((r["keyframe_id"], None if upd is None else dict(upd), p.pgo_map(kf_end=r["keyframe_id"] + 1)))

    p, got, loops, upd, kfs = _run(S, stream, M=base["M"], drain_at_M=False, ahead=ahead, on_pop=on_pop, ring=ring, depth=depth)
    p.close()
    M = base["M"]
    assert _same_poses(got, run_a["got"])
    # only the root (loop) keyframe's pose moves the verification's clouds: every root after M is among the keyframes updated here
    assert all(r["loop_kf"] in upd for r in run_a["loops"] if r["seq"] >= M)
    assert len(loops) == len(run_a["loops"]) and all(_same_record(a, b) for a, b in zip(loops, run_a["loops"]))
    if ahead == 4 and ring == 6:
        assert [k for k, _, _ in maps] == list(K) and maps[0][1] is None and maps[1][1] is not None
        for k, u, m in maps:
            poses = [(u or {}).get(i, kfs[i][0]) for i in range(len(kfs))]
            _, ref, guard = _expected_map(O, kfs, poses, k + 1, 2, 0.4)
            assert guard == 0 and np.array_equal(m.view(np.uint32), ref.view(np.uint32)), k


def _raw_map(S, p, kf_end, skip, leaf, buf=None):
    n = ctypes.c_longlong(-1)
    ptr = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if buf is not None else None
    rc = S.lib().scal_pipeline_pgo_map(p.h, kf_end, skip, leaf, ptr, 0 if buf is None else buf.shape[0], ctypes.byref(n))
    return rc, n.value


def test_errors(S, O, stream, base):
    scans = stream[:8]
    n_pre = 2
    mk = O.SCManager(max_radius=80.0, dist_thres=0.2)
    clouds = [c for _, c in base["kfs"]]
    small = clouds[0].shape[0] + clouds[1].shape[0]
    p = _pipeline(S, scans, prefill=[mk.makeScancontext(c) for c in clouds[:n_pre]], pgo_map_max_points=small)
    assert p.pgo_map_device() == (None, 0)
    got = []
    for xyz in scans:
        p.push(xyz)
        while p.in_flight() > 2:
            got.append(p.pop())
    p.drain()
    while p.in_flight():
        got.append(p.pop())
    ids = [g["keyframe_id"] for g in got if g["is_keyframe"]]
    assert ids[0] == n_pre and len(ids) >= 4
    m0 = p.pgo_map(kf_end=n_pre + 2, skip=1)
    assert m0.shape[0] > 5
    good = _estimate(got[0], n_pre) + DELTA
    bad_pose = good.copy()
    bad_pose[2] = np.nan
    for bad_ids, bad_poses in (([n_pre, 0], [good, good]), ([n_pre, 10 ** 6], [good, good]), ([n_pre, n_pre + 1], [good, bad_pose]),
                               ([-1], [good])):
        with pytest.raises(S.ScalError) as e:
            p.update_keyframe_poses(bad_ids, bad_poses)
        assert e.value.code == S.E_ARG
    assert np.array_equal(p.pgo_map(kf_end=n_pre + 2, skip=1).view(np.uint32), m0.view(np.uint32)), "a refused update changed the map"
    # kf_end beyond the confirmed keyframes
    assert _raw_map(S, p, ids[-1] + 2, 1, 0.4)[0] == S.E_STATE
    # more selected points than pgo_map_max_points: nothing runs, n_out = the points needed
    need = sum(c.shape[0] for c in (p.keyframe(i)[1] for i in ids))
    assert need > small
    assert _raw_map(S, p, ids[-1] + 1, 1, 0.4) == (S.E_CAPACITY, need)
    for leaf, skip in ((0.0, 1), (-0.4, 1), (float("nan"), 1), (float("inf"), 1), (0.4, 0)):
        assert _raw_map(S, p, n_pre + 2, skip, leaf)[0] == S.E_ARG, (leaf, skip)
    # cap below the result: cap records written, the full count reported
    buf = np.full((5, 4), -7.0, np.float32)
    assert _raw_map(S, p, n_pre + 2, 1, 0.4, buf) == (S.OK, m0.shape[0])
    assert np.array_equal(buf.view(np.uint32), m0[:5].view(np.uint32))
    p.close()
    for kw in (dict(sc_mode=S.SC_EVERY_SCAN), dict(kf_max_points=0), dict(pgo_map_max_points=-1)):
        kw.setdefault("pgo_map_max_points", 1000)
        with pytest.raises(S.ScalError) as e:
            _pipeline(S, scans, **kw)
        assert e.value.code == S.E_ARG, kw
    p = _pipeline(S, scans, pgo_map_max_points=0)
    assert _raw_map(S, p, 0, 2, 0.4)[0] == S.E_STATE and p.pgo_map_device() == (None, 0)
    p.close()
    p = _pipeline(S, scans, sc_mode=S.SC_OFF, kf_max_points=0, pgo_map_max_points=0)
    with pytest.raises(S.ScalError) as e:
        p.update_keyframe_poses([0], [np.zeros(6)])
    assert e.value.code == S.E_STATE
    p.close()
