"""Multiview refine (scal_refine_*, csrc/refine.hip): all keyframes aligned at once, each against the points of all the others.

The yardsticks are the single alignment the batched path restates (S.LoopICP on the concatenation of the other frames, bit for bit:
same nearest neighbours, same order of every f64 addition, same host iteration) and the oracle's pcl::IterativeClosestPoint
(O.icp_align) on clouds the oracle's map merge moved.  Frames are the golden KAIST03 keyframes 0 / 7 / 20 thinned at 0.4 m."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IDENT12 = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)


@pytest.fixture(scope="module")
def kf(S, golden):
    """the three thinned keyframes (local frames) and their golden poses"""
    vg = S.VoxelGrid()
    frames = [vg.filter(golden(f"KAIST03_{i:06d}.npy"), 0.4) for i in (0, 7, 20)]
    vg.close()
    poses = golden("KAIST03_poses21.npy").reshape(-1, 12)[[0, 7, 20]].astype(np.float64)
    assert all(14000 < f.shape[0] < 16000 for f in frames)
    return frames, poses


@pytest.fixture(scope="module")
def moved(S):
    """G_f: one frame through the map merge"""
    mm = S.MapMerge(max_points=100000, max_frame_points=100000)

    def run(frame, pose12, near=2.0):
        mm.reset()
        mm.add(frame, pose12, near)
        return mm.download().copy()
    yield run
    mm.close()


def _same(r, s):
    return (np.array_equal(r["T"], s["T"]) and r["iterations"] == s["iterations"] and r["state"] == s["state"]
            and r["n_correspondences"] == s["n_correspondences"] and r["converged"] == s["converged"])


def _vs_single(S, moved, frames, poses, fixed=None, cap=150.0, iters=20, near=2.0, fitness=True):
    """one round of the refine; every non-fixed frame must equal the single alignment against the other frames' moved points"""
    n = sum(f.shape[0] for f in frames)
    rf = S.MultiviewRefine(len(frames), max(n, 1), max_corr_dist=cap, max_iterations=iters)
    icp = S.LoopICP(max_source=max(n, 1), max_target=max(n, 1), max_corr_dist=cap, max_iterations=iters)
    P, res, run = rf.refine(frames, poses, fixed=fixed, rounds=1, near_thres=near)
    G = [moved(f, p, near) for f, p in zip(frames, poses)]
    assert run == 1
    for f in range(len(frames)):
        if fixed is not None and fixed[f]:
            assert res[f]["state"] == 0 and not res[f]["accepted"] and np.array_equal(P[f], np.asarray(poses[f]).reshape(12))
            continue
        others = [G[g] for g in range(len(frames)) if g != f]
        s = icp.align(G[f], np.concatenate(others) if others else np.zeros((0, 4), np.float32))
        assert _same(res[f], s), (f, res[f], s)
        if fitness and s["n_correspondences"] >= 3:
            assert res[f]["fitness"] == s["fitness"], (f, res[f]["fitness"], s["fitness"])
    rf.close(), icp.close()
    return P, res, G


@pytest.fixture(scope="module")
def six(S, moved, kf):
    """cases 1 and 2 share this call: the three keyframes, a frame of exactly 256 points far from everything, one of 2 points, an empty one"""
    frames, poses = kf
    far_pose = IDENT12.copy()
    far_pose[3] = 1000.0
    fr = list(frames) + [frames[0][:256], frames[1][100:102], np.zeros((0, 4), np.float32)]
    assert np.all(np.linalg.norm(fr[3][:, :3], axis=1) > 2.0) and np.all(np.linalg.norm(fr[4][:, :3], axis=1) > 2.0)
    ps = np.concatenate([poses, far_pose[None], poses[1][None], IDENT12[None]])
    P, res, G = _vs_single(S, moved, fr, ps, cap=150.0, iters=20)
    return fr, ps, P, res, G


def test_refine_equals_single_alignments_bit_for_bit(six):
    """rounds=1, cap 150, 20 iterations, nothing fixed: T, iterations, state, correspondences and (every point has a neighbour within
    150 m) fitness of every frame equal S.LoopICP.align(G_f, concat(G_g, g != f)) - asserted in the shared call.  The 256-point frame
    (one whole workgroup, 1 km away: no correspondence), the 2-point frame and the empty frame end in state 5 with their pose kept."""
    fr, ps, P, res, G = six
    assert G[3].shape[0] == 256 and G[4].shape[0] == 2
    for f in (0, 1, 2):
        assert res[f]["iterations"] >= 1 and res[f]["n_correspondences"] > 10000
    for f in (3, 4, 5):
        assert res[f]["state"] == 5 and not res[f]["converged"] and not res[f]["accepted"]
        assert np.array_equal(P[f], ps[f]) and np.array_equal(res[f]["T"], np.eye(4))


def test_refine_matches_oracle(O, six):
    fr, ps, P, res, G = six
    Go = [O.mapmerge([f], [p]) for f, p in zip(fr, ps)]
    for f in (0, 1, 2):
        ro = O.icp_align(Go[f], np.concatenate([Go[g] for g in range(6) if g != f]), max_iter=20)
        assert res[f]["state"] == ro["state"] and res[f]["iterations"] == ro["iterations"] and res[f]["converged"] == ro["converged"]
        assert np.abs(res[f]["T"] - ro["T"]).max() <= 1e-9, (f, res[f]["T"], ro["T"])


def _case3(S, rf, a):
    th = 0.04
    R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    t = np.array([0.4, -0.25, 0.05])
    src = a.copy()
    src[:, :3] = (a[:, :3].astype(np.float64) @ R.T + t).astype(np.float32)
    poses = np.stack([IDENT12, IDENT12])
    P, res, run = rf.refine([a, src], poses, fixed=[1, 0], rounds=1, near_thres=0.0)
    Ti = np.eye(4)
    Ti[:3, :3], Ti[:3, 3] = R.T, -R.T @ t
    T = res[1]["T"]
    assert res[1]["converged"] and res[1]["accepted"] and run == 1
    assert np.abs(T - Ti).max() <= 1e-5, T   # a frame allowed to match itself would come back with the identity
    Pin = IDENT12.reshape(3, 4)
    want = np.zeros((3, 4))
    for r in range(3):
        for c in range(4):
            v = (T[r, 0] * Pin[0, c] + T[r, 1] * Pin[1, c]) + T[r, 2] * Pin[2, c]
            want[r, c] = v + T[r, 3] if c == 3 else v
    assert np.array_equal(P[1], want.reshape(12))
    assert np.array_equal(P[0], IDENT12) and not res[0]["accepted"] and res[0]["state"] == 0


def test_refine_never_matches_a_frame_against_itself(S, kf):
    a = kf[0][0]
    rf = S.MultiviewRefine(2, 2 * a.shape[0], max_corr_dist=150.0)
    _case3(S, rf, a)
    rf.close()


def test_refine_ties_far_path_and_odd_points(S, moved, kf):
    frames, poses = kf
    # two frames that are copies of each other: equal distances resolve to the lower frame, as on the concatenation
    _vs_single(S, moved, [frames[0], frames[0].copy(), frames[1]], poses[[0, 0, 1]], fixed=[1, 1, 0])
    # 30 m off: most queries are unsettled by the rings in the first iterations and go through the dense list
    off = poses[1].copy()
    off[3] += 30.0
    _, res, _ = _vs_single(S, moved, [frames[0], frames[1]], np.stack([poses[0], off]), fixed=[1, 0])
    assert res[1]["iterations"] >= 2
    # a target with a non-finite point and a far outlier
    odd = np.concatenate([frames[0], np.array([[5000.0, -3000.0, 40.0, 0.0], [np.inf, 1.0, 2.0, 0.0]], np.float32)]).astype(np.float32)
    _vs_single(S, moved, [odd, frames[1], frames[2]], poses, fixed=[1, 0, 0])


@pytest.mark.parametrize("cap", [2.0, 150.0])
def test_refine_extent_beyond_a_dense_grid(S, moved, kf, cap):
    """one pair at the origin, the same pair 5 km away: the map spans far more than 2^18 one-metre cells"""
    frames, poses = kf
    a, b = frames[0][::8], frames[1][::8]
    sh = np.zeros(12)
    sh[[3, 7, 11]] = (4000.0, 3000.0, 20.0)
    ps = np.stack([poses[0], poses[1], poses[0] + sh, poses[1] + sh])
    P, res, G = _vs_single(S, moved, [a, b, a, b], ps, cap=cap, fitness=cap > 100)
    lo, hi = np.concatenate(G)[:, :3].min(0), np.concatenate(G)[:, :3].max(0)
    assert np.prod(np.floor(hi - lo) + 1) > 2 ** 18
    assert all(r["n_correspondences"] > 100 for r in res)


def _capped_fitness(Gf, T, others, cap2=np.float32(4.0)):
    """k_icp_apply in f32, brute-force f32 d^2 in the kernel's order, mean of those <= cap^2 in f64.  The x slab only leaves out
    targets whose d^2 exceeds the cap, which cannot change which queries count or their minimum."""
    m = T.astype(np.float32)
    x, y, z = Gf[:, 0], Gf[:, 1], Gf[:, 2]
    q = np.stack([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)], 1)
    assert q.dtype == np.float32
    q = q[np.argsort(q[:, 0], kind="stable")]
    t = others[np.argsort(others[:, 0], kind="stable"), :3]
    t = t[np.isfinite(t).all(1)]
    dmin = []
    for i in range(0, q.shape[0], 512):
        c = q[i:i + 512]
        j0, j1 = np.searchsorted(t[:, 0], c[0, 0] - 2.01), np.searchsorted(t[:, 0], c[-1, 0] + 2.01)
        if j1 <= j0:
            continue
        s = t[j0:j1]
        dx, dy, dz = c[:, None, 0] - s[None, :, 0], c[:, None, 1] - s[None, :, 1], c[:, None, 2] - s[None, :, 2]
        d = dx * dx
        d += dy * dy
        d += dz * dz
        assert d.dtype == np.float32
        dmin.append(d.min(1))
    dmin = np.concatenate(dmin)
    keep = dmin[dmin <= cap2].astype(np.float64)
    return keep.sum() / keep.shape[0], keep.shape[0]


def test_refine_small_cap_and_capped_fitness(S, moved, kf):
    frames, poses = kf
    P, res, G = _vs_single(S, moved, frames, poses, cap=2.0, iters=20, fitness=False)
    for f in range(3):
        want, n = _capped_fitness(G[f], res[f]["T"], np.concatenate([G[g] for g in range(3) if g != f]))
        assert n > 5000
        assert abs(res[f]["fitness"] - want) <= 1e-10 * want, (f, res[f]["fitness"], want)


def _pose_distance(a12, b12):
    A, B = np.asarray(a12).reshape(3, 4), np.asarray(b12).reshape(3, 4)
    c = (np.trace(A[:, :3].T @ B[:, :3]) - 1.0) / 2.0
    return np.linalg.norm(A[:, 3] - B[:, 3]), np.degrees(np.arccos(min(1.0, max(-1.0, c))))


def test_refine_brings_a_displaced_keyframe_back(O, S, kf):
    frames, poses = kf
    th = 0.02
    D = np.eye(4)
    D[:3, :3] = [[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]]
    D[:3, 3] = (0.3, -0.2, 0.05)
    P7 = np.eye(4)
    P7[:3] = poses[1].reshape(3, 4)
    ps = poses.copy()
    ps[1] = (D @ P7)[:3].reshape(12)
    d0, a0 = _pose_distance(ps[1], poses[1])
    assert d0 > 0.2 and a0 > 1.0
    # the premise, on the oracle alone
    Go = [O.mapmerge([f], [p]) for f, p in zip(frames, ps)]
    ro = O.icp_align(Go[1], np.concatenate([Go[0], Go[2]]), max_corr=2.0)
    back = (ro["T"] @ D @ P7)[:3].reshape(12)
    d1, a1 = _pose_distance(back, poses[1])
    assert ro["converged"] and d1 < 0.5 * d0 and a1 < 0.5 * a0, ("the oracle's own refine does not bring the frame back", d0, a0, d1, a1)
    # the device against the oracle
    rf = S.MultiviewRefine(3, sum(f.shape[0] for f in frames), max_corr_dist=2.0)
    P, res, _ = rf.refine(frames, ps, fixed=[1, 0, 1], rounds=1)
    rf.close()
    assert res[1]["iterations"] == ro["iterations"] and res[1]["state"] == ro["state"]
    assert np.abs(res[1]["T"] - ro["T"]).max() <= 1e-9, (res[1]["T"], ro["T"])
    d2, a2 = _pose_distance(P[1], poses[1])
    assert res[1]["accepted"] and d2 < 0.5 * d0 and a2 < 0.5 * a0


def _res_equal(a, b):
    return all(_same(x, y) and x["fitness"] == y["fitness"] and x["accepted"] == y["accepted"] for x, y in zip(a, b))


def test_refine_rounds(S, kf):
    frames, poses = kf
    n = sum(f.shape[0] for f in frames)
    rf = S.MultiviewRefine(3, n, max_corr_dist=2.0, max_iterations=20)
    P3, r3, run3 = rf.refine(frames, poses, fixed=[1, 0, 0], rounds=3)
    P, runs = poses, 0
    for _ in range(run3):
        P, r1, one = rf.refine(frames, P, fixed=[1, 0, 0], rounds=1)
        assert one == 1
        runs += 1
    assert 1 <= run3 <= 3 and np.array_equal(P3, P) and _res_equal(r3, r1)
    assert any(r["accepted"] for r in r3) or run3 == 1
    # two identical runs are bitwise equal
    Pb, rb, runb = rf.refine(frames, poses, fixed=[1, 0, 0], rounds=3)
    assert runb == run3 and np.array_equal(Pb, P3) and _res_equal(rb, r3)
    # nothing can be accepted: the rounds stop after the first
    Pf, rfx, runf = rf.refine(frames, poses, fixed=[1, 1, 1], rounds=3)
    assert runf == 1 and np.array_equal(Pf, poses) and not any(r["accepted"] for r in rfx)
    rf.close()
    gate = S.MultiviewRefine(3, n, max_corr_dist=2.0, max_iterations=20, fitness_gate=-1.0)
    Pg, rg, rung = gate.refine(frames, poses, rounds=3)
    assert rung == 1 and np.array_equal(Pg, poses) and not any(r["accepted"] for r in rg) and all(r["converged"] for r in rg)
    gate.close()


def test_refine_errors_leave_the_context_usable(S, kf):
    a = kf[0][0]
    rf = S.MultiviewRefine(2, 2 * a.shape[0], max_corr_dist=150.0)
    small = a[:100]
    with pytest.raises(S.ScalError) as e:
        rf.refine([small, small, small], np.stack([IDENT12] * 3))
    assert e.value.code == S.E_TOO_MANY
    with pytest.raises(S.ScalError) as e:
        rf.refine([small, small], np.stack([IDENT12] * 2), rounds=0)
    assert e.value.code == S.E_ARG
    with pytest.raises(S.ScalError) as e:
        rf.refine([np.concatenate([a, a]), a[:10]], np.stack([IDENT12] * 2))
    assert e.value.code == S.E_TOO_MANY
    L = S.lib()
    pts = np.ascontiguousarray(small)
    P = np.stack([IDENT12] * 2)
    res = (S.RefineFrameResult * 2)()
    run = C.c_int(0)
    i32p, f64p = C.POINTER(C.c_int), C.POINTER(C.c_double)

    def call(off, poses=P, r=res, rr=run, ptr=pts.ctypes.data_as(C.c_void_p), rounds=1):
        o = np.array(off, np.int32)
        return L.scal_refine_run(rf.h, ptr, o.ctypes.data_as(i32p), 2, poses.ctypes.data_as(f64p) if poses is not None else None, None, 2.0,
                                 rounds, r, C.byref(rr) if rr is not None else None)
    assert call([0, 60, 50]) == S.E_ARG and call([1, 50, 100]) == S.E_ARG and call([0, -1, 100]) == S.E_ARG
    assert call([0, 50, 100], poses=None) == S.E_ARG and call([0, 50, 100], r=None) == S.E_ARG and call([0, 50, 100], rr=None) == S.E_ARG
    assert call([0, 50, 100], ptr=None) == S.E_ARG and call([0, 50, 100], rounds=-3) == S.E_ARG
    assert L.scal_refine_run(rf.h, pts.ctypes.data_as(C.c_void_p), None, 2, P.ctypes.data_as(f64p), None, 2.0, 1, res, C.byref(run)) == S.E_ARG
    assert L.scal_refine_run_device(None, None, None, 0, None, None, 2.0, 1, None, None) == S.E_ARG
    assert b"scal_refine" in L.scal_last_error()
    assert call([0, 50, 100]) == S.OK and run.value == 1
    _case3(S, rf, a)
    rf.close()


def small_frames():
    """three pieces (500, 400 and 350 points) of one room corner of three 24 x 24 lattices at 0.25 m, each moved by a few centimetres
    and a few milliradians and given 5 mm of noise"""
    from test_icp_plane_cpu import corner_scene
    from test_icp_point_cpu import rigid
    rng = np.random.default_rng(71)
    corner = corner_scene()[0][:, :3].astype(np.float64)
    frames = []
    for n, axis, th, t in ((500, [0.0, 0.2, 1.0], 0.004, [0.02, -0.01, 0.015]), (400, [1.0, 0.0, 0.3], -0.006, [-0.03, 0.02, 0.01]),
                           (350, [0.3, 1.0, 0.0], 0.005, [0.01, 0.03, -0.02])):
        M = rigid(axis, th, t)
        xyz = corner[rng.permutation(corner.shape[0])[:n]] @ M[:3, :3].T + M[:3, 3] + rng.normal(0.0, 0.005, (n, 3))
        f = np.zeros((n, 4), np.float32)
        f[:, :3] = xyz
        frames.append(f)
    return frames


@pytest.mark.parametrize("cap", [2.0, 150.0])
def test_refine_at_small_shapes_equals_the_cpu_restatement(S, cap):
    """Identity poses and near_thres = 0 leave the frames as they are, so every frame's result is scaloam.icp_point.align of the frame
    against the concatenation of the others - the cell-hash lookup, the own-frame exclusion and frames of one to two workgroups
    against a reference that is not the GPU.  cap 2.0: the rings alone; 150: with the dense list behind them.  The refine's
    fitness keeps the cap, the restatement's does not: the scenes have every point's neighbour within it."""
    from scaloam import icp_plane, icp_point
    from test_icp_point_cpu import same_result
    frames = small_frames()
    assert [f.shape[0] for f in frames] == [500, 400, 350]
    for fr in (frames, [frames[0], frames[0].copy(), frames[2]]):     # and two identical frames: ties resolve to the lower frame
        want = [icp_point.align(fr[f], np.concatenate([fr[g] for g in range(3) if g != f]), max_corr_dist=cap, max_iterations=20)
                for f in range(3)]
        for f in range(3):
            others = np.concatenate([fr[g] for g in range(3) if g != f])
            moved = icp_plane.transform(want[f]["T"].astype(np.float32), fr[f])
            assert icp_point.sweep_sums(moved, others, np.float32(cap * cap))[0] == fr[f].shape[0]
            assert want[f]["converged"] and want[f]["iterations"] >= 1
        rf = S.MultiviewRefine(3, sum(f.shape[0] for f in fr), max_corr_dist=cap, max_iterations=20)
        P, res, run = rf.refine(fr, np.stack([IDENT12] * 3), rounds=1, near_thres=0.0)
        rf.close()
        assert run == 1
        for f in range(3):
            assert same_result(res[f], want[f]), (f, res[f], want[f])
