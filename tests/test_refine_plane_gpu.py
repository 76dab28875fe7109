"""scal_refine_run_plane* (csrc/refine.hip) against scaloam.refine_plane, its CPU restatement, bit for bit in every result field, and
against the single plane alignment it is defined by (S.LoopICP.align_plane on the moved frames).  The scenes are
tests/test_refine_plane_cpu.py's: three noisy pieces of a room corner with k-NN normals (some NaN), a single-plane pair, and the
golden KAIST03 keyframes 0 / 7 / 20.  `fitness` is the refine's own ([29] / [0] of the final sweep) wherever the restatement is the
yardstick; against LoopICP.align_plane, whose fitness is uncapped, it is compared only after the test has shown the two comparable."""
import ctypes as C

import numpy as np
import pytest

from test_icp_plane_cpu import corner_scene
from test_icp_point_cpu import rigid
from test_refine_gpu import IDENT12
from test_refine_plane_cpu import PLANE_FIELDS, corner_pieces, displaced_poses, plane_pair, same_frame_result, true_poses

pytestmark = pytest.mark.gpu

DBL_MAX = float(np.finfo(np.float64).max)
I3 = np.stack([IDENT12] * 3)


@pytest.fixture(scope="module")
def RP():
    from scaloam import refine_plane
    return refine_plane


def device(S, frames, normals, poses, fixed=None, rounds=1, near=0.0, cap=2.0, iters=20, **kw):
    n = sum(f.shape[0] for f in frames)
    rf = S.MultiviewRefine(max(len(frames), 1), max(n, 1), max_corr_dist=cap, max_iterations=iters, **kw)
    try:
        return rf.refine_plane(frames, normals, poses, fixed=fixed, rounds=rounds, near_thres=near)
    finally:
        rf.close()


def same_run(a, b):
    """(poses, results, rounds) of two runs, bit for bit"""
    assert a[2] == b[2] and np.array_equal(a[0], b[0]) and len(a[1]) == len(b[1])
    for f, (x, y) in enumerate(zip(a[1], b[1])):
        assert same_frame_result(x, y), f
    return True


def vs_single(S, RP, frames, normals, poses, res, near, cap, iters, fixed=None):
    """every non-fixed frame's result against S.LoopICP.align_plane(G_f, concat(G_g, g != f), concat(N_g, g != f)) on move's output"""
    GN = [RP.move(f, n, p, near) for f, n, p in zip(frames, normals, poses)]
    m = max(sum(g.shape[0] for g, _ in GN), 1)
    icp = S.LoopICP(max_source=m, max_target=m, max_corr_dist=cap, max_iterations=iters)
    try:
        for f in range(len(frames)):
            if fixed is not None and fixed[f]:
                continue
            tgt = np.concatenate([GN[g][0] for g in range(len(frames)) if g != f])
            tnc = np.concatenate([GN[g][1] for g in range(len(frames)) if g != f])
            s = icp.align_plane(GN[f][0], tgt, tnc)
            for k in PLANE_FIELDS:
                assert np.array_equal(np.asarray(res[f][k]), np.asarray(s[k])), (f, k, res[f][k], s[k])
    finally:
        icp.close()
    return GN


@pytest.mark.parametrize("cap", [2.0, 150.0])
def test_small_frames_equal_the_restatement(S, RP, cap):
    """cap 2.0: the rings alone; 150: with the dense list behind them.  Then frames 0 and 1 identical: ties resolve to the lower frame."""
    frames, normals = corner_pieces()
    for fr, ns in ((frames, normals), ([frames[0], frames[0].copy(), frames[2]], [normals[0], normals[0].copy(), normals[2]])):
        want = RP.refine_plane(fr, ns, I3, rounds=1, near_thres=0.0, max_corr_dist=cap, max_iterations=20)
        assert all(r["iterations"] >= 1 and r["converged"] for r in want[1])
        assert sum(r["n_correspondences"] < f.shape[0] for r, f in zip(want[1], fr)) >= 2      # correspondences dropped for NaN normals
        got = device(S, fr, ns, I3, cap=cap)
        assert same_run(got, want)


def test_workgroup_edges(S, RP):
    """frames of 1, 5, 6, 255, 257, 1025 and 256 points in one call: most start off a multiple of 256 in the union, two end in a
    workgroup of one point, and every row count is checked - a last partial workgroup left out of the sum loses its rows"""
    tgt, nc, _, _ = corner_scene()
    rng = np.random.default_rng(93)
    sizes = [1, 5, 6, 255, 257, 1025, 256]
    frames, normals = [], []
    for k, n in enumerate(sizes):
        pick = np.sort(rng.permutation(tgt.shape[0])[:n])
        M = rigid([0.1 * k, 1.0, 0.3], 0.002 * (k + 1), [0.01 * (k % 3), -0.008, 0.005 * k])
        f = tgt[pick].copy()
        f[:, :3] = (tgt[pick, :3].astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
        frames.append(f)
        normals.append(nc[pick].copy())
    starts = np.cumsum([0] + sizes)[:-1]
    assert (starts % 256 != 0).sum() >= 5
    poses = np.stack([IDENT12] * len(sizes))
    want = RP.refine_plane(frames, normals, poses, rounds=1, near_thres=0.0, max_corr_dist=2.0, max_iterations=20)
    # every point has a neighbour within the cap and every normal is finite: a frame's rows are its points
    assert [r["n_correspondences"] for r in want[1]] == sizes
    assert [r["state"] for r in want[1]][:2] == [5, 5] and all(r["state"] not in (0, 5) for r in want[1][2:])
    assert all(r["iterations"] >= 1 for r in want[1][3:])
    got = device(S, frames, normals, poses)
    assert [r["n_correspondences"] for r in got[1]] == sizes
    assert same_run(got, want)
    # where every point of the final sweep has its neighbour within the cap and that neighbour's normal is finite (asserted), the
    # refine's fitness [29] / [0] is scal_icp_plane_result's uncapped [31] / [30], bit for bit
    for f in range(2, len(sizes)):
        tgt_f = np.concatenate([frames[g] for g in range(len(sizes)) if g != f])
        tnc_f = np.concatenate([normals[g] for g in range(len(sizes)) if g != f])
        s = RP.icp_plane.sweep_sums(RP.icp_plane.transform(got[1][f]["T"].astype(np.float32), frames[f]), tgt_f, tnc_f, np.float32(4.0))
        assert s[0] == sizes[f] == s[30]
        assert got[1][f]["fitness"] == s[31] / s[30]


def test_poses_and_near_range_move_the_normals_with_their_points(S, RP):
    """non-identity poses and a near-range rule that removes points from the inside of every frame's index range: normals written at
    uncompacted positions or left unrotated do not survive this"""
    frames, normals = corner_pieces()
    poses = displaced_poses(1)
    M = rigid([0.3, -0.2, 1.0], 0.7, [3.0, -2.0, 0.5])               # and the whole session turned by 40 degrees: rotations that matter
    for f in range(3):
        P = np.eye(4)
        P[:3] = poses[f].reshape(3, 4)
        poses[f] = (M @ P)[:3].reshape(12)
    near = 4.0
    for f in frames:
        drop = np.flatnonzero(~(np.sqrt((f[:, :3].astype(np.float64) ** 2).sum(1)) > near))
        assert drop.size >= 1 and drop[0] < f.shape[0] - drop.size    # a dropped point that is not among the frame's last
    want = RP.refine_plane(frames, normals, poses, rounds=1, near_thres=near, max_corr_dist=2.0, max_iterations=20)
    assert all(r["iterations"] >= 1 and r["converged"] for r in want[1])
    got = device(S, frames, normals, poses, near=near)
    assert same_run(got, want)
    GN = vs_single(S, RP, frames, normals, poses, got[1], near, 2.0, 20)
    assert all(g.shape[0] < f.shape[0] for (g, _), f in zip(GN, frames))


def test_golden_keyframes_equal_the_single_plane_alignments(S, RP, golden):
    vg = S.VoxelGrid()
    frames = [vg.filter(golden(f"KAIST03_{i:06d}.npy"), 0.4) for i in (0, 7, 20)]
    vg.close()
    poses = golden("KAIST03_poses21.npy").reshape(-1, 12)[[0, 7, 20]].astype(np.float64)
    normals = []
    idx = S.RadiusIndex(max(f.shape[0] for f in frames), max(f.shape[0] for f in frames))
    for f in frames:
        idx.set_index(f, 0.8)
        normals.append(idx.normals_self(10)[0].copy())
    idx.close()
    assert all(np.isfinite(n[:, :3]).all(1).sum() > 10000 for n in normals)
    P, res, run = device(S, frames, normals, poses, near=2.0, cap=2.0, iters=12)
    assert run == 1 and all(r["iterations"] >= 1 and r["n_correspondences"] > 3000 for r in res)
    vs_single(S, RP, frames, normals, poses, res, 2.0, 2.0, 12)


def test_a_frame_without_normals(S, RP):
    frames, normals = corner_pieces()
    ns = [normals[0], np.full_like(normals[1], np.nan), normals[2]]
    want = RP.refine_plane(frames, ns, I3, rounds=1, near_thres=0.0, max_corr_dist=2.0, max_iterations=20)
    assert want[1][1]["converged"] and want[1][1]["iterations"] >= 1      # it still aligns against the others
    got = device(S, frames, ns, I3)
    assert same_run(got, want)
    # as a target it contributes no rows: frame 0 against it and frame 2 has the rows it has against frame 2 alone ...
    s = RP.icp_plane.sweep_sums(frames[0], np.concatenate([frames[1], frames[2]]), np.concatenate([ns[1], ns[2]]), np.float32(4.0))
    k = RP.icp_plane.nearest_keys(frames[0], np.concatenate([frames[1], frames[2]]))
    on2 = ((k & np.uint64(0xFFFFFFFF)).astype(np.int64) >= frames[1].shape[0])
    assert got[1][0]["first_eq"][0] == s[1] and s[0] <= on2.sum() < frames[0].shape[0]
    # ... and with nothing else there the other frame has none at all
    P, res, run = device(S, frames[:2], ns[:2], I3[:2])
    assert res[0]["state"] == 5 and res[0]["n_correspondences"] == 0 and not res[0]["accepted"] and res[0]["fitness"] == DBL_MAX
    assert not res[0]["normal_eq"].any() and res[1]["n_correspondences"] >= 6 and np.array_equal(P[0], IDENT12)
    assert same_run((P, res, run), RP.refine_plane(frames[:2], ns[:2], I3[:2], near_thres=0.0, max_corr_dist=2.0, max_iterations=20))


def test_single_plane_pair_is_degenerate_and_the_context_goes_on(S, RP):
    pf, pn = plane_pair()
    frames, normals = corner_pieces()
    n = sum(f.shape[0] for f in frames)
    rf, fresh = (S.MultiviewRefine(3, n, max_corr_dist=2.0, max_iterations=20) for _ in range(2))
    P, res, run = rf.refine_plane(pf, pn, I3[:2], rounds=3, near_thres=0.0)
    assert run == 1 and np.array_equal(P, I3[:2])
    for r in res:
        assert r["state"] == 6 and r["iterations"] == 0 and r["n_correspondences"] == 300 and not r["converged"] and not r["accepted"]
    assert same_run((P, res, run), RP.refine_plane(pf, pn, I3[:2], rounds=3, near_thres=0.0, max_corr_dist=2.0, max_iterations=20))
    good = rf.refine_plane(frames, normals, I3, near_thres=0.0)
    assert all(r["converged"] for r in good[1]) and same_run(good, fresh.refine_plane(frames, normals, I3, near_thres=0.0))
    rf.close(), fresh.close()


def test_fixed_frames_keep_their_pose_and_serve_as_targets(S, RP):
    frames, normals = corner_pieces()
    poses = displaced_poses(0)
    fixed = [0, 1, 1]
    want = RP.refine_plane(frames, normals, poses, fixed=fixed, rounds=1, near_thres=0.0, max_corr_dist=2.0, max_iterations=20)
    got = device(S, frames, normals, poses, fixed=fixed)
    assert same_run(got, want)
    P, res, _ = got
    for f in (1, 2):
        assert res[f]["state"] == 0 and not res[f]["accepted"] and not res[f]["converged"] and np.array_equal(P[f], poses[f])
        assert res[f]["fitness"] == DBL_MAX and not res[f]["normal_eq"].any() and np.array_equal(res[f]["T"], np.eye(4))
    # the fixed frames are the target, normals and all
    assert res[0]["accepted"] and res[0]["n_correspondences"] > 400
    vs_single(S, RP, frames, normals, poses, res, 0.0, 2.0, 20, fixed=fixed)
    err = lambda p: np.abs(p - true_poses()[0]).max()
    assert err(P[0]) < err(poses[0])


def test_rounds_early_stop_and_repeatability(S, RP):
    frames, normals = corner_pieces()
    poses = displaced_poses(0)
    n = sum(f.shape[0] for f in frames)
    rf = S.MultiviewRefine(3, n, max_corr_dist=2.0, max_iterations=20)
    P3, r3, run3 = rf.refine_plane(frames, normals, poses, fixed=[0, 0, 1], rounds=3, near_thres=0.0)
    P = poses
    for _ in range(run3):
        P, r1, one = rf.refine_plane(frames, normals, P, fixed=[0, 0, 1], rounds=1, near_thres=0.0)
        assert one == 1
    assert 2 <= run3 <= 3 and same_run((P3, r3, run3), (P, r1, run3))
    assert same_run((P3, r3, run3), RP.refine_plane(frames, normals, poses, fixed=[0, 0, 1], rounds=3, near_thres=0.0, max_corr_dist=2.0,
                                                    max_iterations=20))
    # two identical runs are bitwise equal
    assert same_run(rf.refine_plane(frames, normals, poses, fixed=[0, 0, 1], rounds=3, near_thres=0.0), (P3, r3, run3))
    # nothing can be accepted: the rounds stop after the first
    Pf, rfx, runf = rf.refine_plane(frames, normals, poses, fixed=[1, 1, 1], rounds=3, near_thres=0.0)
    assert runf == 1 and np.array_equal(Pf, poses) and not any(r["accepted"] for r in rfx)
    rf.close()
    Pg, rg, rung = device(S, frames, normals, poses, rounds=3, fitness_gate=-1.0)
    assert rung == 1 and np.array_equal(Pg, poses) and not any(r["accepted"] for r in rg) and all(r["converged"] for r in rg)


def test_point_and_plane_calls_alternate_on_one_context(S):
    frames, normals = corner_pieces()
    poses = displaced_poses(2)
    n = sum(f.shape[0] for f in frames)
    both, point = (S.MultiviewRefine(3, n, max_corr_dist=2.0, max_iterations=20) for _ in range(2))
    want = point.refine(frames, poses, rounds=2, near_thres=0.0)
    a = both.refine(frames, poses, rounds=2, near_thres=0.0)
    pl = both.refine_plane(frames, normals, poses, rounds=2, near_thres=0.0)
    b = both.refine(frames, poses, rounds=2, near_thres=0.0)
    pl2 = both.refine_plane(frames, normals, poses, rounds=2, near_thres=0.0)
    for got in (a, b):
        assert got[2] == want[2] and np.array_equal(got[0], want[0])
        for x, y in zip(got[1], want[1]):
            assert set(x) == set(y) and all(np.array_equal(np.asarray(x[k]), np.asarray(y[k])) for k in x)
    assert same_run(pl, pl2) and not np.array_equal(pl[0], want[0])     # and the two metrics are two metrics
    both.close(), point.close()


def test_host_arrays_and_device_pointers_agree(S):
    import torch
    frames, normals = corner_pieces()
    poses = displaced_poses(1)
    off = np.cumsum([0] + [f.shape[0] for f in frames]).astype(np.int32)
    d_pts = torch.from_numpy(np.ascontiguousarray(np.concatenate(frames), np.float32)).cuda()
    d_nc = torch.from_numpy(np.ascontiguousarray(np.concatenate(normals), np.float32)).cuda()
    rf = S.MultiviewRefine(3, int(off[-1]), max_corr_dist=2.0, max_iterations=20)
    dev = rf.refine_plane_device(d_pts.data_ptr(), d_nc.data_ptr(), off, poses, rounds=2, near_thres=3.0)
    host = rf.refine_plane(frames, normals, poses, rounds=2, near_thres=3.0)
    assert same_run(dev, host) and all(r["iterations"] >= 1 for r in host[1])
    rf.close()


def test_errors_leave_the_context_usable(S):
    frames, normals = corner_pieces()
    n = sum(f.shape[0] for f in frames)
    rf, fresh = (S.MultiviewRefine(3, n, max_corr_dist=2.0, max_iterations=20) for _ in range(2))
    with pytest.raises(S.ScalError) as e:
        rf.refine_plane(frames + [frames[0][:10]], normals + [normals[0][:10]], np.stack([IDENT12] * 4))
    assert e.value.code == S.E_TOO_MANY
    with pytest.raises(S.ScalError) as e:
        rf.refine_plane([frames[0], frames[0], frames[0]], [normals[0]] * 3, I3)
    assert e.value.code == S.E_TOO_MANY
    with pytest.raises(S.ScalError) as e:
        rf.refine_plane(frames, normals, I3, rounds=0)
    assert e.value.code == S.E_ARG
    L = S.lib()
    pts, nc = np.ascontiguousarray(frames[0]), np.ascontiguousarray(normals[0])
    P = np.stack([IDENT12] * 2)
    res = (S.RefinePlaneFrameResult * 2)()
    run = C.c_int(0)
    i32p, f64p = C.POINTER(C.c_int), C.POINTER(C.c_double)

    def call(off, nptr=nc.ctypes.data_as(C.c_void_p), ptr=pts.ctypes.data_as(C.c_void_p), poses=P, r=res, rr=run, fn=L.scal_refine_run_plane):
        o = np.array(off, np.int32)
        return fn(rf.h, ptr, nptr, o.ctypes.data_as(i32p), 2, poses.ctypes.data_as(f64p) if poses is not None else None, None, 0.0, 1, r,
                  C.byref(rr) if rr is not None else None)
    assert call([0, 50, 100], nptr=None) == S.E_ARG and b"scal_refine_run_plane" in L.scal_last_error()
    assert call([0, 50, 100], nptr=None, fn=L.scal_refine_run_plane_device) == S.E_ARG
    assert call([0, 60, 50]) == S.E_ARG and call([1, 50, 100]) == S.E_ARG and call([0, -1, 100]) == S.E_ARG
    assert call([0, 50, 100], ptr=None) == S.E_ARG and call([0, 50, 100], poses=None) == S.E_ARG
    assert call([0, 50, 100], r=None) == S.E_ARG and call([0, 50, 100], rr=None) == S.E_ARG
    assert call([0, 50, n + 1]) == S.E_TOO_MANY
    assert call([0, 0, 0], nptr=None, ptr=None) == S.OK                   # no point present: no normals needed
    assert call([0, 250, 500]) == S.OK and run.value == 1
    assert same_run(rf.refine_plane(frames, normals, I3, near_thres=0.0), fresh.refine_plane(frames, normals, I3, near_thres=0.0))
    rf.close(), fresh.close()
