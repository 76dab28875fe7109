"""scaloam.refine_plane, the CPU restatement of scal_refine_run_plane* (include/scaloam_hip.h), on its own,
and what of the new calls can be checked without a GPU: the move of points and normals, the refine against the single plane
alignment it is defined by, the degenerate pair, a displaced frame coming back, the result struct against the header and the
argument checks.  tests/test_refine_plane_gpu.py holds the device to this module bit for bit and takes its scenes from here."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from test_icp_plane_cpu import same_result
from test_icp_point_cpu import rigid
from test_refine_gpu import IDENT12, small_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = float(np.finfo(np.float64).max)
PLANE_FIELDS = ("converged", "iterations", "state", "n_correspondences", "T", "plane_fitness", "normal_eq", "first_eq")

# the motions test_refine_gpu.small_frames gives its three pieces of the corner: a piece's true pose is the inverse of its motion
PIECE_MOTIONS = (([0.0, 0.2, 1.0], 0.004, [0.02, -0.01, 0.015]), ([1.0, 0.0, 0.3], -0.006, [-0.03, 0.02, 0.01]),
                 ([0.3, 1.0, 0.0], 0.005, [0.01, 0.03, -0.02]))
# max |pose - true pose| of piece 0 after one round of the restatement below: 3.43e-3 from 3.99e-2 (3 iterations, state 2, measured
# on the CPU; the pieces carry 5 mm of noise); times 4, the margin test_icp_plane_cpu.py gives its corner
DISPLACED_ERR = 3.43e-3
DISPLACED_TOL = 4 * DISPLACED_ERR


@pytest.fixture(scope="module")
def RP():
    from scaloam import refine_plane
    return refine_plane


@functools.lru_cache(maxsize=None)
def corner_pieces():
    """small_frames() and their normals at k = 10, r = 0.8 (computed once; do not write to them)"""
    from scaloam import refine_plane
    frames = small_frames()
    return frames, refine_plane.frame_normals(frames, 10, 0.8)


def true_poses():
    return np.stack([np.linalg.inv(rigid(*m))[:3].reshape(12) for m in PIECE_MOTIONS])


def displaced_poses(f=0):
    """the true poses with that of piece f displaced by a known small motion"""
    D = rigid([0.2, -0.3, 1.0], 0.01, [0.04, -0.03, 0.02])
    ps = true_poses()
    M = np.eye(4)
    M[:3] = ps[f].reshape(3, 4)
    ps[f] = (D @ M)[:3].reshape(12)
    return ps


def plane_pair():
    """a 20 x 15 lattice at 0.25 m in z = 0 and a copy shifted by (0.1, 0, 0.03) m, both with the normal (0, 0, 1)"""
    i, j = np.meshgrid(np.arange(1, 21) * 0.25, np.arange(1, 16) * 0.25, indexing="ij")
    a = np.zeros((300, 4), np.float32)
    a[:, 0], a[:, 1] = i.reshape(-1), j.reshape(-1)
    b = a.copy()
    b[:, 0] += np.float32(0.1)
    b[:, 2] += np.float32(0.03)
    nc = np.zeros((300, 4), np.float32)
    nc[:, 2] = 1.0
    return [a, b], [nc, nc.copy()]


def same_frame_result(a, b, fitness=True):
    """every field of two per-frame results of refine_plane, bit for bit (fitness only where the caller has shown it comparable)"""
    assert set(a) == set(b)
    for k in a:
        if k == "fitness" and not fitness:
            continue
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (k, a[k], b[k])
    return True


def pose_err(p12, q12):
    return np.abs(np.asarray(p12).reshape(12) - np.asarray(q12).reshape(12)).max()


def test_move_points_equal_the_map_merge(RP, O, golden):
    frame = golden("KAIST03_000007.npy")
    pose = golden("KAIST03_poses21.npy").reshape(-1, 12)[7].astype(np.float64)
    nc = np.zeros_like(frame)
    G, N = RP.move(frame, nc, pose, 2.0)
    want = O.mapmerge([frame], [pose], 2.0)
    assert 0 < G.shape[0] < frame.shape[0] and N.shape == G.shape
    assert np.array_equal(G.view(np.uint32), want.view(np.uint32))


def test_move_identity_keeps_the_normals_bits(RP):
    frames, normals = corner_pieces()
    for f, n in zip(frames, normals):
        nan = ~np.isfinite(n[:, :3]).all(1)
        assert nan.any() and not nan.all()
        G, N = RP.move(f, n, IDENT12, 0.0)
        assert np.array_equal(G.view(np.uint32), f.view(np.uint32))
        assert np.array_equal(N[~nan].view(np.uint32), n[~nan].view(np.uint32))
        assert not np.isfinite(N[nan, :3]).all(1).any()             # a NaN row stays a row the sums drop


def test_move_rotates_the_normals_and_keeps_them_beside_their_points(RP, golden):
    frames, normals = corner_pieces()
    pose = golden("KAIST03_poses21.npy").reshape(-1, 12)[20].astype(np.float64)
    R = pose.reshape(3, 4)[:, :3]
    # the golden poses are six-digit text: R stretches a unit vector by at most |R R^T - I|_2 / 2 (to first order), 3.4 f32 ulps here
    stretch = 0.5 * np.linalg.norm(R @ R.T - np.eye(3), 2)
    assert stretch <= 5e-7
    f, n = frames[0].copy(), normals[0].copy()
    f[:, 3] = n[:, 3] = np.arange(f.shape[0])                      # .w carries the input position through the move
    near = 4.0
    keep = np.sqrt((f[:, :3].astype(np.float64) ** 2).sum(1)) > near
    dropped = np.flatnonzero(~keep)
    assert 20 < dropped.size < f.shape[0] - 20 and dropped[0] < keep.size - dropped.size      # dropped points are not (all) at the end
    G, N = RP.move(f, n, pose, near)
    assert G.shape[0] == keep.sum() and np.array_equal(G[:, 3], N[:, 3]) and np.array_equal(G[:, 3], np.flatnonzero(keep))
    G0, N0 = RP.move(f[keep], n[keep], pose, 0.0)
    assert np.array_equal(G.view(np.uint32), G0.view(np.uint32)) and np.array_equal(N.view(np.uint32), N0.view(np.uint32))
    fin = np.isfinite(N[:, :3]).all(1)
    assert np.array_equal(fin, np.isfinite(n[keep, :3]).all(1)) and 0 < (~fin).sum() < fin.size
    ln_in = np.sqrt((n[keep][fin, :3].astype(np.float64) ** 2).sum(1))
    ln = np.sqrt((N[fin, :3].astype(np.float64) ** 2).sum(1))
    ulp = 2.0 ** -23
    assert np.abs(ln_in - 1.0).max() <= 2 * ulp                     # unit on the way in ...
    # ... and on the way out: the pose's own stretch, and one ulp for the three roundings to f32 (sqrt(3) 2^-25 < 2^-23)
    assert np.abs(ln - ln_in).max() <= 1.01 * stretch + ulp and np.abs(ln - 1.0).max() <= 8 * ulp
    want = n[keep][fin, :3].astype(np.float64) @ R.T                # and the rotation is the pose's
    assert np.abs(N[fin, :3] - want).max() <= 2 * ulp


@pytest.mark.parametrize("cap", [2.0, 150.0])
def test_refine_plane_equals_the_single_plane_alignments(RP, cap):
    from scaloam import icp_plane
    frames, normals = corner_pieces()
    assert [f.shape[0] for f in frames] == [500, 400, 350]
    P, res, run = RP.refine_plane(frames, normals, np.stack([IDENT12] * 3), rounds=1, near_thres=0.0, max_corr_dist=cap, max_iterations=20)
    assert run == 1
    for f in range(3):
        tgt = np.concatenate([frames[g] for g in range(3) if g != f])
        tnc = np.concatenate([normals[g] for g in range(3) if g != f])
        want = icp_plane.align_plane(frames[f], tgt, tnc, max_corr_dist=cap, max_iterations=20)
        # the premises: converged by the increment, an iteration made, NaN normals in play and correspondences dropped for them
        assert want["state"] == 2 and want["iterations"] >= 1
        assert (~np.isfinite(normals[f][:, :3]).all(1)).any() and want["n_correspondences"] < frames[f].shape[0]
        for k in PLANE_FIELDS:
            assert np.array_equal(np.asarray(res[f][k]), np.asarray(want[k])), (f, k)
        moved = icp_plane.transform(want["T"].astype(np.float32), frames[f])
        s = icp_plane.sweep_sums(moved, tgt, tnc, np.float32(cap * cap))
        assert res[f]["fitness"] == s[29] / s[0] and res[f]["accepted"]
        # pose <- T pose from the identity is T's first three rows
        assert np.array_equal(P[f], want["T"][:3].reshape(12))
    assert [r["iterations"] for r in res] == [3, 4, 4] and [r["n_correspondences"] for r in res] == [498, 397, 349]


def test_refine_plane_single_plane_pair_is_degenerate(RP):
    frames, normals = plane_pair()
    P, res, run = RP.refine_plane(frames, normals, np.stack([IDENT12] * 2), rounds=3, near_thres=0.0, max_corr_dist=2.0)
    assert run == 1 and np.array_equal(P, np.stack([IDENT12] * 2))
    for r in res:
        assert r["state"] == 6 and r["iterations"] == 0 and r["n_correspondences"] == 300
        assert not r["converged"] and not r["accepted"] and np.array_equal(r["T"], np.eye(4))
        assert np.array_equal(r["first_eq"], r["normal_eq"]) and r["first_eq"].any()


def test_refine_plane_fixed_and_empty_frames(RP):
    frames, normals = corner_pieces()
    empty = np.zeros((0, 4), np.float32)
    P, res, run = RP.refine_plane([frames[0], empty, frames[1]], [normals[0], empty, normals[1]], np.stack([IDENT12] * 3), fixed=[1, 0, 0],
                                  near_thres=0.0, max_iterations=20)
    assert res[0]["state"] == 0 and not res[0]["accepted"] and res[0]["fitness"] == DBL_MAX and not res[0]["normal_eq"].any()
    assert res[1]["state"] == 5 and not res[1]["accepted"] and res[1]["plane_fitness"] == DBL_MAX and not res[1]["first_eq"].any()
    assert res[2]["state"] == 2 and res[2]["accepted"] and np.array_equal(P[:2], np.stack([IDENT12] * 2))
    with pytest.raises(ValueError):
        RP.refine_plane(frames, normals[:2], np.stack([IDENT12] * 3))
    with pytest.raises(ValueError):
        RP.refine_plane(frames, normals, np.stack([IDENT12] * 3), rounds=0)


def test_refine_plane_brings_a_displaced_piece_back(RP):
    frames, normals = corner_pieces()
    true, ps = true_poses(), displaced_poses(0)
    before = pose_err(ps[0], true[0])
    P, res, run = RP.refine_plane(frames, normals, ps, fixed=[0, 1, 1], rounds=1, near_thres=0.0, max_corr_dist=2.0)
    after = pose_err(P[0], true[0])
    print("displaced piece: max |pose - true| before", before, "after", after, "iterations", res[0]["iterations"], "state", res[0]["state"])
    assert res[0]["converged"] and res[0]["accepted"] and np.array_equal(P[1:], ps[1:])
    assert after < before
    assert after <= DISPLACED_TOL


def test_refine_plane_result_layout_matches_the_header(S, tmp_path):
    names = ["converged", "iterations", "state", "n_correspondences", "accepted", "fitness", "T", "plane_fitness", "normal_eq", "first_eq"]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scaloam_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu", sizeof(scal_refine_plane_frame_result), sizeof(scal_refine_frame_result), sizeof(scal_refine_config));\n'
                   + "".join(f'    printf(" %zu", offsetof(scal_refine_plane_frame_result, {n}));\n' for n in names) + '    return 0;\n}\n')
    exe = tmp_path / "sizes"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    R, B = S.RefinePlaneFrameResult, S.RefineFrameResult
    assert got[:3] == [C.sizeof(R), C.sizeof(B), C.sizeof(S.RefineConfig)]
    assert got[3:] == [getattr(R, n).offset for n in names]
    assert [n for n, _ in R._fields_] == names
    # the fields it shares with scal_refine_frame_result sit where they sit there
    assert all(getattr(R, n).offset == getattr(B, n).offset for n, _ in B._fields_)
    assert {"scal_refine_run_plane", "scal_refine_run_plane_device"} <= set(S.EXPORTED_SYMBOLS)


def test_refine_plane_argument_checks_and_no_device(S):
    L = S.lib()
    i32p, f64p = C.POINTER(C.c_int), C.POINTER(C.c_double)
    off = np.array([0, 1], np.int32)
    P = np.zeros(12)
    pts, nc = np.zeros((1, 4), np.float32), np.zeros((1, 4), np.float32)
    res = (S.RefinePlaneFrameResult * 1)()
    run = C.c_int(0)
    for fn in (L.scal_refine_run_plane, L.scal_refine_run_plane_device):
        assert fn(None, pts.ctypes.data_as(C.c_void_p), nc.ctypes.data_as(C.c_void_p), off.ctypes.data_as(i32p), 1, P.ctypes.data_as(f64p), None, 2.0, 1,
                  res, C.byref(run)) == S.E_ARG
        assert b"scal_refine_run" in L.scal_last_error()
    if S.device_count() < 1:
        with pytest.raises(S.ScalError) as e:
            S.MultiviewRefine(4, 1000)
        assert e.value.code == S.E_NO_DEVICE
        return
    rf = S.MultiviewRefine(1, 10)
    try:
        def call(fn, p=pts, n=nc, o=off, poses=P, r=res, rr=run, rounds=1, near=2.0):
            return fn(rf.h, p.ctypes.data_as(C.c_void_p) if p is not None else None, n.ctypes.data_as(C.c_void_p) if n is not None else None,
                      o.ctypes.data_as(i32p) if o is not None else None, 1, poses.ctypes.data_as(f64p) if poses is not None else None, None, near,
                      rounds, r, C.byref(rr) if rr is not None else None)
        fn = L.scal_refine_run_plane
        assert call(fn, n=None) == S.E_ARG and b"scal_refine_run_plane" in L.scal_last_error()
        assert call(fn, p=None) == S.E_ARG and call(fn, o=None) == S.E_ARG and call(fn, poses=None) == S.E_ARG
        assert call(fn, r=None) == S.E_ARG and call(fn, rr=None) == S.E_ARG and call(fn, rounds=0) == S.E_ARG
        assert call(fn, near=float("nan")) == S.E_ARG and call(fn, o=np.array([1, 2], np.int32)) == S.E_ARG
        assert call(fn, o=np.array([0, 11], np.int32)) == S.E_TOO_MANY
        assert call(fn, o=np.array([0, 0], np.int32), p=None, n=None) == S.OK and res[0].state == 5
    finally:
        rf.close()
