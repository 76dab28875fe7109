"""CPU restatement of scal_refine_run_plane* (include/scaloam_hip.h): the multiview refine with the point-to-plane metric, the
specification csrc/refine.hip's plane path is held to bit for bit.  numpy only here; the alignment itself is icp_plane's.  Every f64
expression is elementwise, one rounding per operation, in the order the header states.  DESIGN.md section 8.16 has the reasoning.

A round: every frame and its local normals moved by the frame's pose (move), every non-fixed frame aligned by
icp_plane.align_plane against the concatenation of the other frames' moved points and normals, the refine's own fitness (the mean
f32 d over the rows of the final sweep) from icp_plane.sweep_sums, acceptance and pose update as the point refine's."""
import numpy as np

from . import icp_plane

_DBL_MAX = float(np.finfo(np.float64).max)


def _xyzi(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 4)


def move(frame_xyzi, nc, pose12, near_thres):
    """(G, N): the points of the frame that pass the near-range rule sqrt((x x + y y) + z z) > near_thres, moved by the pose in the
    map merge's order ((P0 x + P1 y) + P2 z) + P3, and their normals rotated as (P0 nx + P1 ny) + P2 nz - f64 on the promoted f32
    values, rounded to f32 once; .w (intensity, curvature) copied.  Both in the frame's order."""
    f = np.float64
    A, Nc = _xyzi(frame_xyzi), _xyzi(nc)
    if A.shape[0] != Nc.shape[0]:
        raise ValueError("nc is [n, 4]: one normal and curvature per point of the frame")
    P = np.asarray(pose12, f).reshape(12)
    with np.errstate(all="ignore"):
        x, y, z = A[:, 0].astype(f), A[:, 1].astype(f), A[:, 2].astype(f)
        keep = np.sqrt((x * x + y * y) + z * z) > f(near_thres)
        x, y, z = x[keep], y[keep], z[keep]
        G = A[keep].copy()
        for r in range(3):
            G[:, r] = (((P[4 * r] * x + P[4 * r + 1] * y) + P[4 * r + 2] * z) + P[4 * r + 3]).astype(np.float32)
        nn = Nc[keep]
        nx, ny, nz = nn[:, 0].astype(f), nn[:, 1].astype(f), nn[:, 2].astype(f)
        N = nn.copy()
        for r in range(3):
            N[:, r] = ((P[4 * r] * nx + P[4 * r + 1] * ny) + P[4 * r + 2] * nz).astype(np.float32)
    return G, N


def _compose(T, pose12):
    """pose <- T pose in f64: ((T[r][0] P[0][c] + T[r][1] P[1][c]) + T[r][2] P[2][c]) (+ T[r][3] for c = 3)"""
    P = np.asarray(pose12, np.float64).reshape(3, 4)
    Q = np.zeros((3, 4), np.float64)
    for r in range(3):
        for c in range(4):
            v = (T[r, 0] * P[0, c] + T[r, 1] * P[1, c]) + T[r, 2] * P[2, c]
            Q[r, c] = v + T[r, 3] if c == 3 else v
    return Q.reshape(12)


def refine_plane(frames, normals, poses12, fixed=None, rounds=1, near_thres=2.0, max_corr_dist=2.0, max_iterations=100,
                 transformation_epsilon=1e-6, fitness_epsilon=1e-6, fitness_gate=0.3):
    """scal_refine_run_plane on the CPU: (poses12 [K, 12], per-frame dicts, rounds_run) as scaloam.MultiviewRefine.refine_plane
    returns them.  frames: [n_f, 4] xyzi in their local frames; normals: [n_f, 4] per frame, as frame_normals gives them."""
    fs, ns = [_xyzi(a) for a in frames], [_xyzi(a) for a in normals]
    K = len(fs)
    P = np.array(poses12, np.float64).reshape(-1, 12).copy()
    if len(ns) != K or P.shape[0] != K or any(a.shape[0] != b.shape[0] for a, b in zip(fs, ns)):
        raise ValueError("one normals array and one pose12 row per frame are needed")
    if rounds < 1:
        raise ValueError("rounds must be >= 1")
    fx = np.zeros(K, bool) if fixed is None else np.asarray(fixed) != 0
    max2 = np.float32(np.float64(max_corr_dist) * np.float64(max_corr_dist))
    empty = np.zeros((0, 4), np.float32)
    res, run = [], 0
    for _ in range(rounds):
        GN = [move(fs[f], ns[f], P[f], near_thres) for f in range(K)]
        res, moved = [], False
        for f in range(K):
            r = dict(converged=False, iterations=0, state=0, n_correspondences=0, accepted=False, fitness=_DBL_MAX, T=np.eye(4),
                     plane_fitness=_DBL_MAX, normal_eq=np.zeros(27), first_eq=np.zeros(27))
            res.append(r)
            if fx[f]:
                continue
            tgt = np.concatenate([GN[g][0] for g in range(K) if g != f] + [empty])
            tnc = np.concatenate([GN[g][1] for g in range(K) if g != f] + [empty])
            a = icp_plane.align_plane(GN[f][0], tgt, tnc, None, max_corr_dist, max_iterations, transformation_epsilon, fitness_epsilon)
            r.update({k: a[k] for k in ("converged", "iterations", "state", "n_correspondences", "T", "plane_fitness", "normal_eq", "first_eq")})
            if GN[f][0].shape[0] == 0 or tgt.shape[0] == 0:
                continue
            s = icp_plane.sweep_sums(icp_plane.transform(a["T"].astype(np.float32), GN[f][0]), tgt, tnc, max2)
            assert np.array_equal(s[1:28], a["normal_eq"])
            with np.errstate(all="ignore"):
                r["fitness"] = float(s[29] / s[0]) if s[0] > 0 else _DBL_MAX
            r["accepted"] = bool(a["converged"] and r["fitness"] <= fitness_gate)
            if r["accepted"]:
                P[f] = _compose(a["T"], P[f])
                moved = moved or not np.array_equal(a["T"], np.eye(4))
        run += 1
        if not moved:
            break
    return P, res, run


def frame_normals(frames, k=10, r=0.8, device=False):
    """per frame nbr.estimate_normals' nc [n_f, 4]: the normal and curvature of every point among the points of its own frame, in
    the frame's local coordinates (device=True: scaloam.RadiusIndex.normals_self, the same bits)"""
    from . import nbr
    return [nbr.estimate_normals(_xyzi(a), k, r, device=device)[0] for a in frames]
