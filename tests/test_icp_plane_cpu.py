"""scaloam.icp_plane, the CPU restatement of scal_icp_align_plane (include/scaloam_hip.h), on its own: the
solve against numpy's least squares, convergence on a room corner, the degenerate and the short systems, NaN normals, the guess, the
layout of the 32 sums and of the result struct.  tests/test_icp_plane_gpu.py holds the device to this module bit for bit and takes
its scenes from here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = float(np.finfo(np.float64).max)

# |T - T_true|.max() of the restatement on the room corner below is 5.2e-8 (3 iterations, state 2; measured on the CPU, DESIGN.md
# section 8.14); times 4 for the f32 rounding of other seeds and sizes
CORNER_TOL = 4 * 5.2e-8


@pytest.fixture(scope="module")
def P():
    from scaloam import icp_plane
    return icp_plane


def lattice(normal, n=24, step=0.25):
    """n x n points at `step` in the plane through the origin with the given normal, and that normal (f32) for each"""
    nrm = np.asarray(normal, np.float64)
    nrm = nrm / np.linalg.norm(nrm)
    u = np.cross(nrm, [1.0, 0, 0] if abs(nrm[0]) < 0.9 else [0, 1.0, 0])
    u /= np.linalg.norm(u)
    v = np.cross(nrm, u)
    i, j = np.meshgrid(np.arange(1, n + 1) * step, np.arange(1, n + 1) * step, indexing="ij")
    xyz = i.reshape(-1, 1) * u + j.reshape(-1, 1) * v
    pts = np.zeros((n * n, 4), np.float32)
    pts[:, :3] = xyz
    nc = np.zeros((n * n, 4), np.float32)
    nc[:, :3] = nrm
    return pts, nc


def planes(normals):
    parts = [lattice(n) for n in normals]
    return np.concatenate([p for p, _ in parts]), np.concatenate([n for _, n in parts])


def motion():
    """the 4x4 of rotation vector (0.01, -0.015, 0.02), translation (0.05, -0.04, 0.03)"""
    w = np.array([0.01, -0.015, 0.02])
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    M[:3, 3] = [0.05, -0.04, 0.03]
    return M


def moved(pts, M):
    out = pts.copy()
    out[:, :3] = (pts[:, :3].astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    return out


def corner_scene():
    """three orthogonal 24 x 24 lattices at 0.25 m with analytic normals; (target, normals, all of it moved, the motion)"""
    tgt, nc = planes([(0, 0, 1), (0, 1, 0), (1, 0, 0)])
    M = motion()
    return tgt, nc, moved(tgt, M), M


def same_result(a, b):
    """every field of two align_plane results, bit for bit"""
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (k, a[k], b[k])
    return True


def test_solve_agrees_with_lstsq(P):
    rng = np.random.default_rng(5)
    for n in (6, 40, 500):
        A = rng.standard_normal((n, 6)) * np.array([3.0, 1.0, 2.0, 1.0, 0.5, 1.5])
        r = rng.standard_normal(n)
        N = A.T @ A
        ratios = np.diag(np.linalg.cholesky(N)) ** 2 / np.diag(N)     # the LDL^T pivots d_j over A_jj
        assert ratios.min() >= 1e-3, ratios
        tri = np.array([N[i, j] for i in range(6) for j in range(i, 6)])
        x = P.solve_normal_equations(tri, A.T @ r)
        ref = np.linalg.lstsq(A, r, rcond=None)[0]
        assert x is not None and np.abs(x - ref).max() <= 1e-9 * np.abs(ref).max()


def test_room_corner_converges_to_the_inverse_motion(P):
    tgt, nc, mv, M = corner_scene()
    r = P.align_plane(mv[::3], tgt, nc, max_corr_dist=2.0)
    err = np.abs(r["T"] - np.linalg.inv(M)).max()
    print("corner: iterations", r["iterations"], "state", r["state"], "max |T - T_true|", err, "plane_fitness", r["plane_fitness"])
    assert r["converged"] and r["state"] == 2
    assert err <= CORNER_TOL
    assert r["n_correspondences"] == mv[::3].shape[0] and r["plane_fitness"] < 1e-10
    assert r["first_eq"].shape == (27,) and r["normal_eq"].shape == (27,) and not np.array_equal(r["first_eq"], r["normal_eq"])


@pytest.mark.parametrize("normals", [[(0, 0, 1)], [(0, 0, 1), (0, 1, 0)], [(0.3, -0.2, -1)], [(0.3, -0.2, -1), (0.5, 0.7, 0.1)]])
def test_one_or_two_planes_are_degenerate(P, normals):
    tgt, nc = planes(normals)
    for src in (tgt[::3], moved(tgt, motion())[::3]):
        r = P.align_plane(src, tgt, nc, max_corr_dist=2.0)
        assert r["state"] == 6 and r["iterations"] == 0 and not r["converged"]
        assert np.array_equal(r["T"], np.eye(4)) and r["n_correspondences"] == src.shape[0]
        assert r["fitness"] < DBL_MAX and np.array_equal(r["first_eq"], r["normal_eq"])


def test_too_few_rows_and_nan_normals(P):
    tgt, nc, mv, _ = corner_scene()
    six = mv[[0, 300, 576, 900, 1152, 1500]]
    r5, r6 = P.align_plane(six[:5], tgt, nc, max_corr_dist=2.0), P.align_plane(six, tgt, nc, max_corr_dist=2.0)
    assert r5["state"] == 5 and r5["n_correspondences"] == 5 and not r5["converged"] and np.array_equal(r5["T"], np.eye(4))
    assert r6["state"] != 5 and r6["iterations"] >= 1
    # every normal NaN: no row at all, while the uncapped fitness is still the sweep's
    nan = np.full_like(nc, np.nan)
    src = mv[::3]
    r = P.align_plane(src, tgt, nan, max_corr_dist=2.0)
    s = P.sweep_sums(src, tgt, nc, np.float32(4.0))
    assert r["state"] == 5 and r["n_correspondences"] == 0 and r["iterations"] == 0 and r["plane_fitness"] == DBL_MAX
    assert s[30] == src.shape[0] and r["fitness"] == s[31] / s[30] and not r["first_eq"].any()
    # a NaN in one component of one normal drops exactly the correspondence that lands on it
    own = tgt[::3]
    full = P.sweep_sums(own, tgt, nc, np.float32(4.0))
    for comp in range(3):
        one = nc.copy()
        one[3 * 7, comp] = np.nan
        cut = P.sweep_sums(own, tgt, one, np.float32(4.0))
        assert full[0] == own.shape[0] and cut[0] == full[0] - 1 and cut[30] == full[30] and cut[31] == full[31]
        alone = P.sweep_sums(own[7:8], tgt, nc, np.float32(4.0))
        assert np.allclose(full[1:30] - cut[1:30], alone[1:30], rtol=0, atol=1e-9 * np.abs(full[1:30]).max())


def test_guess_and_empty_clouds(P):
    tgt, nc, mv, M = corner_scene()
    src = mv[::3]
    none = P.align_plane(src, tgt, nc, max_corr_dist=2.0)
    assert same_result(none, P.align_plane(src, tgt, nc, None, max_corr_dist=2.0))
    assert same_result(none, P.align_plane(src, tgt, nc, np.eye(4), max_corr_dist=2.0))
    g = np.linalg.inv(M).astype(np.float32)
    r = P.align_plane(src, tgt, nc, g, max_corr_dist=2.0)
    assert r["converged"] and np.abs(r["T"] - np.linalg.inv(M)).max() <= CORNER_TOL and r["iterations"] <= none["iterations"]
    bad = np.eye(4)
    bad[3, 3] = 2.0
    nan = np.eye(4)
    nan[0, 3] = np.nan
    for guess in (bad, nan, np.eye(3)):
        with pytest.raises(ValueError):
            P.align_plane(src, tgt, nc, guess)
    empty = np.zeros((0, 4), np.float32)
    for s, t, n in ((empty, tgt, nc), (src, empty, empty), (empty, empty, empty)):
        r = P.align_plane(s, t, n)
        assert r["state"] == 5 and not r["converged"] and r["iterations"] == 0 and r["n_correspondences"] == 0
        assert np.array_equal(r["T"], np.eye(4)) and r["fitness"] == DBL_MAX and r["plane_fitness"] == DBL_MAX
        assert not r["first_eq"].any() and not r["normal_eq"].any()


def test_sweep_sums_layout_against_a_plain_loop(P):
    """Small integers as coordinates and axis normals: every term and every partial sum is an integer below 2^53, so any summation
    order gives the same bits and a plain loop pins what each of the 32 entries holds."""
    rng = np.random.default_rng(11)
    g = np.arange(12)
    a, b = [m.reshape(-1) for m in np.meshgrid(g, g, indexing="ij")]
    z = np.zeros_like(a)
    tgt = np.zeros((3 * 144, 4), np.float32)
    tgt[:, :3] = np.concatenate([np.stack([a, b, z], 1), np.stack([a, z - 1, b], 1), np.stack([z - 2, a, b], 1)])
    nc = np.zeros_like(tgt)
    nc[:144, 2], nc[144:288, 1], nc[288:, 0] = 1, -1, 1
    nc[5, 0] = np.nan                                   # one dropped normal
    src = tgt[rng.permutation(tgt.shape[0])[:300]].copy()
    src[:, :3] += rng.integers(-2, 3, (300, 3)).astype(np.float32)
    src[17, 0] = np.nan                                 # a source point that takes no part
    src[40, :3] += 50                                   # one beyond the cap
    max2 = 9.0
    want = [0.0] * 32
    for p in src[:, :3].astype(np.float64):
        if not np.isfinite(p).all():
            continue
        d2 = ((p[None, :] - tgt[:, :3].astype(np.float64)) ** 2).sum(1)
        j = int(np.argmin(d2))                          # the first of equal distances: the lowest index
        want[30] += 1.0
        want[31] += d2[j]
        n = nc[j, :3].astype(np.float64)
        if d2[j] > max2 or not np.isfinite(n).all():
            continue
        q = tgt[j, :3].astype(np.float64)
        row = [p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0], n[0], n[1], n[2]]
        r = (q - p) @ n
        want[0] += 1.0
        k = 1
        for i in range(6):
            for jj in range(i, 6):
                want[k] += row[i] * row[jj]
                k += 1
        for i in range(6):
            want[22 + i] += row[i] * r
        want[28] += r * r
        want[29] += d2[j]
    got = P.sweep_sums(src, tgt, nc, np.float32(max2))
    assert got.shape == (32,) and got.dtype == np.float64
    assert 250 < want[0] < want[30] == 299.0
    assert np.array_equal(got, np.array(want))


def test_plane_result_layout_matches_the_header(S, tmp_path):
    names = ["converged", "iterations", "state", "n_correspondences", "fitness", "plane_fitness", "T", "normal_eq", "first_eq"]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scaloam_hip.h"\nint main(void) {\n'
                   '    printf("%zu %d %.17g", sizeof(scal_icp_plane_result), SCAL_ICP_PLANE_NSUM, SCAL_ICP_PLANE_PIVOT_MIN);\n'
                   + "".join(f'    printf(" %zu", offsetof(scal_icp_plane_result, {n}));\n' for n in names) + '    return 0;\n}\n')
    exe = tmp_path / "sizes"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    R = S.ICPPlaneResult
    from scaloam import icp_plane
    assert [int(got[0]), int(got[1]), float(got[2])] == [C.sizeof(R), icp_plane.NSUM, icp_plane.PIVOT_MIN]
    assert [int(v) for v in got[3:]] == [getattr(R, n).offset for n in names]
    assert [n for n, _ in R._fields_] == names
    assert {"scal_icp_align_plane", "scal_icp_align_plane_device"} <= set(S.EXPORTED_SYMBOLS)
