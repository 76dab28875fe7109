"""scal_reloc_* and its companions without a GPU: struct layouts against the header's own, the argument checks that precede the device,
SCAL_E_NO_DEVICE where there is none, the host arithmetic of the query (yaw guess, submap transforms), and the premise of the yaw
guess on the CPU oracle alone."""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _cfg(S, **kw):
    v = dict(max_keyframes=4, max_points=1000, max_query_points=1000)
    v.update(kw)
    return S.RelocConfig(**v)


def test_reloc_struct_layouts_match_the_header(S, tmp_path):
    src = tmp_path / "sizes.c"
    fields_a = ["max_query_points", "sc_max_radius", "float_math", "leaf", "submap_half", "fitness_thres", "max_corr_dist", "fitness_epsilon",
                "max_iterations", "no_yaw_guess", "device"]
    fields_b = ["status", "n_src", "n_tgt", "icp", "pose12"]
    args = ["sizeof(scal_reloc_config)"] + [f"offsetof(scal_reloc_config, {f})" for f in fields_a]
    args += ["sizeof(scal_reloc_result)"] + [f"offsetof(scal_reloc_result, {f})" for f in fields_b]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scaloam_hip.h"\nint main(void) {\n'
                   + "".join(f'    printf("%zu ", (size_t)({a}));\n' for a in args) + '    printf("\\n");\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    A, B = S.RelocConfig, S.RelocResult
    assert got == [C.sizeof(A)] + [getattr(A, f).offset for f in fields_a] + [C.sizeof(B)] + [getattr(B, f).offset for f in fields_b]


def test_reloc_argument_checks_and_no_device(S):
    L = S.lib()
    h = C.c_void_p()
    assert L.scal_reloc_create(None, C.byref(h)) == S.E_ARG
    for bad in (dict(max_keyframes=0), dict(max_points=0), dict(max_query_points=0), dict(max_query_points=-3), dict(leaf=-0.4),
                dict(leaf=float("nan")), dict(submap_half=-2), dict(fitness_thres=float("nan")), dict(max_corr_dist=-1.0),
                dict(sc_dist_thres=float("nan")), dict(max_iterations=-1)):
        cfg = _cfg(S, **bad)
        assert L.scal_reloc_create(C.byref(cfg), C.byref(h)) == S.E_ARG, bad
        assert b"scal_reloc_create" in L.scal_last_error()
    cfg = _cfg(S)
    assert L.scal_reloc_create(C.byref(cfg), None) == S.E_ARG
    rc = L.scal_reloc_create(C.byref(cfg), C.byref(h))
    if S.device_count() < 1:
        assert rc == S.E_NO_DEVICE and not h.value
        with pytest.raises(S.ScalError) as e:
            S.Relocalizer(4, 1000, 1000)
        assert e.value.code == S.E_NO_DEVICE
    else:
        assert rc == S.OK and h.value
        assert L.scal_reloc_size(h) == 0 and L.scal_reloc_sc(h)
        L.scal_reloc_destroy(h)
    # null contexts are refused before anything touches a device
    res = S.RelocResult()
    P = np.zeros(12)
    off = np.zeros(2, np.int32)
    assert L.scal_reloc_query(None, None, 0, C.byref(res)) == S.E_ARG
    assert L.scal_reloc_query_batch(None, None, off.ctypes.data_as(C.POINTER(C.c_int)), 1, C.byref(res)) == S.E_ARG
    assert L.scal_reloc_add_keyframe(None, None, 0, P.ctypes.data_as(C.POINTER(C.c_double)), None) == S.E_ARG
    assert L.scal_reloc_size(None) == S.E_ARG and not L.scal_reloc_sc(None)
    L.scal_reloc_destroy(None)
    sr = S.SCResult()
    d = np.zeros(1200)
    dp = d.ctypes.data_as(C.POINTER(C.c_double))
    ip = off.ctypes.data_as(C.POINTER(C.c_int))
    assert L.scal_sc_detect_between(None, dp, 1, C.byref(sr)) == S.E_ARG
    assert L.scal_sc_detect_between_device(None, None, 1, C.byref(sr)) == S.E_ARG
    assert L.scal_sc_cross_matrix(None, None, 0, 1, 0, 1, 0, dp, ip) == S.E_ARG
    assert L.scal_sc_cross_search(None, None, 0, 1, 3, 2, ip, dp, ip) == S.E_ARG
    # a guess is checked before the context: not finite, or a last row other than 0 0 0 1
    ir = S.ICPResult()
    g = np.eye(4, dtype=np.float32)
    for bad in ((0, 3, np.nan), (1, 1, np.inf), (3, 3, 2.0), (3, 0, 1.0)):
        b = g.copy()
        b[bad[0], bad[1]] = bad[2]
        assert L.scal_icp_align_guess(None, None, 0, None, 0, b.ctypes.data_as(C.POINTER(C.c_float)), C.byref(ir)) == S.E_ARG
        assert b"guess" in L.scal_last_error()
        assert L.scal_icp_align_guess_device(None, None, 0, None, 0, b.ctypes.data_as(C.POINTER(C.c_float)), C.byref(ir)) == S.E_ARG
    assert L.scal_icp_align_guess(None, None, 0, None, 0, g.ctypes.data_as(C.POINTER(C.c_float)), C.byref(ir)) == S.E_ARG
    assert b"scal_icp_align" in L.scal_last_error()


def test_yaw_guess_sign_and_rounding(S):
    """G = Rz(-yaw): it undoes a turn of the query by +yaw about z; its entries are cos / sin of the f32 yaw, taken in double, rounded to f32"""
    for shift in (0, 1, 15, 16, 30, 40, 59):
        yaw = np.float32(np.float32(shift * 6.0) * np.pi / 180.0)  # scal_sc_result::yaw_rad
        G = S.yaw_guess(yaw)
        assert G.dtype == np.float32 and np.array_equal(G[2:], np.eye(4, dtype=np.float32)[2:]) and np.array_equal(G[:2, 2:], np.zeros((2, 2), np.float32))
        c, s = np.float32(np.cos(np.float64(yaw))), np.float32(np.sin(np.float64(yaw)))
        assert np.array_equal(G[:2, :2], np.array([[c, s], [-s, c]], np.float32))
        th = np.float64(yaw)
        Rz = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
        assert np.abs(G[:3, :3].astype(np.float64) @ Rz - np.eye(3)).max() < 1e-7
    assert np.array_equal(S.yaw_guess(np.float32(0.0)), np.eye(4, dtype=np.float32))  # shift 0: the identity, today's ICP path


def _term_by_term(Pc, Pj):
    """the f64 value before the rounding, one scalar operation at a time"""
    Pc, Pj = Pc.reshape(3, 4), Pj.reshape(3, 4)
    ref = np.zeros((3, 4))
    for r in range(3):
        ti = -((Pc[0, r] * Pc[0, 3] + Pc[1, r] * Pc[1, 3]) + Pc[2, r] * Pc[2, 3])
        for k in range(4):
            v = (Pc[0, r] * Pj[0, k] + Pc[1, r] * Pj[1, k]) + Pc[2, r] * Pj[2, k]
            ref[r, k] = v + ti if k == 3 else v
    return ref


def test_relative_transform_replay(S, golden):
    """M_j = P_c^-1 P_j with the inverse taken as R^T, -(R^T t) and every sum left to right in f64, then one rounding to f32.  For rigid
    poses (rotations orthonormal to f64) that is numpy's inverse within 1e-12; the golden poses went through optimized_poses.txt's six
    significant digits, their rotations are orthonormal to about 1e-6 only and R^T is the inverse to that much - which is what the
    library documents and the reference's own tools assume of that file - so for them the replay is held term by term."""
    def P4(p):
        M = np.eye(4)
        M[:3] = p.reshape(3, 4)
        return M
    rng = np.random.default_rng(5)
    rigid = []
    for _ in range(6):
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        Q *= np.sign(np.linalg.det(Q))
        rigid.append(np.concatenate([Q, rng.uniform(-1000, 1000, (3, 1))], 1).reshape(12))
    for c, j in ((0, 1), (1, 0), (2, 3), (4, 5), (5, 5)):
        M = S.relative_transform(rigid[c], rigid[j])
        want = (np.linalg.inv(P4(rigid[c])) @ P4(rigid[j]))[:3]
        ref = _term_by_term(rigid[c], rigid[j])
        assert np.abs(ref - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
        assert M.dtype == np.float32 and M.shape == (3, 4) and np.array_equal(M, ref.astype(np.float32))
    poses = golden("KAIST03_poses21.npy").reshape(-1, 12).astype(np.float64)
    for c, j in ((7, 0), (7, 20), (0, 20), (20, 7), (5, 5)):
        M = S.relative_transform(poses[c], poses[j])
        want = (np.linalg.inv(P4(poses[c])) @ P4(poses[j]))[:3]
        assert np.array_equal(M, _term_by_term(poses[c], poses[j]).astype(np.float32))
        assert np.abs(M - want).max() <= 1e-5 * max(1.0, np.abs(want).max())  # the six digits of the pose file


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_identity_start_fails_at_90_degrees_on_the_oracle(S, O, golden):
    """The premise of the yaw guess, on the CPU oracle alone.  Session: golden KAIST03 keyframes 0 / 7 / 20 at the 0.4 m leaf, brought
    into keyframe 7's frame each by its own golden pose and filtered again (32,853 points); query: keyframe 5 turned by 90 degrees;
    the reference's ICP settings.  From the identity the alignment runs into the iteration cap with fitness 22.6, 26.5 m from the
    golden relative pose; started from Rz(-90 deg) - the source pre-moved by the guess - it ends with fitness 0.271, 0.021 m and 0.10
    degrees from it.  The identity-start answer is also what tests/golden/reloc_premise_oracle.npz records for the GPU test."""
    fx = _tool("make_reloc_fixture")  # the clouds are built where the record of the GPU test is: one definition of the case
    poses = golden("KAIST03_poses21.npy").reshape(-1, 12).astype(np.float64)
    src, tgt = fx.premise_clouds()
    assert tgt.shape[0] == 32853

    def P4(p):
        M = np.eye(4)
        M[:3] = p.reshape(3, 4)
        return M
    rel = np.linalg.inv(P4(poses[7])) @ P4(poses[5])  # keyframe 5 in keyframe 7's frame
    Rz = np.eye(4)
    Rz[:2, :2] = [[0.0, -1.0], [1.0, 0.0]]
    want = rel @ np.linalg.inv(Rz)                     # the turned query -> keyframe 7's frame
    r = O.icp_align(src, tgt)
    assert r["fitness"] > 1.0 and np.linalg.norm(r["T"][:3, 3] - want[:3, 3]) > 10.0
    rec = golden("reloc_premise_oracle.npz")
    assert int(rec["n_src"]) == src.shape[0] and int(rec["n_tgt"]) == tgt.shape[0]
    assert int(rec["iterations"]) == r["iterations"] and int(rec["state"]) == r["state"] and bool(rec["converged"]) == r["converged"]
    assert np.abs(rec["T"] - r["T"]).max() <= 1e-6 and abs(float(rec["fitness"]) - r["fitness"]) <= 1e-6 * r["fitness"]
    G = S.yaw_guess(np.float32(np.float32(15 * 6.0) * np.pi / 180.0))
    g = O.icp_align(fx.apply34(G[:3], src), tgt)
    T = g["T"] @ G.astype(np.float64)
    ang = np.degrees(np.arccos(np.clip((np.trace(T[:3, :3] @ want[:3, :3].T) - 1) / 2, -1, 1)))
    assert g["converged"] and g["fitness"] <= 0.3 and np.linalg.norm(T[:3, 3] - want[:3, 3]) <= 0.1 and ang <= 0.5


def test_relocalize_session_tool_checks_its_session_before_the_device(S, tmp_path):
    """tools/relocalize_session.py on the CPU: a session whose Scans/ and optimized_poses.txt disagree is refused with a message, a
    consistent one gets as far as the device - and without one says so (SCAL_E_NO_DEVICE) instead of writing poses"""
    from scaloam import formats
    tool = os.path.join(ROOT, "tools", "relocalize_session.py")
    ses = tmp_path / "session"
    (ses / "Scans").mkdir(parents=True)
    cloud = np.random.default_rng(3).uniform(-20, 20, (500, 4)).astype(np.float32)
    for k in range(2):
        formats.write_pcd_binary(str(ses / "Scans" / f"{k:06d}.pcd"), cloud)
    formats.write_pcd_binary(str(tmp_path / "q.pcd"), cloud)
    formats.write_poses(str(ses / "optimized_poses.txt"), np.tile(np.eye(4)[:3].reshape(1, 12), (3, 1)))  # three poses, two clouds
    r = subprocess.run([sys.executable, tool, str(ses), str(tmp_path / "q.pcd"), "--out", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode != 0 and "2 keyframe clouds" in r.stderr and "3 poses" in r.stderr
    formats.write_poses(str(ses / "optimized_poses.txt"), np.tile(np.eye(4)[:3].reshape(1, 12), (2, 1)))
    r = subprocess.run([sys.executable, tool, str(ses), str(tmp_path / "q.pcd"), "--out", str(tmp_path)], capture_output=True, text=True)
    if S.device_count() < 1:
        assert r.returncode != 0 and "error -7" in r.stderr and not (tmp_path / "relocalized_poses.txt").exists()
    else:
        assert r.returncode == 0, r.stderr
        out = json.loads(r.stdout)
        assert out["keyframes"] == 2 and out["queries"] == 1 and out["accepted"] + out["rejected"] + out["no_place"] == 1
