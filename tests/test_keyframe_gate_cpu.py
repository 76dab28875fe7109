"""scal_keyframe_gate (laserPosegraphOptimization.cpp:598-617), the library's host-only keyframe gate that scal_pipeline's sc_mode 3
runs, against scaloam.pgo.KeyframeGate: no GPU needed.  The two compute the f32 delta transform in different orders (the Python
restatement inverts through numpy), so a decision may only differ where an accumulator lies within 1e-5 of its gap."""
import numpy as np
import pytest

from scaloam.pgo import KeyframeGate as PyGate


def _quat_rpy(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy])


def _walks(seed):
    rng = np.random.default_rng(seed)
    out = []
    # random walk in 6 DoF, steps around the gaps
    t, rpy = np.zeros(3), np.zeros(3)
    for _ in range(1500):
        t = t + rng.normal(0, 0.35, 3)
        rpy = rpy + rng.normal(0, 0.03, 3)
        out.append((_quat_rpy(*rpy), t.copy()))
    # pure yaw, slow spin in place
    for k in range(800):
        out.append((_quat_rpy(0.0, 0.0, 0.013 * k), np.array([5.0, -2.0, 0.3])))
    # roll / pitch wobble while driving straight
    for k in range(800):
        out.append((_quat_rpy(0.08 * np.sin(0.21 * k), 0.06 * np.cos(0.17 * k), 0.4), np.array([0.25 * k, 0.02 * k, 0.0])))
    # getRPY's gimbal-lock branch: pitch at +-90 deg, with and without a non-unit quaternion
    for k in range(300):
        sgn = 1.0 if k % 2 else -1.0
        q = _quat_rpy(0.3 * k, sgn * np.pi / 2, 0.0) * (1.0 + 0.5 * (k % 3))
        out.append((q, np.array([0.1 * k, 0.0, 0.05 * k])))
    return out


@pytest.mark.parametrize("gaps", [(2.0, 10.0), (1.0, 10.0), (0.5, 3.0)])
def test_gate_matches_python_restatement(S, gaps):
    from scaloam.pgo import diff_transformation, rpy_from_quat
    meter_gap, deg_gap = gaps
    poses = _walks(7)
    g, p = S.KeyframeGate(meter_gap, deg_gap), PyGate(meter_gap, deg_gap)
    n_kf = n_cmp = 0
    for k, (q, t) in enumerate(poses):
        # the accumulators this pose's decision compares (before a reset)
        d = diff_transformation(p.curr, (float(t[0]), float(t[1]), float(t[2])) + tuple(rpy_from_quat(q)))
        tr, rot = p.tr + float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])), p.rot + float(d[3] + d[4] + d[5])
        close = abs(tr - meter_gap) <= 1e-5 or abs(rot - np.deg2rad(deg_gap)) <= 1e-5
        a, b = g(q, t), p(q, t)
        if close:  # too close to a gap to call: re-align the library's accumulators and go on
            g.st.translation_accumulated, g.st.rotation_accumulated = p.tr, p.rot
            continue
        assert a == b, (k, tr, rot)
        n_cmp += 1
        n_kf += b
        assert abs(g.st.translation_accumulated - p.tr) <= 1e-4 * max(1.0, p.tr), k
        assert abs(g.st.rotation_accumulated - p.rot) <= 1e-4 * max(1.0, p.rot), k
    assert n_cmp >= len(poses) - 10
    assert 50 < n_kf < len(poses) - 50, n_kf


def test_gate_first_pose_is_keyframe_and_state(S):
    g = S.KeyframeGate(2.0, 10.0)
    assert g.st.translation_accumulated == 1e6 and g.st.rotation_accumulated == 1e6
    assert abs(g.st.rad_gap - np.deg2rad(10.0)) < 1e-15
    assert g([0, 0, 0, 1], [0, 0, 0])
    assert not g([0, 0, 0, 1], [0.5, 0, 0])
    assert not g([0, 0, 0, 1], [1.5, 0, 0])
    assert g([0, 0, 0, 1], [2.6, 0, 0])  # 2.6 m accumulated > 2.0
    assert list(g.st.curr) == [2.6, 0, 0, 0, 0, 0]


def test_gate_rejects_bad_arguments(S):
    import ctypes as C
    L = S.lib()
    st = S.KeyframeGateState()
    for mg, dg in ((-1.0, 10.0), (2.0, -1.0), (float("nan"), 10.0), (2.0, float("inf"))):
        assert L.scal_keyframe_gate_init(C.byref(st), mg, dg) == S.E_ARG
    assert L.scal_keyframe_gate_init(None, 2.0, 10.0) == S.E_ARG
    assert L.scal_keyframe_gate_init(C.byref(st), 2.0, 10.0) == 0
    q, t, k = np.array([0, 0, 0, 1.0]), np.zeros(3), C.c_int(0)
    f64 = C.POINTER(C.c_double)
    assert L.scal_keyframe_gate(C.byref(st), None, t.ctypes.data_as(f64), C.byref(k)) == S.E_ARG
    assert L.scal_keyframe_gate(C.byref(st), q.ctypes.data_as(f64), t.ctypes.data_as(f64), None) == S.E_ARG
    z = np.zeros(4)
    assert L.scal_keyframe_gate(C.byref(st), z.ctypes.data_as(f64), t.ctypes.data_as(f64), C.byref(k)) == S.E_ARG
    bad_t = np.array([np.nan, 0, 0])
    assert L.scal_keyframe_gate(C.byref(st), q.ctypes.data_as(f64), bad_t.ctypes.data_as(f64), C.byref(k)) == S.E_ARG
    # a rejected call leaves the state alone
    assert st.translation_accumulated == 1e6
    assert L.scal_keyframe_gate(C.byref(st), q.ctypes.data_as(f64), t.ctypes.data_as(f64), C.byref(k)) == 0 and k.value == 1
    with pytest.raises(S.ScalError):
        S.KeyframeGate(-2.0, 10.0)
