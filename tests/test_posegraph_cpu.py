"""The pose-graph optimizer's CPU restatement (scaloam.pgo: SE(3) maps, between residual and its analytic Jacobians, the batch
Gauss-Newton loop, the pipeline's graph), which the device optimizer (csrc/posegraph.hip) is held to, and the parts of the
scal_posegraph C-ABI that need no device."""
import ctypes as C

import numpy as np
import pytest

from scaloam import pgo as G


def _random_poses(rng, n, rot, trans=5.0):
    return G.se3_exp(np.concatenate([rng.normal(size=(n, 3)) * rot, rng.normal(size=(n, 3)) * trans], 1))


def test_log_exp_round_trip():
    rng = np.random.default_rng(3)
    w = rng.normal(size=(400, 3))
    w *= (rng.uniform(0, 3.1, 400) / np.linalg.norm(w, axis=1))[:, None]   # rotation angles in [0, 3.1] rad
    w[:100] *= 1e-3       # the series branch of the coefficients
    w[100:150] *= 1e-7    # the series branch of the rotation logarithm
    w[150] = 0
    xi = np.concatenate([w, rng.normal(size=(400, 3)) * 4], 1)
    assert np.abs(G.se3_log(G.se3_exp(xi)) - xi).max() <= 1e-9
    T = G.se3_exp(xi)
    assert np.abs(G.se3_between(T, T)[:, :3]).max() <= 1e-15 and np.abs(G.se3_between(T, T)[:, 4:]).max() <= 1e-12
    assert np.abs(G.se3_log(G.se3_compose(G.se3_inverse(T), T))).max() <= 1e-12


@pytest.mark.parametrize("pose_rot,res", [(1.0, 0.5), (1.0, 1e-3), (1.0, 1e-7), (1.0, 0.0999), (1.0, 0.1001), (1.5708 / np.sqrt(3), 1.5708 / np.sqrt(3))])
def test_between_jacobians_against_central_differences(pose_rot, res):
    """dr/dd_i and dr/dd_j for T <- T Exp(d) against central differences (h = 1e-6: truncation ~1e-12, rounding ~1e-9 for residuals of
    order 1): residual rotations from 1e-7 rad (series branches) over the branch switch at 0.1 rad to about pi/2"""
    rng = np.random.default_rng(11)
    n = 40
    Ti, Tj = _random_poses(rng, n, pose_rot), _random_poses(rng, n, pose_rot)
    xi = rng.normal(size=(n, 6))
    xi[:, :3] *= res / np.linalg.norm(xi[:, :3], axis=1, keepdims=True)
    Z = G.se3_compose(G.se3_between(Ti, Tj), G.se3_exp(xi))
    r, Ji, Jj = G.between_residual(Ti, Tj, Z, True)
    assert abs(np.linalg.norm(r[:, :3], axis=1) - res).max() <= 1e-9
    h, err = 1e-6, 0.0
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        fi = (G.between_residual(G.se3_retract(Ti, d), Tj, Z) - G.between_residual(G.se3_retract(Ti, -d), Tj, Z)) / (2 * h)
        fj = (G.between_residual(Ti, G.se3_retract(Tj, d), Z) - G.between_residual(Ti, G.se3_retract(Tj, -d), Z)) / (2 * h)
        err = max(err, np.abs(fi - Ji[:, :, k]).max(), np.abs(fj - Jj[:, :, k]).max())
    print("max |analytic - central difference|", err)
    assert err <= 1e-7
    P = _random_poses(rng, n, pose_rot)
    rp, Jp = G.prior_residual(G.se3_compose(P, G.se3_exp(xi)), P, True)
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        T = G.se3_compose(P, G.se3_exp(xi))
        f = (G.prior_residual(G.se3_retract(T, d), P) - G.prior_residual(G.se3_retract(T, -d), P)) / (2 * h)
        assert np.abs(f - Jp[:, :, k]).max() <= 1e-7


def test_against_scipy_least_squares():
    """The restatement against scipy.optimize.least_squares (trf, xtol = ftol = gtol = machine epsilon, analytic-free: its own 2-point
    Jacobian) on the whitened residuals of a 30-node graph without robust edges - an independent solver on the same cost.  Poses
    within the 1e-5 pose bar; observed maximum 8.3e-09 (translation and rotation vector over all nodes)."""
    from scipy.optimize import least_squares
    init, prior, edges, _ = G.two_lap_graph(30, 4, seed=5, bad_offset=None)
    edges["k"][:] = 0.0
    x, st = G.optimize_pose_graph(init, prior, edges)
    assert st["converged"] == 1 and all(b <= a for a, b in zip(st["costs"], st["costs"][1:]))

    def fun(d):
        ep, e, _, _ = G.whitened_residuals(G.se3_retract(init, d.reshape(-1, 6)), prior, edges)
        return np.concatenate([ep, e.reshape(-1)])

    eps = np.finfo(float).eps
    sol = least_squares(fun, np.zeros(6 * len(init)), method="trf", xtol=eps, ftol=eps, gtol=eps, x_scale=1.0, max_nfev=400)
    y = G.se3_retract(init, sol.x.reshape(-1, 6))
    diff = G.se3_log(G.se3_between(y, x))
    dmax = max(np.abs(diff).max(), np.abs(y[:, 4:] - x[:, 4:]).max())
    print("max pose difference to least_squares", dmax, "costs", st["final_cost"], sol.cost)
    assert dmax <= 1e-5
    assert abs(st["final_cost"] - sol.cost) <= 1e-9 * max(sol.cost, 1e-3)


def test_two_lap_graph_with_displaced_loop():
    init, prior, edges, bad = G.two_lap_graph(600, 20)
    x, st = G.optimize_pose_graph(init, prior, edges)
    assert st["converged"] == 1 and st["iterations"] < G.PG_DEFAULTS["max_iterations"]
    assert all(b <= a for a, b in zip(st["costs"], st["costs"][1:])) and st["costs"][-1] < st["costs"][0]
    assert st["final_cost"] == st["costs"][-1]
    w = st["weights"][599:]
    print("iterations", st["iterations"], "cost", st["costs"][0], "->", st["costs"][-1], "weights: bad", w[bad], "others >=", np.delete(w, bad).min())
    assert w[bad] < 0.05 and np.delete(w, bad).min() > 0.5
    assert np.all(st["weights"][:599] == 1.0)
    assert np.abs(x[0] - init[0]).max() <= 1e-9      # the 1e-12 prior holds node 0
    # a bound on the iterations: not converged, cost still not above the initial one
    x1, s1 = G.optimize_pose_graph(init, prior, edges, dict(max_iterations=1))
    assert s1["converged"] == 0 and s1["iterations"] == 1 and s1["final_cost"] <= st["costs"][0]


def test_no_loops_stays_put():
    init, prior, edges, _ = G.two_lap_graph(50, 0)
    x, st = G.optimize_pose_graph(init, prior, edges)
    assert st["converged"] == 1 and st["iterations"] <= 1 and np.abs(x - init).max() <= G.PG_DEFAULTS["step_tol"]


def test_build_pipeline_graph_by_hand():
    """three keyframes 1 m apart along x, the third turned by 90 deg about z; one accepted loop 0 -> 2 and one rejected record"""
    p6 = np.array([[0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [2, 0, 0, 0, 0, np.pi / 2]], float)
    s = np.sqrt(0.5)
    loops = [dict(verified=1, curr_kf=2, loop_kf=0, q_rel=[0, 0, s, s], t_rel=[2.1, 0, 0]),
             dict(verified=0, curr_kf=2, loop_kf=1, q_rel=[0, 0, 0, 1], t_rel=[9, 9, 9]),
             dict(verified=-1, curr_kf=1, loop_kf=0, q_rel=[0, 0, 0, 1], t_rel=[9, 9, 9])]
    prior, e = G.build_pipeline_graph(p6, loops)
    assert prior["node"] == 0 and np.allclose(prior["pose7"], [0, 0, 0, 1, 0, 0, 0]) and np.all(prior["var"] == 1e-12)
    assert e["i"].tolist() == [0, 1, 0] and e["j"].tolist() == [1, 2, 2] and e["k"].tolist() == [0, 0, 1]
    assert np.allclose(e["z"][0], [0, 0, 0, 1, 1, 0, 0]) and np.allclose(e["z"][1], [0, 0, s, s, 1, 0, 0]) and np.allclose(e["z"][2], [0, 0, s, s, 2.1, 0, 0])
    assert np.all(e["var"][:2] == [1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4]) and np.all(e["var"][2] == 0.5)
    # the odometry residuals vanish at the gated poses, the loop's is a 0.1 m shift seen from the measured pose (turned by 90 deg: along its y)
    ep, r, w, cost = G.whitened_residuals(G.pose7_from_pose6(p6), prior, e)
    assert np.abs(ep).max() == 0 and np.abs(r[:2]).max() <= 1e-12
    assert np.allclose(r[2] * np.sqrt(0.5), [0, 0, 0, 0, 0.1, 0], atol=1e-12)
    assert np.isclose(w[2], 1 / (1 + 0.02)) and np.isclose(cost, 0.5 * np.log1p(0.02))
    # database indices with two pre-filled entries in front
    for l in loops:
        l["curr_kf"] += 2
        l["loop_kf"] += 2
    _, e2 = G.build_pipeline_graph(p6, loops, kf_ids=[2, 3, 4])
    assert e2["i"].tolist() == [0, 1, 0] and e2["j"].tolist() == [1, 2, 2]
    # pose6 <-> pose7
    back = G.pose6_from_pose7(G.pose7_from_pose6(p6))
    assert np.abs(back - p6).max() <= 1e-12


def test_capi_argument_checks_and_no_device(S):
    """the checks that come before the device is touched; scal_posegraph_create itself answers SCAL_E_NO_DEVICE where there is no GPU"""
    L = S.lib()
    h = C.c_void_p()
    assert L.scal_posegraph_create(None, C.byref(h)) == S.E_ARG
    for cfg in (S.PoseGraphConfig(0, 0, 10), S.PoseGraphConfig(0, 10, -1)):
        assert L.scal_posegraph_create(C.byref(cfg), C.byref(h)) == S.E_ARG
    cfg = S.PoseGraphConfig(0, 100, 200)
    assert L.scal_posegraph_create(C.byref(cfg), None) == S.E_ARG
    rc = L.scal_posegraph_create(C.byref(cfg), C.byref(h))
    if S.device_count() < 1:
        assert rc == S.E_NO_DEVICE and not h.value
        with pytest.raises(S.ScalError) as e:
            S.PoseGraph(100, 200)
        assert e.value.code == S.E_NO_DEVICE
    else:
        assert rc == S.OK and h.value
        L.scal_posegraph_destroy(h)
    z7, z6 = np.zeros(7), np.ones(6)
    f64p = C.POINTER(C.c_double)
    assert L.scal_posegraph_set_nodes(None, z7.ctypes.data_as(f64p), 1) == S.E_ARG
    assert L.scal_posegraph_set_prior(None, 0, z7.ctypes.data_as(f64p), z6.ctypes.data_as(f64p)) == S.E_ARG
    assert L.scal_posegraph_add_between(None, 0, None, None, None, None, None) == S.E_ARG
    assert L.scal_posegraph_clear_edges(None) == S.E_ARG
    assert L.scal_posegraph_optimize(None, None, None) == S.E_ARG
    assert L.scal_posegraph_get_nodes(None, z7.ctypes.data_as(f64p), 1) == S.E_ARG
    assert L.scal_posegraph_get_edge_weights(None, z6.ctypes.data_as(f64p), 0) == S.E_ARG
    assert L.scal_pipeline_optimize_keyframes(None, 0, 0, None, None, 0, None) == S.E_ARG
    L.scal_posegraph_destroy(None)
