"""The pose-graph optimizer's CPU restatement (scaloam.pgo: SE(3) maps, between residual and its analytic Jacobians, the batch
Gauss-Newton loop, the pipeline's graph), which the device optimizer (csrc/posegraph.hip) is held to, and the parts of the
scal_posegraph C-ABI that need no device."""
import ctypes as C

import numpy as np
import pytest

import posegraph_cases as PC
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


# ---------------------------------------------------------------------------------------------- the restated linear solver
# (pgo.normal_blocks / pcr_factor / pcr_solve / pcg_solve: what csrc/posegraph.hip's solve() does, in numpy) and the properties of the
# small graphs that tests/test_posegraph_small_gpu.py relies on.
CASES = PC.cases()
ALL_CASES = {**CASES["one_step"], **CASES["variants"], **CASES["chains"], **CASES["damping"]}


def _pose_diff(a, b):
    d = G.se3_log(G.se3_between(a, b))
    return max(np.abs(a[:, 4:] - b[:, 4:]).max(), np.abs(d[:, :3]).max())


def _angles(init, edges):
    r = G.between_residual(init[edges["i"]], init[edges["j"]], edges["z"])
    return np.linalg.norm(r[:, :3], axis=1)


def test_normal_blocks_are_the_normal_equations():
    """H and g in blocks against J^T J and J^T b assembled densely from whitened_residuals, with and without damping; blocks_matvec"""
    init, prior, edges = PC.small_graph(9, 2, 0.3, "parallel_loop_reversed")
    n, m = len(init), len(edges["i"])
    ep, e, w, _, Jp, Ji, Jj = G.whitened_residuals(init, prior, edges, True)
    J, b = np.zeros((6 * m + 6, 6 * n)), np.concatenate([ep, (e * np.sqrt(w)[:, None]).reshape(-1)])
    J[:6, 6 * prior["node"]:6 * prior["node"] + 6] = Jp
    for k in range(m):
        J[6 * k + 6:6 * k + 12, 6 * edges["i"][k]:6 * edges["i"][k] + 6] = Ji[k] * np.sqrt(w[k])
        J[6 * k + 6:6 * k + 12, 6 * edges["j"][k]:6 * edges["j"][k] + 6] = Jj[k] * np.sqrt(w[k])
    Hd = J.T @ J
    for lam in (0.0, 1e-4):
        H, g = G.normal_blocks(init, prior, edges, lam)
        want = Hd + lam * np.diag(np.diag(Hd))
        assert np.abs(G.blocks_dense(H) - want).max() <= 1e-12 * np.abs(want).max()
        assert np.abs(g.reshape(-1) - J.T @ b).max() <= 1e-12 * np.abs(J.T @ b).max()
        p = np.random.default_rng(0).normal(size=(n, 6))
        assert np.abs(G.blocks_matvec(H, p).reshape(-1) - want @ p.reshape(-1)).max() <= 1e-12 * np.abs(want @ p.reshape(-1)).max()
    # M keeps the parallel loop edge's block and drops the other loops'
    M = G.blocks_dense(H, tridiagonal=True).reshape(n, 6, n, 6)
    A = G.blocks_dense(H).reshape(n, 6, n, 6)
    for a in range(n):
        for c in range(n):
            assert np.array_equal(M[a, :, c, :], A[a, :, c, :] if abs(a - c) <= 1 else np.zeros((6, 6)))


@pytest.mark.parametrize("n", [1, 2, 3, 6, 7, 8, 9, 14, 15, 32, 33, 100])
def test_pcr_against_a_dense_solve(n):
    """pcr_solve(pcr_factor(H), r) against numpy's dense solve of the block-tridiagonal part, on a looped graph (M != H) where n
    allows loops: relative error <= 1e-6 of |solution|_inf (observed <= 3.2e-12 at cond(H) up to 4e12)"""
    init, prior, edges = PC.prior_only_graph() if n == 1 else PC.small_graph(n, {1: 0, 2: 0}.get(n, max(1, n // 8)), 0.3, "prior_middle" if n % 2 else "plain")
    H, _ = G.normal_blocks(init, prior, edges)
    F = G.pcr_factor(H)
    assert len(F["levels"]) == int(np.ceil(np.log2(n))) if n > 1 else len(F["levels"]) == 0
    r = np.random.default_rng(n).normal(size=(n, 6))
    want = np.linalg.solve(G.blocks_dense(H, tridiagonal=True), r.reshape(-1)).reshape(n, 6)
    err = np.abs(G.pcr_solve(F, r) - want).max() / np.abs(want).max()
    print("n", n, "relative error", err)
    assert err <= 1e-6


@pytest.mark.parametrize("name", list(CASES["chains"]))
def test_chain_only_graphs_need_at_most_two_pcg_iterations(name):
    init, prior, edges = PC.small_graph(*CASES["chains"][name])
    H, g = G.normal_blocks(init, prior, edges)
    d, its, status = G.pcg_solve(H, g)
    assert status == 0 and 1 <= its <= 2
    assert _angles(init, edges).min() >= 0.1


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_pcg_against_a_dense_solve(name):
    """the first system of every small graph: pcg_solve within 1e-8 (the optimizer's step_tol) of numpy's dense solve; observed
    <= 4.7e-10"""
    init, prior, edges = PC.small_graph(*ALL_CASES[name])
    H, g = G.normal_blocks(init, prior, edges)
    d, its, status = G.pcg_solve(H, g)
    want = np.linalg.solve(G.blocks_dense(H), -g.reshape(-1)).reshape(-1, 6)
    print(name, "iterations", its, "max |d_pcg - d_dense|", np.abs(d - want).max(), "max |d|", np.abs(want).max())
    assert status == 0 and np.abs(d - want).max() <= 1e-8


def test_pcg_reports_the_bound_and_a_breakdown():
    init, prior, edges = PC.small_graph(33, 4, 0.3)
    H, g = G.normal_blocks(init, prior, edges)
    d, its, status = G.pcg_solve(H, g, max_iterations=2)
    assert (its, status) == (2, 1)
    d, its, status = G.pcg_solve(H, np.zeros_like(g))
    assert (its, status) == (0, 0) and not d.any()
    H["O"][-1] *= 1e4     # a loop's off-diagonal block that its nodes' diagonal blocks do not cover: H is indefinite, M is not
    assert G.pcg_solve(H, g)[2] == 2


@pytest.mark.parametrize("name", list(CASES["one_step"]))
def test_one_step_inputs(name):
    """what the device's one-step tests assume of their graphs: the first Gauss-Newton step is accepted with room (trial cost <= 0.99 x
    the cost), the pcg restatement makes the same step as splu within 1e-8 (observed <= 2.7e-10), perturb 0.3 has every residual angle
    on the closed-form side of 0.1 rad and perturb 0.05 has angles below it"""
    n, loops, perturb, _, _ = CASES["one_step"][name]
    init, prior, edges = PC.small_graph(*CASES["one_step"][name])
    x, s = G.optimize_pose_graph(init, prior, edges, dict(max_iterations=1))
    xp, sp = G.optimize_pose_graph(init, prior, edges, dict(max_iterations=1, linear="pcg"))
    assert not s["rejected"] and not sp["rejected"] and s["final_cost"] <= 0.99 * s["costs"][0]
    assert _pose_diff(x, xp) <= 1e-8 and sp["linear_status"] == 0 and sp["linear_iterations"] >= 1
    a = _angles(init, edges)
    if n == 1:      # no between edge: the prior's own residual is on the closed-form side
        assert np.linalg.norm(G.prior_residual(init[0], prior["pose7"])[:3]) >= 0.1
    elif perturb == 0.3:
        assert a.min() >= 0.1
    else:
        assert a.min() < 0.1


def test_mixed_case_has_angles_on_both_sides_of_the_switch():
    init, prior, edges = PC.small_graph(33, 4, 0.05)
    a = _angles(init, edges)
    assert (a < 0.1).sum() >= 5 and (a >= 0.1).sum() >= 5


def test_damping_case_rejects_its_first_step():
    """33 nodes, 4 loops, perturb 0.5, seed 1: the first step raises the cost from 4.90e7 to 8.92e7 (1.82 x, no knife edge), the run
    converges all the same, to the optimum of the perturb 0.3 graph (same seed: same measurements); pcg makes the same decisions"""
    init, prior, edges = PC.small_graph(*CASES["damping"][PC.DAMPING_CASE])
    x1, s1 = G.optimize_pose_graph(init, prior, edges, dict(max_iterations=1))
    assert len(s1["rejected"]) == 1 and s1["rejected"][0][1] >= 1.01 * s1["rejected"][0][0]
    assert np.array_equal(x1, init) and s1["converged"] == 0 and s1["final_cost"] == s1["costs"][0] and s1["iterations"] == 1
    x, s = G.optimize_pose_graph(init, prior, edges)
    xp, sp = G.optimize_pose_graph(init, prior, edges, dict(linear="pcg"))
    assert s["converged"] == 1 and sp["converged"] == 1 and s["iterations"] == sp["iterations"] == 9
    assert s["rejected"][0][1] >= 1.01 * s["rejected"][0][0] and sp["rejected"][0][1] >= 1.01 * sp["rejected"][0][0]
    assert _pose_diff(x, xp) <= 1e-7
    y, t = G.optimize_pose_graph(*PC.small_graph(33, 4, 0.3))
    assert _pose_diff(x, y) <= 1e-7 and abs(s["final_cost"] - t["final_cost"]) <= 1e-9 * t["final_cost"]


@pytest.mark.parametrize("variant,noise", [("loops_reversed", 0.0), ("odometry_alternate_reversed", 0.0), ("parallel_loop_reversed", 0.0),
                                           ("interleaved", 0.0), ("interleaved", 1.0)])
def test_reversed_and_reordered_forms_have_the_same_optimum(variant, noise):
    """(i, j, Z) -> (j, i, Z^-1) and another add order leave the restatement's optimum where it was, within 1e-9.  A reversed edge's
    residual is -Ad(Z) r - the same zero, another whitened norm - so the reversed forms are compared on the consistent graph (noise 0:
    every residual vanishes at the optimum); with noise the optimum itself moves, by 6.6e-6 (loops) and 1.2e-4 (odometry) here.
    parallel_loop_reversed is compared with parallel_loop."""
    plain = "parallel_loop" if variant.startswith("parallel") else "plain"
    x, s = G.optimize_pose_graph(*PC.small_graph(33, 4, 0.3, plain, noise))
    y, t = G.optimize_pose_graph(*PC.small_graph(33, 4, 0.3, variant, noise))
    print(variant, noise, "pose difference", _pose_diff(x, y), "iterations", s["iterations"], t["iterations"])
    assert s["converged"] == 1 and t["converged"] == 1
    assert _pose_diff(x, y) <= 1e-9
    if "reversed" in variant:   # the first residuals: -Ad(Z) r
        init, prior, e0 = PC.small_graph(33, 4, 0.3, plain, noise)
        _, _, e1 = PC.small_graph(33, 4, 0.3, variant, noise)
        r0 = G.between_residual(init[e0["i"]], init[e0["j"]], e0["z"])
        r1 = G.between_residual(init[e1["i"]], init[e1["j"]], e1["z"])
        rev = e0["i"] != e1["i"]
        assert rev.any() and np.array_equal(e0["i"][rev], e1["j"][rev])
        want = -np.einsum("eij,ej->ei", G.se3_adjoint(e0["z"][rev]), r0[rev])
        assert np.abs(r1[rev] - want).max() <= 1e-9 * np.abs(want).max() and np.array_equal(r0[~rev], r1[~rev])


@pytest.mark.parametrize("name", [k for k, v in ALL_CASES.items() if v[1] > 0])
def test_looped_runs_decide_with_room_at_the_counting_step_tol(name):
    """The device's count of CG iterations is compared with the restatement's over whole runs, which holds only while both make the
    same accept / reject decisions and end on the same step.  At the default step_tol the last steps change the cost by parts in
    1e13: rounding decides (a cost of 0.04 summed from whitened residuals of order 0.1, each known to about 1e-12, is known to a few
    parts in 1e10).  At COUNTING_STEP_TOL = 1e-5 every decision that a count depends on (steps >= the tolerance; the ending step's
    own decision changes no count) has a relative margin >= 1e-9 - observed >= 3.8e-8 - and no step is within 10 % of the tolerance."""
    init, prior, edges = PC.small_graph(*ALL_CASES[name])
    tol = PC.COUNTING_STEP_TOL
    x, s = G.optimize_pose_graph(init, prior, edges, dict(step_tol=tol, linear="pcg"))
    y, t = G.optimize_pose_graph(init, prior, edges, dict(step_tol=tol))
    assert s["converged"] == 1 and s["linear_status"] == 0 and t["iterations"] == s["iterations"]
    margins = [abs(cn - c) / c for c, cn, step, ok in s["trials"] if step >= tol]
    print(name, "iterations", s["iterations"], "linear", s["linear_iterations"], "smallest margin", min(margins))
    assert min(margins) >= 1e-9
    assert all(not (0.9 * tol <= step <= 1.1 * tol) for _, _, step, _ in s["trials"])
    assert s["trials"][-1][2] < tol and all(step >= tol for _, _, step, _ in s["trials"][:-1])
