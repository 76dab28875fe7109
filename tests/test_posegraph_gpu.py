"""scal_posegraph (csrc/posegraph.hip) against its CPU restatement scaloam.pgo.optimize_pose_graph on the same inputs: poses within the
project's 1e-5 pose bar, final cost within 1e-9 relative (absolute floor 1e-12 for zero-cost graphs), robust weights within 1e-4,
bitwise reproducibility, the iteration bounds and every error path of the header."""
import ctypes as C

import numpy as np
import pytest

from scaloam import pgo as G

pytestmark = pytest.mark.gpu

POSE_BAR = 1e-5


def _device(S, init, prior, edges, g=None, **params):
    own = g is None
    if own:
        g = S.PoseGraph(len(init), len(edges["i"]))
    g.set_nodes(init)
    g.set_prior(prior["node"], prior["pose7"], prior["var"])
    g.clear_edges()
    g.add_edges(edges)
    st = g.optimize(**params)
    x, w = g.nodes(), g.edge_weights()
    if own:
        g.close()
    return x, w, st


def _pose_diff(a, b):
    """max over nodes of |translation difference| and |rotation vector of a^-1 b|"""
    d = G.se3_log(G.se3_between(a, b))
    return max(np.abs(a[:, 4:] - b[:, 4:]).max(), np.abs(d[:, :3]).max())


CASES = {
    "two_lap_600_20": lambda: G.two_lap_graph(600, 20),
    "two_lap_5000_500": lambda: G.two_lap_graph(5000, 500),
    "out_and_back_400_30": lambda: G.out_and_back_graph(400, 30, seed=2, bad_offset=(3.0, 4.0, -1.0)),
    "consistent_600_20": lambda: G.two_lap_graph(600, 20, seed=4, noise=0.0, bad_offset=None, perturb=2e-3),
}


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_restatement(S, name):
    init, prior, edges, bad = CASES[name]()
    ref, rs = G.optimize_pose_graph(init, prior, edges)
    x, w, st = _device(S, init, prior, edges)
    dp = _pose_diff(ref, x)
    dc = abs(st["final_cost"] - rs["final_cost"])
    dw = np.abs(w - rs["weights"]).max()
    print(name, "pose diff", dp, "cost", rs["costs"][0], "->", rs["final_cost"], "device", st["initial_cost"], "->", st["final_cost"], "weight diff", dw,
          "iterations", rs["iterations"], st["iterations"], "linear iterations", st["linear_iterations"], "last step", st["last_step_max"])
    assert rs["converged"] == 1 and st["converged"] == 1 and st["linear_status"] == 0
    assert dp <= POSE_BAR
    assert dc <= max(1e-9 * rs["final_cost"], 1e-12)
    assert abs(st["initial_cost"] - rs["costs"][0]) <= max(1e-9 * rs["costs"][0], 1e-12)
    assert dw <= 1e-4
    assert abs(st["iterations"] - rs["iterations"]) <= 1
    n_odo = len(init) - 1
    assert np.all(w[:n_odo] == 1.0)
    if bad >= 0:
        assert w[n_odo + bad] < 0.05 and np.delete(w[n_odo:], bad).min() > 0.5
    if name.startswith("consistent"):
        assert st["final_cost"] <= 1e-12 and st["initial_cost"] > 1.0


def test_no_loops_stays_at_the_initial_poses(S):
    init, prior, edges, _ = G.two_lap_graph(300, 0)
    x, w, st = _device(S, init, prior, edges)
    assert st["converged"] == 1 and st["iterations"] <= 1
    assert _pose_diff(init, x) <= 1e-8 and np.all(w == 1.0)   # the default step_tol


def test_bitwise_reproducible(S):
    init, prior, edges, _ = G.two_lap_graph(600, 20)
    x0, w0, s0 = _device(S, init, prior, edges)
    x1, w1, s1 = _device(S, init, prior, edges)
    assert np.array_equal(x0, x1) and np.array_equal(w0, w1) and s0 == s1
    # the same object again, and the edges added one by one
    g = S.PoseGraph(len(init), len(edges["i"]))
    x2, w2, s2 = _device(S, init, prior, edges, g=g)
    g.set_nodes(init)
    g.clear_edges()
    for k in range(len(edges["i"])):
        g.add_between(edges["i"][k:k + 1], edges["j"][k:k + 1], edges["z"][k:k + 1], edges["var"][k:k + 1], edges["k"][k:k + 1])
    s3 = g.optimize()
    assert np.array_equal(x0, x2) and np.array_equal(w0, w2) and s0 == s2
    assert np.array_equal(x0, g.nodes()) and np.array_equal(w0, g.edge_weights()) and s0 == s3
    g.close()


def test_iteration_bounds(S):
    init, prior, edges, _ = G.two_lap_graph(600, 20)
    full = _device(S, init, prior, edges)
    g = S.PoseGraph(len(init), len(edges["i"]))
    g.set_nodes(init)
    _, _, _, c0 = G.whitened_residuals(g.nodes(), prior, edges)   # the initial poses as the object holds them (quaternions renormalised)
    for params in (dict(max_iterations=1), dict(max_linear_iterations=1)):
        x, w, st = _device(S, init, prior, edges, g=g, **params)
        _, _, _, c = G.whitened_residuals(x, prior, edges)
        print(params, st, "cost by the restatement", c, "initial", c0)
        assert st["converged"] == 0 and np.all(np.isfinite(x)) and c <= c0
        assert st["iterations"] == 1
        if "max_linear_iterations" in params:
            assert st["linear_status"] == 1 and st["linear_iterations"] == 1 and np.abs(x - init).max() <= 1e-15   # the last accepted poses
        else:
            assert c < c0
    # the object optimises normally afterwards
    x, w, st = _device(S, init, prior, edges, g=g)
    assert np.array_equal(x, full[0]) and st == full[2]
    g.close()


def test_error_paths(S):
    L = S.lib()
    f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int)

    def d(a):
        return np.ascontiguousarray(a, np.float64).ctypes.data_as(f64p)

    def i(a):
        return np.ascontiguousarray(a, np.int32).ctypes.data_as(i32p)

    g = S.PoseGraph(4, 3)
    ident = np.array([0, 0, 0, 1, 0, 0, 0.0])
    P = np.tile(ident, (4, 1))
    P[:, 4] = np.arange(4)
    var = np.ones(6)
    st = S.PoseGraphStats()
    # optimize without nodes / prior
    assert L.scal_posegraph_optimize(g.h, None, C.byref(st)) == S.E_STATE
    # edges and prior before any node: indices out of range
    assert L.scal_posegraph_add_between(g.h, 1, i([0]), i([1]), d(ident), d(var), None) == S.E_ARG
    assert L.scal_posegraph_set_prior(g.h, 0, d(ident), d(var)) == S.E_ARG
    # set_nodes
    assert L.scal_posegraph_set_nodes(g.h, d(P), 0) == S.E_ARG
    assert L.scal_posegraph_set_nodes(g.h, None, 4) == S.E_ARG
    assert L.scal_posegraph_set_nodes(g.h, d(np.tile(ident, (5, 1))), 5) == S.E_CAPACITY
    for bad in (np.nan, np.inf):
        Q = P.copy()
        Q[2, 5] = bad
        assert L.scal_posegraph_set_nodes(g.h, d(Q), 4) == S.E_ARG
    Q = P.copy()
    Q[1, :4] = 0
    assert L.scal_posegraph_set_nodes(g.h, d(Q), 4) == S.E_ARG
    assert L.scal_posegraph_set_nodes(g.h, d(P), 4) == S.OK
    assert L.scal_posegraph_optimize(g.h, None, C.byref(st)) == S.E_STATE   # still no prior
    # set_prior
    for node in (-1, 4):
        assert L.scal_posegraph_set_prior(g.h, node, d(ident), d(var)) == S.E_ARG
    for bad in (0.0, -1.0, np.nan, np.inf):
        v = var.copy()
        v[3] = bad
        assert L.scal_posegraph_set_prior(g.h, 0, d(ident), d(v)) == S.E_ARG
    nan7 = ident.copy()
    nan7[6] = np.nan
    assert L.scal_posegraph_set_prior(g.h, 0, d(nan7), d(var)) == S.E_ARG
    assert L.scal_posegraph_set_prior(g.h, 0, d(ident), d(var)) == S.OK
    # add_between
    step = np.array([0, 0, 0, 1, 1, 0, 0.0])
    for a, b in ((0, 0), (-1, 1), (0, 4), (4, 0)):
        assert L.scal_posegraph_add_between(g.h, 1, i([a]), i([b]), d(step), d(var), None) == S.E_ARG
    assert L.scal_posegraph_add_between(g.h, 1, i([0]), i([1]), d(nan7), d(var), None) == S.E_ARG
    for bad in (0.0, -2.0, np.nan):
        v = var.copy()
        v[0] = bad
        assert L.scal_posegraph_add_between(g.h, 1, i([0]), i([1]), d(step), d(v), None) == S.E_ARG
    for bad in (-1.0, np.nan, np.inf):
        assert L.scal_posegraph_add_between(g.h, 1, i([0]), i([1]), d(step), d(var), d([bad])) == S.E_ARG
    assert L.scal_posegraph_add_between(g.h, -1, None, None, None, None, None) == S.E_ARG
    # all or nothing: the second edge is bad, nothing is added
    assert L.scal_posegraph_add_between(g.h, 2, i([0, 1]), i([1, 1]), d(np.tile(step, (2, 1))), d(np.tile(var, (2, 1))), None) == S.E_ARG
    w = np.zeros(3)
    assert L.scal_posegraph_get_edge_weights(g.h, d(w), 0) == S.E_STATE   # nothing optimised yet
    assert L.scal_posegraph_add_between(g.h, 3, i([0, 1, 2]), i([1, 2, 3]), d(np.tile(step, (3, 1))), d(np.tile(var, (3, 1))), None) == S.OK
    assert L.scal_posegraph_add_between(g.h, 1, i([0]), i([3]), d(step), d(var), None) == S.E_CAPACITY
    assert L.scal_posegraph_get_edge_weights(g.h, d(w), 3) == S.E_STATE
    # parameters
    for prm in (S.PoseGraphParams(-1, 0, 0, 0), S.PoseGraphParams(0, -1.0, 0, 0), S.PoseGraphParams(0, 0, -1, 0), S.PoseGraphParams(0, 0, 0, float("nan"))):
        assert L.scal_posegraph_optimize(g.h, C.byref(prm), C.byref(st)) == S.E_ARG
    assert L.scal_posegraph_optimize(g.h, None, C.byref(st)) == S.OK and st.converged == 1 and st.final_cost <= 1e-20
    out = np.zeros((4, 7))
    assert L.scal_posegraph_get_nodes(g.h, d(out), 3) == S.E_ARG
    assert L.scal_posegraph_get_nodes(g.h, None, 4) == S.E_ARG
    outp = out.ctypes.data_as(f64p)
    assert L.scal_posegraph_get_nodes(g.h, outp, 4) == S.OK and np.abs(out - P).max() <= 1e-12
    wp = w.ctypes.data_as(f64p)
    assert L.scal_posegraph_get_edge_weights(g.h, wp, 2) == S.E_ARG
    assert L.scal_posegraph_get_edge_weights(g.h, wp, 3) == S.OK and np.all(w == 1.0)
    # fewer nodes than the edges name: optimize refuses
    assert L.scal_posegraph_set_nodes(g.h, d(P[:3]), 3) == S.OK
    assert L.scal_posegraph_optimize(g.h, None, C.byref(st)) == S.E_STATE
    assert L.scal_posegraph_clear_edges(g.h) == S.OK
    # nodes that no factor holds: the system is singular, which is reported as a solve that did not converge, not as a fault
    assert L.scal_posegraph_optimize(g.h, None, C.byref(st)) == S.OK and st.converged == 0 and st.linear_status == 2
    assert L.scal_posegraph_set_nodes(g.h, d(P[:1]), 1) == S.OK
    assert L.scal_posegraph_optimize(g.h, None, C.byref(st)) == S.OK and st.converged == 1
    assert L.scal_posegraph_get_edge_weights(g.h, wp, 0) == S.OK
    g.close()
