"""scal_posegraph (csrc/posegraph.hip) on small graphs (1 to 200 nodes) where test_posegraph_gpu.py's four large ones leave it
unobserved: the closed-form branches of pg_coeffs (every residual angle above 0.1 rad), one Gauss-Newton step on its own (a Jacobian
error shows at first order there; converged runs correct it), the PCR preconditioner through the count of CG iterations, edges
entered from either end and in any order, the prior on any node, a rejected step (Levenberg damping), quaternions of either sign and
one context used for graphs of several sizes.  The yardstick is scaloam.pgo: optimize_pose_graph with its exact splu solve for the
poses, and its restatement of the device's own linear solver (pcg_solve, linear="pcg") for the iteration counts.  The graphs and
what the bars below assume of them are checked without a device in test_posegraph_cpu.py.

Bars: ONE_STEP_BAR 1e-8 is the optimizer's own step_tol - two solvers that agree below it are the same solver to the optimizer; the
restated PCG is within 4.7e-10 of the dense solve on these graphs.  POSE_BAR 1e-5, cost 1e-9 relative, weights 1e-4 and iterations
+-1 are test_posegraph_gpu.py's.  CG iterations: the restatement's count + 1 for one solve of a chain-only graph, + 2 per
Gauss-Newton iteration over a run - a last-bit difference in the stop test, no more; a broken PCR level costs tens."""
import functools

import numpy as np
import pytest

import posegraph_cases as PC
from scaloam import pgo as G

pytestmark = pytest.mark.gpu

POSE_BAR = 1e-5
ONE_STEP_BAR = 1e-8
CASES = PC.cases()
ALL_CASES = {**CASES["one_step"], **CASES["variants"], **CASES["chains"], **CASES["damping"]}
LOOPED = [k for k, v in ALL_CASES.items() if v[1] > 0]


@functools.lru_cache(maxsize=None)
def _graph(name):
    return PC.small_graph(*ALL_CASES[name])


@functools.lru_cache(maxsize=None)
def _restated(name, **params):
    """the restatement's result on a case, computed once per set of parameters and left unchanged"""
    init, prior, edges = _graph(name)
    return G.optimize_pose_graph(init, prior, edges, dict(params))


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


def _weight_diff(w, ref):
    return np.abs(w - ref).max() if len(ref) else 0.0


def _close(a, b, rel=1e-9, floor=1e-12):
    return abs(a - b) <= max(rel * abs(b), floor)


@pytest.mark.parametrize("name", list(CASES["one_step"]))
def test_one_gauss_newton_step(S, name):
    """max_iterations = 1 against the restatement's one step with the exact solve.  The step is accepted on both sides (with room:
    test_one_step_inputs), so the returned poses are the step.  A chain-only graph's system is square: its step solves
    Jr^-1(r) (d_j - Ad d_i) = -r edge by edge, and Jr^-1(r) r = r whatever c, c2 and c3 are, so those cases hold the residual (Log,
    with its own c), Ad, the assembly and the solve; the looped cases hold Jr^-1 to its coefficients, the tight_loops ones (loops
    that weigh what the odometry does) in the step's leading digits.  Figures: DESIGN.md section 8.7."""
    init, prior, edges = _graph(name)
    ref, rs = _restated(name, max_iterations=1)
    x, w, st = _device(S, init, prior, edges, max_iterations=1)
    dp, dw = _pose_diff(ref, x), _weight_diff(w, rs["weights"])
    print(name, "pose diff", dp, "step", rs["step_norms"], "cost", rs["costs"][0], "->", rs["final_cost"], "device", st["initial_cost"], "->",
          st["final_cost"], "weight diff", dw, "linear iterations", st["linear_iterations"])
    assert st["iterations"] == 1 and st["linear_status"] == 0 and st["final_cost"] < st["initial_cost"]
    assert _pose_diff(init, x) >= 1e-3      # the step was taken
    assert dp <= ONE_STEP_BAR
    assert _close(st["initial_cost"], rs["costs"][0])
    assert dw <= 1e-4


@pytest.mark.parametrize("name", list({**CASES["one_step"], **CASES["variants"]}))
def test_converged_against_the_restatement(S, name):
    init, prior, edges = _graph(name)
    ref, rs = _restated(name)
    x, w, st = _device(S, init, prior, edges)
    dp, dw = _pose_diff(ref, x), _weight_diff(w, rs["weights"])
    print(name, "pose diff", dp, "cost", rs["costs"][0], "->", rs["final_cost"], "device", st["initial_cost"], "->", st["final_cost"], "weight diff", dw,
          "iterations", rs["iterations"], st["iterations"], "linear iterations", st["linear_iterations"], "last step", st["last_step_max"])
    assert rs["converged"] == 1 and st["converged"] == 1 and st["linear_status"] == 0
    assert dp <= POSE_BAR
    assert _close(st["final_cost"], rs["final_cost"]) and _close(st["initial_cost"], rs["costs"][0])
    assert dw <= 1e-4
    assert abs(st["iterations"] - rs["iterations"]) <= 1
    n, loops, perturb, variant, noise = ALL_CASES[name]
    assert np.all(w[edges["k"] == 0] == 1.0)
    if noise > 0 and (edges["k"] > 0).any():
        assert 0 < w[edges["k"] > 0].min() < 1.0      # the robust weights are compared at non-trivial values
    if variant == "interleaved" or ("reversed" in variant and noise == 0.0):
        # the same graph entered differently: the device's own answers agree (the reversed forms on the consistent graph, where
        # reversing keeps the optimum: test_reversed_and_reordered_forms_have_the_same_optimum; with noise they are other problems)
        plain = PC.small_graph(n, loops, perturb, "parallel_loop" if variant.startswith("parallel") else "plain", noise)
        xp, _, sp = _device(S, *plain)
        print(name, "device against the device's plain form", _pose_diff(xp, x))
        assert sp["converged"] == 1 and _pose_diff(xp, x) <= POSE_BAR


@pytest.mark.parametrize("name", list(CASES["chains"]))
def test_preconditioner_solves_a_chain(S, name):
    """chain-only: H = M, so CG with an exact M^-1 ends after one iteration; the restated PCR needs 1 or 2"""
    init, prior, edges = _graph(name)
    H, g = G.normal_blocks(init, prior, edges)
    _, its, status = G.pcg_solve(H, g)
    x, w, st = _device(S, init, prior, edges, max_iterations=1)
    print(name, "linear iterations: restated", its, "device", st["linear_iterations"])
    assert status == 0 and st["linear_status"] == 0 and st["iterations"] == 1
    assert 1 <= st["linear_iterations"] <= its + 1


@pytest.mark.parametrize("name", LOOPED)
def test_preconditioner_over_a_run(S, name):
    """looped graphs to convergence at COUNTING_STEP_TOL, where both sides make the same decisions
    (test_looped_runs_decide_with_room_at_the_counting_step_tol): CG iterations summed over the solves"""
    init, prior, edges = _graph(name)
    ref, rs = _restated(name, step_tol=PC.COUNTING_STEP_TOL, linear="pcg")
    x, w, st = _device(S, init, prior, edges, step_tol=PC.COUNTING_STEP_TOL)
    print(name, "iterations: restated", rs["iterations"], "device", st["iterations"], "linear iterations: restated", rs["linear_iterations"], "device",
          st["linear_iterations"], "pose diff", _pose_diff(ref, x))
    assert rs["converged"] == 1 and st["converged"] == 1 and st["linear_status"] == 0
    assert st["linear_iterations"] <= rs["linear_iterations"] + 2 * rs["iterations"]
    assert _pose_diff(ref, x) <= POSE_BAR


def test_damping(S):
    """the first step is rejected (trial cost 1.8 x the cost: test_damping_case_rejects_its_first_step) and solved again with
    lambda diag(H)"""
    name = PC.DAMPING_CASE
    init, prior, edges = _graph(name)
    ref, rs = _restated(name)
    x, w, st = _device(S, init, prior, edges)
    dp = _pose_diff(ref, x)
    print(name, "pose diff", dp, "cost", rs["final_cost"], st["final_cost"], "iterations", rs["iterations"], st["iterations"], "linear iterations",
          st["linear_iterations"])
    assert len(rs["rejected"]) >= 1 and rs["trials"][0][3] is False
    assert rs["converged"] == 1 and st["converged"] == 1 and st["linear_status"] == 0
    assert dp <= POSE_BAR and _close(st["final_cost"], rs["final_cost"]) and _close(st["initial_cost"], rs["costs"][0])
    assert abs(st["iterations"] - rs["iterations"]) <= 1      # the rejected solve counts on both sides
    assert _weight_diff(w, rs["weights"]) <= 1e-4
    # one solve only: it is the rejected one, the initial poses stand
    x1, w1, s1 = _device(S, init, prior, edges, max_iterations=1)
    print(name, "max_iterations = 1:", s1)
    assert s1["iterations"] == 1 and s1["converged"] == 0 and s1["linear_status"] == 0
    assert np.abs(x1 - init).max() <= 1e-15 and s1["final_cost"] == s1["initial_cost"]


def test_quaternion_sign(S):
    """q and -q are the same rotation: every second node, the prior and every third measurement negated (rot_log's flip, put_pose)"""
    init, prior, edges = _graph("n33_l4_p0.3")
    x, w, st = _device(S, init, prior, edges)
    init2, prior2, edges2 = init.copy(), dict(prior, pose7=np.array(prior["pose7"])), {k: v.copy() for k, v in edges.items()}
    init2[::2, :4] *= -1
    prior2["pose7"][:4] *= -1
    edges2["z"][::3, :4] *= -1
    y, w2, s2 = _device(S, init2, prior2, edges2)
    print("pose diff", _pose_diff(x, y), "costs", st["initial_cost"], s2["initial_cost"], st["final_cost"], s2["final_cost"], "iterations", st["iterations"],
          s2["iterations"])
    assert st["converged"] == 1 and s2["converged"] == 1
    assert _pose_diff(x, y) <= POSE_BAR
    assert _close(s2["initial_cost"], st["initial_cost"]) and _close(s2["final_cost"], st["final_cost"])
    assert _weight_diff(w2, w) <= 1e-4


def test_one_context_for_several_sizes(S):
    """33 nodes, then 7, then 100 in one context sized for 100: bitwise what a fresh context gives (the multipliers of a PCR level are
    addressed with the current n, so a larger graph's levels must not show through)"""
    g = S.PoseGraph(100, 120)
    for name in ("n33_l4_p0.3", "n7_l2_p0.3", "n100_l0_p0.3_prior_middle", "n9_l2_p0.05"):
        init, prior, edges = _graph(name)
        x, w, st = _device(S, init, prior, edges, g=g)
        y, v, su = _device(S, init, prior, edges)
        assert st["converged"] == 1
        assert np.array_equal(x, y) and np.array_equal(w, v) and st == su, name
    g.close()
