"""The small pose graphs shared by test_posegraph_cpu.py (their properties, no device) and test_posegraph_small_gpu.py (the device
on them): scaloam.pgo.two_lap_graph(n, loops, seed, bad_offset=None, perturb) in one of pgo.graph_variant's forms.  perturb 0.3 puts
every between residual's angle above pgo.SERIES_THETA (the closed-form branches), 0.05 on both sides of it.  Seed 1 unless the
first Gauss-Newton step from it is rejected (n = 64, 65 at perturb 0.3: seed 3)."""
import numpy as np

from scaloam import pgo as G

SMALL_CHAIN_N = (2, 3, 7, 8, 9, 15, 33, 64, 65)
SMALL_LOOPS = {3: 1, 7: 2, 8: 2, 9: 2, 15: 3, 33: 4, 64: 1, 65: 6}   # n = 3: the loop is (1, 2), next to an odometry edge
PCR_CHAIN_N = (2, 3, 6, 7, 8, 9, 14, 15, 32, 33, 100)
REVERSED = ("loops_reversed", "odometry_alternate_reversed", "parallel_loop_reversed")
COUNTING_STEP_TOL = 1e-5             # step_tol of the runs whose CG iterations are counted: every decision has room there
DAMPING_CASE = "n33_l4_p0.5"          # the first step from here is rejected (trial cost 1.8 x the cost)


def name_of(n, loops, perturb, variant="plain", noise=1.0):
    return "n%d_l%d_p%g" % (n, loops, perturb) + ("" if noise == 1.0 else "_noise%g" % noise) + ("" if variant == "plain" else "_" + variant)


def prior_only_graph():
    """one node, 0.35 rad and 0.35 m away from its prior, no edges"""
    init = G.pose7_from_pose6(np.array([[1.0, 2.0, 3.0, 0.1, 0.2, 0.3]]))
    prior = dict(node=0, pose7=G.se3_retract(init, np.full((1, 6), 0.2))[0], var=np.array(G.PRIOR_VARIANCES))
    return init, prior, G.make_edges([], [], np.zeros((0, 7)), G.ODOM_VARIANCES, 0.0)


def small_graph(n, loops, perturb, variant="plain", noise=1.0):
    if n == 1:
        return prior_only_graph()
    seed = 3 if (n in (64, 65) and perturb == 0.3) else 1
    init, prior, edges, _ = G.two_lap_graph(n, loops, seed=seed, bad_offset=None, perturb=perturb, noise=noise)
    return G.graph_variant(init, prior, edges, variant)


def cases():
    """name -> (n, loops, perturb, variant, noise), in four families: 'one_step' (chain-only and looped, perturb 0.3 and 0.05, some
    with tight loops, two with edges entered from their other end; also run to convergence), 'variants' (the forms of
    graph_variant on 33 nodes / 4 loops; the reversed ones with noise - the device against the restatement at an optimum with
    non-zero residuals - and on the consistent graph, noise 0, where reversing an edge keeps the optimum and the forms can be compared
    with each other), 'chains' (perturbed chain-only graphs with the prior on node 0, on the last and on a middle node: H = M, the
    preconditioner alone solves them) and the damping case."""
    one, var, chains = {}, {}, {}
    for p in (0.3, 0.05):
        for n in SMALL_CHAIN_N:
            one[name_of(n, 0, p)] = (n, 0, p, "plain", 1.0)
        for n, l in SMALL_LOOPS.items():
            one[name_of(n, l, p)] = (n, l, p, "plain", 1.0)
    one[name_of(200, 10, 0.05)] = (200, 10, 0.05, "plain", 1.0)
    one["n1_prior_only"] = (1, 0, 0.3, "plain", 1.0)
    for n, l, p in ((9, 2, 0.3), (33, 4, 0.3), (65, 6, 0.3), (33, 4, 0.05)):
        one[name_of(n, l, p, "tight_loops")] = (n, l, p, "tight_loops", 1.0)
    for v in ("loops_reversed", "odometry_alternate_reversed"):
        one[name_of(33, 4, 0.3, v)] = (33, 4, 0.3, v, 1.0)
    one[name_of(15, 3, 0.3, "tight_loops_reversed")] = (15, 3, 0.3, "tight_loops_reversed", 1.0)
    for v in G.GRAPH_VARIANTS:
        if v.startswith("tight_loops"):
            continue
        var[name_of(33, 4, 0.3, v)] = (33, 4, 0.3, v, 1.0)
    for v in ("plain", "interleaved", "parallel_loop") + REVERSED:
        var[name_of(33, 4, 0.3, v, 0.0)] = (33, 4, 0.3, v, 0.0)
    for n in PCR_CHAIN_N:
        for v in ("plain", "prior_last", "prior_middle"):
            chains[name_of(n, 0, 0.3, v)] = (n, 0, 0.3, v, 1.0)
    return dict(one_step=one, variants=var, chains=chains, damping={DAMPING_CASE: (33, 4, 0.5, "plain", 1.0)})
