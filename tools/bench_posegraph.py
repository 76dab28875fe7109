"""scal_posegraph (batch pose-graph optimisation on the device, csrc/posegraph.hip) against its CPU restatement
scaloam.pgo.optimize_pose_graph (numpy + scipy.sparse, exact sparse solve), timed on the same host in this script.
  - standalone: synthetic two-lap graphs with one displaced loop (scaloam.pgo.two_lap_graph) at --sizes nodes/loops: wall time per
    scal_posegraph_optimize (host clock around the synchronous call, the initial poses set again before every call; median of --reps
    after warm-up), Gauss-Newton and linear iterations, largest pose difference to the restatement, the restatement's wall time
    (median of --ref-reps runs after one warm-up run, which also takes scipy's import out of the timing);
  - in the pipeline: the out-and-back drive of tools/bench_keyframe_stream.py through scal_pipeline sc_mode 3 with
    optimize_keyframes(apply=True) after every 10th keyframe popped against the same run without it, alternated in one process.
Per-kernel times come from a separate run under rocprofv3 (--profile-only: --reps optimisations of ONE size, nothing timed), merged
with --merge from its kernel statistics.

Usage: python tools/bench_posegraph.py [--reps 9] [--revisit-steps 280] [--out profiles/posegraph.json]
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_posegraph.py --profile-only --profile-size 5000/500
       python tools/bench_posegraph.py --merge profiles/posegraph.json --kernel-stats DIR/.../kernel_stats.csv --profile-size 5000/500"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", os.path.join("sc-a-loam_amd", "python"), os.path.join("tools", "synth")):
    sys.path.insert(0, os.path.join(ROOT, p))


def sizes_of(text):
    return [tuple(int(v) for v in s.split("/")) for s in text.split(",")]


def device_run(S, g, init, prior, edges):
    g.set_nodes(init)
    t0 = time.perf_counter()
    st = g.optimize()
    return time.perf_counter() - t0, st


def load(S, init, prior, edges):
    g = S.PoseGraph(len(init), len(edges["i"]))
    g.set_nodes(init)
    g.set_prior(prior["node"], prior["pose7"], prior["var"])
    g.add_edges(edges)
    return g


def standalone(S, G, n_nodes, n_loops, reps, with_restatement=True, ref_reps=3):
    init, prior, edges, bad = G.two_lap_graph(n_nodes, n_loops)
    g = load(S, init, prior, edges)
    for _ in range(2):
        device_run(S, g, init, prior, edges)
    times = []
    for _ in range(reps):
        dt, st = device_run(S, g, init, prior, edges)
        times.append(dt)
    x, w = g.nodes(), g.edge_weights()
    g.close()
    out = {"nodes": n_nodes, "loops": n_loops, "device_ms_per_optimize": {"median": 1e3 * float(np.median(times)), "min": 1e3 * float(np.min(times)), "calls": reps},
           "gauss_newton_iterations": st["iterations"], "linear_iterations": st["linear_iterations"], "converged": st["converged"],
           "cost": [st["initial_cost"], st["final_cost"]], "weight_of_displaced_loop": float(w[n_nodes - 1 + bad])}
    if with_restatement:
        G.optimize_pose_graph(init, prior, edges)   # warm-up: scipy's imports, numpy's first calls at this shape
        t_ref = []
        for _ in range(ref_reps):
            t0 = time.perf_counter()
            ref, rs = G.optimize_pose_graph(init, prior, edges)
            t_ref.append(time.perf_counter() - t0)
        dt = float(np.median(t_ref))
        d = G.se3_log(G.se3_between(ref, x))
        out["restatement"] = {"what": "scaloam.pgo.optimize_pose_graph: numpy + scipy.sparse splu on this host's CPU, median after one warm-up run", "wall_ms": 1e3 * dt,
                              "min_ms": 1e3 * float(np.min(t_ref)), "calls": ref_reps,
                              "gauss_newton_iterations": rs["iterations"], "cost": [rs["costs"][0], rs["final_cost"]]}
        out["max_pose_difference"] = float(max(np.abs(ref[:, 4:] - x[:, 4:]).max(), np.abs(d[:, :3]).max()))
        out["device_slower_than_restatement"] = bool(out["device_ms_per_optimize"]["median"] > 1e3 * dt)
    return out


def run_stream(S, d_scans, ns, cap, W, kf_points, every, ahead=4):
    p = S.Pipeline(S.OS1_64, 0.5, max_points=cap, line_res=0.4, plane_res=0.8, max_map_points=4000000, sc_mode=S.SC_KEYFRAME,
                   sc_max_radius=80.0, sc_dist_thres=0.2, sc_max_keyframes=len(ns) + 64, keyframe_meter_gap=1.0, keyframe_deg_gap=10.0,
                   kf_max_points=kf_points)
    n_kf, calls, last = 0, [], None

    def take():
        nonlocal n_kf, last
        r = p.pop()
        if r["is_keyframe"]:
            n_kf += 1
            if every and n_kf % every == 0:
                t0 = time.perf_counter()
                _, _, last = p.optimize_keyframes(apply=True)
                calls.append(time.perf_counter() - t0)
        while p.pop_loop(wait=False) is not None:
            pass

    t0 = None
    for k in range(len(ns)):
        if k == W:
            p.drain()
            while p.in_flight():
                take()
            t0 = time.perf_counter()
        p.push_device(d_scans[k].data_ptr(), ns[k], 3)
        while p.in_flight() > ahead:
            take()
    p.drain()
    while p.in_flight():
        take()
    dt = time.perf_counter() - t0
    p.close()
    return {"scans_per_s": (len(ns) - W) / dt, "keyframes": n_kf, "calls": len(calls),
            "call_ms_median": None if not calls else 1e3 * float(np.median(calls)), "last_call": last}


def pipeline_part(S, a):
    import torch
    import scansynth
    world = scansynth.World(scansynth.OS1_64, 301, threads=min(16, len(os.sched_getaffinity(0))))
    q0, t0 = world.pose(0)
    d = world.pose(10)[1] - t0
    d[2] = 0
    d /= np.linalg.norm(d)
    W = a.warmup
    n_rev = W + a.revisit_steps
    half = n_rev // 2
    steps = [0.5] * (half - 4) + [0.3, 0.1, 0.0, -0.1, -0.3] + [-0.5] * (n_rev - half - 2)
    x = np.concatenate([[0.0], np.cumsum(steps)])[:n_rev]
    scans = [world.scan_pose(q0, t0 + d * xi, 5000 + k) for k, xi in enumerate(x)]
    ns = [s.shape[0] for s in scans]
    cap = max(ns) + 1024
    d_scans = [torch.from_numpy(s).cuda() for s in scans]
    run_stream(S, d_scans, ns, cap, W, a.kf_points, 10)  # warm-up of every shape
    rates = {"none": [], "optimize_every_10th_keyframe": []}
    info = None
    for _ in range(a.alternations):
        for key, every in (("none", 0), ("optimize_every_10th_keyframe", 10)):
            r = run_stream(S, d_scans, ns, cap, W, a.kf_points, every)
            rates[key].append(r["scans_per_s"])
            if every:
                info = r
    return {"stream": "out-and-back drive of tools/bench_keyframe_stream.py (OS1-64, seed 301, 0.5 m per scan, gate 1 m / 10 deg)",
            "timed_scans": a.revisit_steps, "warmup": W, "scans_per_s": rates, "keyframes": info["keyframes"], "calls_per_stream": info["calls"],
            "call_ms_median": info["call_ms_median"], "last_call": info["last_call"]}


def merge(a):
    line = json.load(open(a.merge))
    rows = [r for r in csv.DictReader(open(a.kernel_stats)) if "k_pg_" in r["Name"]]
    reps = a.reps + 2
    per = {r["Name"].split("(")[0].replace("scal::", "").replace("void ", ""): {"dispatches_per_optimize": int(r["Calls"]) / reps, "us_per_optimize": float(r["TotalDurationNs"]) * 1e-3 / reps,
                                                        "average_us": float(r["AverageNs"]) * 1e-3} for r in rows}
    line["kernels_rocprofv3"] = {"size": a.profile_size, "optimizes": reps, "kernels": per,
                                 "kernel_us_per_optimize": float(sum(v["us_per_optimize"] for v in per.values())),
                                 "dispatches_per_optimize": float(sum(v["dispatches_per_optimize"] for v in per.values()))}
    s = json.dumps(line)
    print(s)
    with open(a.out or a.merge, "w") as f:
        f.write(s + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="600/20,5000/500,20000/2000")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--ref-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--revisit-steps", type=int, default=280)
    ap.add_argument("--alternations", type=int, default=2)
    ap.add_argument("--kf-points", type=int, default=8000000)
    ap.add_argument("--no-pipeline", action="store_true")
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--profile-size", default="5000/500")
    ap.add_argument("--merge", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posegraph.json"))
    a = ap.parse_args()
    if a.merge:
        return merge(a)
    import torch  # noqa: F401  (its HIP runtime first, as in tests/conftest.py)
    import scaloam as S
    from scaloam import pgo as G
    if S.device_count() < 1:
        raise SystemExit("bench_posegraph.py needs a GPU: there is no CPU fallback to time")
    if a.profile_only:
        n, l = sizes_of(a.profile_size)[0]
        print(json.dumps(standalone(S, G, n, l, a.reps, with_restatement=False)))
        return
    line = {"metric": "scal_posegraph_optimize wall time against the scipy restatement; scal_pipeline_optimize_keyframes inside the keyframe stream",
            "defaults": {"max_iterations": 50, "step_tol": 1e-8, "max_linear_iterations": 2000, "linear_rtol": 1e-12},
            "standalone": [standalone(S, G, n, l, a.reps, ref_reps=a.ref_reps) for n, l in sizes_of(a.sizes)]}
    if not a.no_pipeline:
        line["pipeline"] = pipeline_part(S, a)
    s = json.dumps(line)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
