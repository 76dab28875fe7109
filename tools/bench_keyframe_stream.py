"""scal_pipeline sc_mode 3 (keyframe ScanContext + ICP-verified loops) on the BASELINE config #3 stream: the OS1-64 sequence of seed 301,
launch/aloam_mulran.launch's values (minimum_range 0.5, mapping resolutions 0.4 / 0.8, keyframe gap 1 m / 10 deg, sc_dist_thres 0.2,
sc_max_radius 80).  Prints one JSON line:
  - the pipeline in mode 3 without keyframe clouds (kf_max_points 0: nothing verified) and with them (every detected loop verified):
    scans/s, keyframes, loops detected / accepted / rejected / not verifiable, verification latency p50 / p99;
  - for comparison, the synchronous per-stage loop (features -> odometry -> mapping -> Python keyframe gate -> insert + detect) on
    the same scans, which is what bench.py --config 3 measures.
Two streams: the config #3 sequence (no revisits within a few hundred scans), and the same world driven out and back along one line
(0.5 m per scan), whose way back revisits the way out and gives the verification loops to check.
Verification latency: from the pop of the query scan's result to the loop record being ready, polled after every scan (so it is
rounded up to the next scan's pop), the records still pending at the end waited for.

Usage: python tools/bench_keyframe_stream.py [--steps 400] [--revisit-steps 280] [--warmup 20] [--kf-points 8000000] [--out profiles/keyframe_stream.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", os.path.join("sc-a-loam_amd", "python"), os.path.join("tools", "synth")):
    sys.path.insert(0, os.path.join(ROOT, p))


def run_pipeline(S, d_scans, ns, cap, W, kf_points, ahead=4):
    p = S.Pipeline(S.OS1_64, 0.5, max_points=cap, line_res=0.4, plane_res=0.8, max_map_points=4000000, sc_mode=S.SC_KEYFRAME,
                   sc_max_radius=80.0, sc_dist_thres=0.2, sc_max_keyframes=len(ns) + 64, keyframe_meter_gap=1.0, keyframe_deg_gap=10.0,
                   kf_max_points=kf_points)
    res, loops, lat, t_det = [], [], [], {}

    def take(r):
        res.append(r)
        if r["loop"] is not None and r["loop"]["loop_id"] >= 0:
            t_det[r["seq"]] = time.perf_counter()

    def poll(wait):
        while True:
            rec = p.pop_loop(wait=wait)
            if rec is None:
                return
            now = time.perf_counter()
            lat.append(now - t_det.get(rec["seq"], now))  # a record can be ready before its scan's result has been popped: no wait
            loops.append(rec)

    t0 = None
    for k in range(len(ns)):
        if k == W:
            p.drain()
            while p.in_flight():
                take(p.pop())
            poll(True)
            t0 = time.perf_counter()
        p.push_device(d_scans[k].data_ptr(), ns[k], 3)
        while p.in_flight() > ahead:
            take(p.pop())
        poll(False)
    p.drain()
    while p.in_flight():
        take(p.pop())
    poll(True)
    dt = time.perf_counter() - t0
    p.close()
    lat_ms = np.array(lat) * 1e3
    return {
        "scans_per_s": (len(ns) - W) / dt,
        "keyframes": int(sum(r["is_keyframe"] for r in res)),
        "loops_detected": int(sum(1 for r in res if r["loop"] is not None and r["loop"]["loop_id"] >= 0)),
        "loops_accepted": int(sum(r["verified"] == 1 for r in loops)),
        "loops_rejected": int(sum(r["verified"] == 0 for r in loops)),
        "loops_not_verifiable": int(sum(r["verified"] == -1 for r in loops)),
        "verify_latency_ms": None if lat_ms.size == 0 else {"p50": float(np.percentile(lat_ms, 50)), "p99": float(np.percentile(lat_ms, 99))},
    }, [(r["seq"], r["is_keyframe"], r["keyframe_id"], None if r["loop"] is None else r["loop"]["loop_id"]) for r in res]


def run_serial(S, d_scans, ns, cap, W):
    import torch
    from scaloam.pgo import KeyframeGate
    reg = S.ScanRegistration(S.OS1_64, 0.5, max_points=cap)
    od = S.LaserOdometry(max_points=cap)
    mp = S.LaserMapping(0.4, 0.8, max_scan_points=cap, max_map_points=4000000)
    sc = S.SCManager(max_radius=80.0, dist_thres=0.2, max_keyframes=len(ns) + 64)
    gate = KeyframeGate(1.0, 10.0)
    n_kf, out = 0, []
    t0 = None
    for k in range(len(ns)):
        if k == W:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        reg.run_device(d_scans[k].data_ptr(), ns[k], 3)
        _, _, qw, tw, _ = od.step_features(reg)
        qm, tm, _ = mp.process_features(reg, qw, tw)
        kf, lid = gate(qm, tm), None
        if kf:
            sc.insert_features(reg)
            n_kf += 1
            if n_kf >= 30:  # performSCLoopClosure's guard (:715), as the pipeline applies it
                lid = sc.detectLoopClosureID()["loop_id"]
        out.append((k, kf, n_kf - 1 if kf else -1, lid))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    for x in (reg, od, mp, sc):
        x.close()
    return {"scans_per_s": (len(ns) - W) / dt}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--revisit-steps", type=int, default=280, help="timed scans of the out-and-back stream (0.5 m each, half out, half back)")
    ap.add_argument("--kf-points", type=int, default=8000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyframe_stream.json"))
    a = ap.parse_args()
    import torch
    import scaloam as S
    import scansynth
    W, K = a.warmup, a.steps
    world = scansynth.World(scansynth.OS1_64, 301, threads=min(16, len(os.sched_getaffinity(0))))

    def measure(scans):
        ns = [s.shape[0] for s in scans]
        cap = max(ns) + 1024
        d_scans = [torch.from_numpy(s).cuda() for s in scans]
        no_clouds, seq0 = run_pipeline(S, d_scans, ns, cap, W, 0)
        clouds, seq1 = run_pipeline(S, d_scans, ns, cap, W, a.kf_points)
        serial, seq2 = run_serial(S, d_scans, ns, cap, W)
        return {"points_per_scan_in": int(np.mean(ns)), "pipeline_no_clouds": no_clouds, "pipeline_with_clouds": clouds, "serial_per_stage": serial,
                "keyframes_and_loops_equal_across_runs": seq0 == seq1 and [x[1:] for x in seq0] == [x[1:] for x in seq2]}

    # the config #3 sequence itself (its trajectory does not come back within a few hundred scans: no loops), then the same world
    # driven out and back along one line (0.5 m per scan, the way back in reverse gear) so that the verification has work
    config3 = measure([world.scan(k) for k in range(W + K)])
    q0, t0 = world.pose(0)
    d = world.pose(10)[1] - t0
    d[2] = 0
    d /= np.linalg.norm(d)
    n_rev = W + a.revisit_steps
    half = n_rev // 2
    steps = [0.5] * (half - 4) + [0.3, 0.1, 0.0, -0.1, -0.3] + [-0.5] * (n_rev - half - 2)
    x = np.concatenate([[0.0], np.cumsum(steps)])[:n_rev]
    revisit = measure([world.scan_pose(q0, t0 + d * xi, 5000 + k) for k, xi in enumerate(x)])
    line = {
        "metric": "scans/s, config #3 OS1-64 stream through scal_pipeline sc_mode 3 (keyframe ScanContext + ICP-verified loops)",
        "steps": K, "revisit_steps": a.revisit_steps, "warmup": W,
        "config": {"workload": "OS1-64, seed 301, minimum_range 0.5, line/plane 0.4/0.8, keyframe gap 1 m / 10 deg, sc_dist_thres 0.2",
                   "kf_max_points": a.kf_points, "out_and_back": "same world, 0.5 m per scan along one line, turning back at the middle"},
        "config3_stream": config3,
        "out_and_back_stream": revisit,
    }
    s = json.dumps(line)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
