"""scal_pipeline's pose-graph map (scal_pipeline_pgo_map: pubMap, laserPosegraphOptimization.cpp:810-834, on the device) on the BASELINE
config #3 stream: the OS1-64 sequence of seed 301 through sc_mode 3 (launch/aloam_mulran.launch's values: minimum_range 0.5, mapping
resolutions 0.4 / 0.8, sc_dist_thres 0.2, sc_max_radius 80), at the default 2 m / 10 deg keyframe gate and at 0.4 m for a larger store.
For each gate, after a drain, the map of every keyframe (kf_end = all, skip 2, leaf 0.4 - the reference's settings):
  - points before and after the filter;
  - wall time per call (host clock around the synchronous call; median of --reps calls after warm-up), with the map left in device
    memory (cap 0) and with its download through the Python binding;
  - the host-side comparison: numpy pgo_map_cloud + the oracle's VoxelGrid (oracle/voxel.cpp: the oracle, not PCL) on the same map;
  - scans/s of the stream with a map built after every 10th keyframe popped against none, in this process, alternated.
Per-kernel times come from a separate run under rocprofv3 (--profile-only: the stream and the map calls, nothing timed), merged with
--kernel-trace: only the dispatches of the thread that called scal_pipeline_pgo_map are the map's (the pipeline launches from its own
threads).  The gather's algorithmic bytes are 32 per point (16 in, 16 out).

Usage: python tools/bench_pgo_map.py [--steps 400] [--warmup 20] [--reps 25] [--out profiles/pgo_map.json]
       rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_pgo_map.py --profile-only --out DIR/tid.json
       python tools/bench_pgo_map.py --merge profiles/pgo_map.json --kernel-trace DIR/.../kernel_trace.csv --tid-file DIR/tid.json"""
import argparse
import csv
import ctypes
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", os.path.join("sc-a-loam_amd", "python"), os.path.join("tools", "synth")):
    sys.path.insert(0, os.path.join(ROOT, p))

HBM_PEAK = 8.0e12  # bytes/s, MI355X spec
GATES = (2.0, 0.4)


def make_pipeline(S, cap, n, gap, kf_points, map_points):
    return S.Pipeline(S.OS1_64, 0.5, max_points=cap, line_res=0.4, plane_res=0.8, max_map_points=4000000, sc_mode=S.SC_KEYFRAME,
                      sc_max_radius=80.0, sc_dist_thres=0.2, sc_max_keyframes=n + 64, keyframe_meter_gap=gap, keyframe_deg_gap=10.0,
                      kf_max_points=kf_points, pgo_map_max_points=map_points)


def run_stream(S, d_scans, ns, cap, W, gap, kf_points, map_points, map_every=0, ahead=4):
    """the stream (timed from scan W); map_every > 0: pgo_map() after every map_every-th keyframe popped.  Returns the drained pipeline."""
    p = make_pipeline(S, cap, len(ns), gap, kf_points, map_points)
    n_kf, n_maps = 0, 0

    def take():
        nonlocal n_kf, n_maps
        r = p.pop()
        if r["is_keyframe"]:
            n_kf += 1
            if map_every and n_kf % map_every == 0:
                p.pgo_map()
                n_maps += 1
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
    while p.pop_loop(wait=True) is not None:
        pass
    return p, {"scans_per_s": (len(ns) - W) / dt, "keyframes": n_kf, "maps_built": n_maps}


def raw_map(S, p, kf_end, skip, leaf):
    n = ctypes.c_longlong(0)
    rc = S.lib().scal_pipeline_pgo_map(p.h, kf_end, skip, leaf, None, 0, ctypes.byref(n))
    if rc != 0:
        raise S.ScalError(rc, S.lib().scal_last_error().decode())
    return n.value


def measure_gate(S, O, d_scans, ns, cap, W, gap, a):
    from scaloam.pgo import pgo_map_cloud
    p, _ = run_stream(S, d_scans, ns, cap, W, gap, a.kf_points, a.map_points)
    n_kf = p._kf_end
    kfs = [p.keyframe(i) for i in range(n_kf)]
    n_in = sum(c.shape[0] for _, c in kfs[::2])
    for _ in range(3):
        raw_map(S, p, n_kf, 2, 0.4)
    t_dev, t_host = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        n_out = raw_map(S, p, n_kf, 2, 0.4)
        t_dev.append(time.perf_counter() - t0)
    for _ in range(3):
        p.pgo_map(kf_end=n_kf)
    for _ in range(a.reps):
        t0 = time.perf_counter()
        m = p.pgo_map(kf_end=n_kf)
        t_host.append(time.perf_counter() - t0)
    t_orc = []
    for _ in range(3):
        t0 = time.perf_counter()
        ref, guard = O.voxel_grid(pgo_map_cloud([c for _, c in kfs], [q for q, _ in kfs], n_kf, 2), 0.4)
        t_orc.append(time.perf_counter() - t0)
    p.close()
    # throughput with a map every 10th keyframe against none, alternated
    rates = {"none": [], "every_10th_keyframe": []}
    maps_built = 0
    for _ in range(a.alternations):
        for key, every in (("none", 0), ("every_10th_keyframe", 10)):
            q, r = run_stream(S, d_scans, ns, cap, W, gap, a.kf_points, a.map_points, map_every=every)
            q.close()
            rates[key].append(r["scans_per_s"])
            maps_built = max(maps_built, r["maps_built"])
    return {
        "keyframe_gap_m": gap, "keyframes": n_kf, "kf_end": n_kf, "skip": 2, "leaf": 0.4,
        "points_before_filter": int(n_in), "points_after_filter": int(n_out),
        "equal_to_oracle": bool(guard == 0 and np.array_equal(m.view(np.uint32), ref.view(np.uint32))),
        "wall_ms_per_call_device": {"median": 1e3 * float(np.median(t_dev)), "min": 1e3 * float(np.min(t_dev)), "calls": a.reps},
        "wall_ms_per_call_with_download": {"median": 1e3 * float(np.median(t_host)), "min": 1e3 * float(np.min(t_host)), "calls": a.reps},
        "host_oracle_ms": {"what": "numpy pgo_map_cloud + oracle VoxelGrid (oracle/voxel.cpp, not PCL), one CPU thread",
                           "median": 1e3 * float(np.median(t_orc))},
        "stream_scans_per_s": {"none": rates["none"], "map_every_10th_keyframe": rates["every_10th_keyframe"], "maps_per_stream": maps_built},
    }


def profile_only(S, d_scans, ns, cap, W, a):
    """the calls rocprofv3 traces: each gate's stream, then --reps maps from this thread"""
    for gap in GATES:
        p, _ = run_stream(S, d_scans, ns, cap, W, gap, a.kf_points, a.map_points)
        for _ in range(a.reps):
            raw_map(S, p, p._kf_end, 2, 0.4)
        p.close()
    return {"map_thread_id": threading.get_native_id(), "gates": list(GATES), "reps": a.reps}


def merge(a):
    """per-kernel times of the map (dispatches of the map thread) into the JSON of a measuring run, gate by gate in call order"""
    line = json.load(open(a.merge))
    tid = json.load(open(a.tid_file))
    rows = [r for r in csv.DictReader(open(a.kernel_trace)) if int(r["Thread_Id"]) == tid["map_thread_id"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    # one map call = one k_pgo_gather and the kernels up to the next one
    calls, cur = [], None
    for r in rows:
        if "k_pgo_gather" in r["Kernel_Name"]:
            cur = []
            calls.append(cur)
        if cur is not None:
            cur.append((r["Kernel_Name"].split("(")[0], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3))
    reps = tid["reps"]
    for g, gate in enumerate(line["maps"]):
        per = {}
        for call in calls[g * reps:(g + 1) * reps]:
            for name, us in call:
                per.setdefault(name, []).append(us)
        stats = {k: {"median_us": float(np.median(v)), "dispatches": len(v)} for k, v in per.items()}
        gather = next(v for k, v in stats.items() if "k_pgo_gather" in k)
        n = gate["points_before_filter"]
        bytes_ = 32.0 * n
        gate["kernels_rocprofv3"] = stats
        gate["gather"] = {"algorithmic_bytes": bytes_, "kernel_us": gather["median_us"],
                          "bytes_per_s": bytes_ / (gather["median_us"] * 1e-6), "share_of_8TBps": bytes_ / (gather["median_us"] * 1e-6) / HBM_PEAK}
        gate["kernels_per_call_us"] = float(sum(v["median_us"] * v["dispatches"] / reps for v in stats.values()))
    s = json.dumps(line)
    print(s)
    with open(a.out or a.merge, "w") as f:
        f.write(s + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--alternations", type=int, default=2)
    ap.add_argument("--kf-points", type=int, default=16000000)
    ap.add_argument("--map-points", type=int, default=10000000)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--merge", default=None)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--tid-file", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pgo_map.json"))
    a = ap.parse_args()
    if a.merge:
        return merge(a)
    import torch
    import scaloam as S
    import oracle_py as O
    import scansynth
    W, K = a.warmup, a.steps
    world = scansynth.World(scansynth.OS1_64, 301, threads=min(16, len(os.sched_getaffinity(0))))
    scans = [world.scan(k) for k in range(W + K)]
    ns = [s.shape[0] for s in scans]
    cap = max(ns) + 1024
    d_scans = [torch.from_numpy(s).cuda() for s in scans]
    if a.profile_only:
        line = profile_only(S, d_scans, ns, cap, W, a)
    else:
        line = {
            "metric": "scal_pipeline_pgo_map (pubMap on the device) on the config #3 stream through scal_pipeline sc_mode 3",
            "steps": K, "warmup": W,
            "config": {"workload": "OS1-64, seed 301, minimum_range 0.5, line/plane 0.4/0.8, sc_dist_thres 0.2, keyframe gate x m / 10 deg",
                       "kf_max_points": a.kf_points, "pgo_map_max_points": a.map_points},
            "maps": [measure_gate(S, O, d_scans, ns, cap, W, gap, a) for gap in GATES],
        }
    s = json.dumps(line)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
