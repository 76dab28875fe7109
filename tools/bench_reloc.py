#!/usr/bin/env python3
"""Relocalisation against a stored session (scal_reloc_*) on one MI355X.
Session: K synthetic HDL-64 keyframes along the generator's path (1 m apart on a 100 m circle: one lap is 628 keyframes), stored with
their true poses - the setup of tools/bench_refine.py.  Queries: Q scans of the SECOND lap (every other one, 0.3 m beside a stored
keyframe's place), each turned about z by a seeded yaw; the truth of a query is its generator pose times the inverse turn.
  - wall ms per query: scal_reloc_query one by one, and scal_reloc_query_batch over all of them;
  - the search alone: scal_sc_detect_between over the queries' descriptors, batched (64 per launch set) and one by one;
  - device time per stage from the library's own per-kernel timers, in a separate pass (they add a little to every launch; of the ICP
    only its neighbour-search kernels carry a timer, which is where its time goes);
  - accepted share and median error against the truth; the same run with no_yaw_guess = 1.
cross_search: N x N, mode 2, alternating in one process with distance_matrix_device over an equally sized block inside one database -
the same k_sc_gram launches, plus the row top-k.
Wall times are the median of --reps (5) after one warm-up.  Writes one JSON document (default profiles/reloc.json) and prints it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join("sc-a-loam_amd", "python"), os.path.join("tools", "synth")):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np  # noqa: E402

LAP = 628  # keyframes per lap of the generator's circle


def pose12(q_xyzw, t):
    x, y, z, w = q_xyzw
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return np.hstack([R, np.asarray(t).reshape(3, 1)])


def P4(p):
    M = np.eye(4)
    M[:3] = np.asarray(p).reshape(3, 4)
    return M


def median_ms(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), r, [float(t) for t in ts]


def same_record(a, b):
    """two result records (nested dicts of numbers and arrays): every field, bit for bit"""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same_record(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, float):
        return np.float64(a).tobytes() == np.float64(b).tobytes()
    return a == b


STAGES = (("filter", ("k_vox", "k_deinterleave", "k_interleave4", "k_radix", "k_sort")), ("descriptor", ("k_sc_bin", "k_sc_finish")),
          ("search", ("k_sc_keys", "k_sc_topk", "k_sc_detect")), ("submap", ("k_submap_gather",)), ("icp_neighbours", ("k_icp",)))


def stage_ms(prof, n):
    out = {name: 0.0 for name, _ in STAGES}
    other = 0.0
    for kernel, (ms, _) in prof.items():
        for name, prefixes in STAGES:
            if kernel.startswith(prefixes):
                out[name] += ms / n
                break
        else:
            other += ms / n
    out["other"] = other
    return out


def reloc_part(a, S, scansynth, out):
    world = scansynth.World(scansynth.HDL64, 99)
    rng = np.random.default_rng(21)
    t0 = time.perf_counter()
    raw = [world.scan(k) for k in range(a.keyframes)]
    raw = [np.hstack([x, np.zeros((x.shape[0], 1), np.float32)]) for x in raw]
    poses = [pose12(*world.pose(k)).reshape(12) for k in range(a.keyframes)]
    qs, truth, yaws = [], [], []
    for i in range(a.queries):
        k = LAP + 2 * i
        x = world.scan(k)
        yaw = float(rng.uniform(-np.pi, np.pi))
        R = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
        T = np.eye(4)
        T[:3, :3] = R
        qs.append(np.hstack([(x.astype(np.float64) @ R.T).astype(np.float32), np.zeros((x.shape[0], 1), np.float32)]))
        truth.append(P4(pose12(*world.pose(k))) @ np.linalg.inv(T))
        yaws.append(yaw)
    gen_s = time.perf_counter() - t0
    max_q = max(max(x.shape[0] for x in raw), max(x.shape[0] for x in qs))
    rec = {"keyframes": a.keyframes, "queries": a.queries, "generation_s": gen_s, "raw_points_per_scan": int(np.mean([x.shape[0] for x in raw]))}
    for name, no_guess in (("yaw_guess", False), ("no_yaw_guess", True)):
        # work buffers: a submap of 51 filtered keyframes is larger than a raw scan
        rl = S.Relocalizer(a.keyframes, 24000 * a.keyframes, max_query_points=max(max_q, 51 * 24000), no_yaw_guess=no_guess)
        t0 = time.perf_counter()
        for x, P in zip(raw, poses):
            rl.add_keyframe(x, P)
        add_ms = (time.perf_counter() - t0) * 1e3 / a.keyframes
        reps = a.noguess_reps if no_guess else a.reps
        ms_single, res, all_single = median_ms(lambda: [rl.query(q) for q in qs], reps)
        ms_batch, resb, all_batch = median_ms(lambda: rl.query_batch(qs), reps)
        err_t = np.array([np.linalg.norm(P4(r["pose12"])[:3, 3] - t[:3, 3]) for r, t in zip(res, truth)])
        err_r = np.array([np.degrees(np.arccos(np.clip((np.trace(P4(r["pose12"])[:3, :3] @ t[:3, :3].T) - 1) / 2, -1, 1))) for r, t in zip(res, truth)])
        ok = np.array([r["status"] == 1 for r in res])
        found = np.array([r["status"] != 0 for r in res])
        r1 = {"timed_repetitions": reps, "add_keyframe_ms": add_ms, "query_ms": ms_single / a.queries, "query_ms_runs": [t / a.queries for t in all_single],
              "query_batch_ms_per_query": ms_batch / a.queries, "query_batch_ms_runs": [t / a.queries for t in all_batch],
              "batch_equals_single_bitwise": bool(all(same_record(x, y) for x, y in zip(res, resb))),
              "place_found_share": float(found.mean()), "accepted_share": float(ok.mean()),
              "icp_iterations_mean": float(np.mean([r["icp"]["iterations"] for r in res if r["status"]])) if found.any() else 0.0,
              "n_src_mean": float(np.mean([r["n_src"] for r in res])), "n_tgt_mean": float(np.mean([r["n_tgt"] for r in res if r["status"]])) if found.any() else 0.0,
              "accepted_error_median": {"m": float(np.median(err_t[ok])) if ok.any() else None, "deg": float(np.median(err_r[ok])) if ok.any() else None},
              "accepted_error_max_m": float(err_t[ok].max()) if ok.any() else None,
              "accepted_more_than_1m_off": int((err_t[ok] > 1.0).sum())}
        if not no_guess:
            db = rl.sc()
            vg, gm = S.VoxelGrid(max_points=max_q), S.SCManager()
            descs = [gm.makeScancontext(vg.filter(q, 0.4)) for q in qs]
            vg.close(), gm.close()
            ms_sb, _, _ = median_ms(lambda: db.detect_between(descs))
            ms_ss, _, _ = median_ms(lambda: [db.detect_between([d]) for d in descs])
            r1["search_ms_per_query"] = {"batched": ms_sb / a.queries, "single": ms_ss / a.queries}
        S.prof_reset()
        S.prof_enable(True)
        for q in qs:
            rl.query(q)
        S.prof_enable(False)
        r1["device_ms_per_query_by_stage"] = stage_ms(S.prof_read_all(), a.queries)
        S.prof_reset()
        rl.close()
        rec[name] = r1
        print(f"{name} done", file=sys.stderr, flush=True)
    out["reloc"] = rec
    out["value"] = rec["yaw_guess"]["query_ms"]


def cross_part(a, S, torch, out):
    n = a.cross
    rng = np.random.default_rng(31)
    A, B = S.SCManager(max_keyframes=n), S.SCManager(max_keyframes=n)
    for m in (A, B):
        for _ in range(n):
            d = rng.uniform(-2.0, 18.0, (20, 60)) * (rng.uniform(size=(20, 60)) < 0.5)
            m.saveScancontextAndKeys(d)
    d_dist = torch.empty(n * n, dtype=torch.float64, device="cuda")
    d_shift = torch.empty(n * n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def inside():
        A.distance_matrix_device(0, n, 0, n, 2, d_dist.data_ptr(), d_shift.data_ptr())
        A.sync()

    def cross():
        return A.cross_search(B, 0, n, 3, 2)
    inside(), cross()
    t_in, t_cr = [], []
    for _ in range(5):  # alternating
        t0 = time.perf_counter()
        inside()
        t_in.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        cross()
        t_cr.append((time.perf_counter() - t0) * 1e3)
    out["cross_search"] = {"n": n, "mode": 2, "k": 3, "distance_matrix_device_ms": float(np.median(t_in)), "distance_matrix_device_runs": t_in,
                           "cross_search_ms": float(np.median(t_cr)), "cross_search_runs": t_cr,
                           "pairs_per_s_cross": n * n / (float(np.median(t_cr)) * 1e-3)}
    A.close(), B.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=512)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--cross", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=5, help="timed repetitions after the warm-up; the median is reported")
    ap.add_argument("--noguess-reps", type=int, default=5, help="the same for the no_yaw_guess run (its queries mostly run into the iteration cap)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reloc.json"))
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)  # torch's HIP context first, as in bench.py
    torch.zeros(1, device="cuda")
    import scaloam as S
    import scansynth
    out = {"metric": "relocalisation against a stored session, ms per query", "unit": "ms", "sensor": "HDL-64 synthetic", "leaf_m": 0.4}

    def dump():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    if a.keyframes > 0 and a.queries > 0:
        reloc_part(a, S, scansynth, out)
        dump()
    if a.cross > 0:
        cross_part(a, S, torch, out)
        dump()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
