#!/usr/bin/env python3
"""The radius neighbour index (scal_nbr_*) on one MI355X.
Input: the map of tools/removert_scene.py corridor_session(--keyframes) - the input of tools/bench_removert.py - at r = --r.
  - wall ms of set_index (upload, keys, sort, index) and of query_self, median of --reps after a warm-up;
  - a cross query: the map against a copy of itself shifted by --shift metres along the tunnel (upload, sort, query, download);
  - (query, record) pairs tested per second over the query's wall time, and the work items;
  - device ms per kernel from the library's own per-kernel timers, in a separate pass (they add a little to every launch);
  - the CPU restatement (scipy cKDTree candidates, exact f32 decision; one core) on the same self query, whether the outlier masks
    at --min-neighbors are equal, and the ratio of the wall times (--cpu-points N restricts the restatement's queries to the first
    N points and says so; -1 skips it).
Writes one JSON document (default profiles/mapdiff.json) and prints it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sc-a-loam_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [float(t) for t in ts], r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=400)
    ap.add_argument("--spacing", type=float, default=2.0)
    ap.add_argument("--step", type=float, default=1.0, help="ray grid of the synthetic scans, degrees")
    ap.add_argument("--r", type=float, default=0.5)
    ap.add_argument("--shift", type=float, default=5.0)
    ap.add_argument("--min-neighbors", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5, help="timed repetitions after the warm-up; the median is reported")
    ap.add_argument("--cpu-points", type=int, default=0, help="queries the CPU restatement runs (0 = all, -1 = skip it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapdiff.json"))
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)  # torch's HIP context first, as in bench.py
    torch.zeros(1, device="cuda")
    import scaloam as S
    from scaloam import nbr
    import removert_scene
    t0 = time.perf_counter()
    mp, _, _, _ = removert_scene.corridor_session(a.keyframes, a.spacing, a.step, seed=7)
    gen_s = time.perf_counter() - t0
    n = mp.shape[0]
    shifted = mp.copy()
    shifted[:, 0] += np.float32(a.shift)
    idx = S.RadiusIndex(n, n)
    set_ms, set_runs, _ = timed(lambda: idx.set_index(mp, a.r), a.reps)
    self_ms, self_runs, (count, d2) = timed(idx.query_self, a.reps)
    self_stats = idx.stats()
    cross_ms, cross_runs, (ccount, _) = timed(lambda: idx.query(shifted), a.reps)
    cross_stats = idx.stats()
    S.prof_reset()
    S.prof_enable(True)
    idx.set_index(mp, a.r)
    idx.query_self()
    prof_self = S.prof_read_all()
    S.prof_reset()
    idx.query(shifted)
    S.prof_enable(False)
    prof_cross = S.prof_read_all()
    S.prof_reset()
    idx.close()
    keep = (count.astype(np.int64) > a.min_neighbors) & np.isfinite(mp[:, :3]).all(1)
    pick = lambda prof: {k: ms for k, (ms, _) in sorted(prof.items()) if k.startswith(("k_nb_", "k_rs_"))}  # noqa: E731
    out = {"metric": "radius neighbour self query of a merged map, ms", "unit": "ms", "value": self_ms,
           "input": {"keyframes": a.keyframes, "spacing_m": a.spacing, "ray_step_deg": a.step, "map_points": n, "radius_m": a.r,
                     "shift_m": a.shift, "generation_s": gen_s},
           "timed_repetitions": a.reps, "set_index_ms": set_ms, "set_index_ms_runs": set_runs, "query_self_ms": self_ms,
           "query_self_ms_runs": self_runs, "query_self_stats": self_stats, "query_self_pairs_per_s": self_stats["pairs_tested"] / (self_ms * 1e-3),
           "cross_query_ms": cross_ms, "cross_query_ms_runs": cross_runs, "cross_query_stats": cross_stats,
           "cross_query_pairs_per_s": cross_stats["pairs_tested"] / (cross_ms * 1e-3), "cross_query_without_neighbour": int((ccount == 0).sum()),
           "mean_count": float(count.mean()), "max_count": int(count.max()), "outlier_min_neighbors": a.min_neighbors, "outlier_kept": int(keep.sum()),
           "device_ms_by_kernel_index_and_self_query": pick(prof_self), "device_ms_by_kernel_cross_query": pick(prof_cross)}
    if a.cpu_points >= 0:
        m = a.cpu_points or n
        t0 = time.perf_counter()
        rc, rd = nbr.radius_counts(mp, mp[:m], a.r, path="tree",
                                   progress=lambda done, total: done % (1 << 20) == 0 and print(f"restatement: {done} of {total} queries", file=sys.stderr, flush=True))
        cpu_s = time.perf_counter() - t0
        rkeep = (rc.astype(np.int64) > a.min_neighbors) & np.isfinite(mp[:m, :3]).all(1)
        out["cpu_restatement"] = {"queries": m, "all_queries": m == n, "wall_s": cpu_s, "masks_equal": bool(np.array_equal(rkeep, keep[:m])),
                                  "counts_equal": bool(np.array_equal(rc, count[:m])),
                                  "min_d2_bits_equal": bool(np.array_equal(rd.view(np.uint32), d2[:m].view(np.uint32))),
                                  "ratio_to_device_set_index_plus_query_self": cpu_s * 1e3 / (set_ms + self_ms) if m == n else None}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
