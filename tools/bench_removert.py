#!/usr/bin/env python3
"""Dynamic-point removal (scal_removert_*) on one MI355X.
Session: K synthetic keyframes `--spacing` metres apart inside a tunnel, each with a ball the other keyframes look through
(tools/removert_scene.py corridor_session; scans are ray casts on a `--step` degree grid); the map is the union of the scans.
The tunnel's walls are seen at grazing angles, where the ranges inside one pixel differ by more than diff_thres: most of the map is
flagged, as a range-image test flags such surfaces.  The cost of a pair does not depend on the answer; the labelled (ball) points
found are reported beside the flagged total.
  - wall ms of set_map (upload + binning) and of run (scan upload, images, test, mask download), median of --reps after a warm-up;
  - (point, keyframe) pairs per second over the run's wall time, as tested after the culling and as the brute-force equivalent n K;
  - device ms per phase from the library's own per-kernel timers, in a separate pass (they add a little to every launch);
  - the CPU restatement's wall time on the same input (one run; --cpu-keyframes N restricts it to the first N keyframes and says so),
    and whether its mask equals the device's.
Writes one JSON document (default profiles/removert.json) and prints it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sc-a-loam_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

PHASES = (("bin", ("k_rv_bounds", "k_rv_count", "k_rv_scatter")), ("images", ("k_rv_images",)), ("test", ("k_rv_test",)),
          ("finish", ("k_rv_finish",)))


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
    ap.add_argument("--max-keyframes", type=int, default=0, help="keyframes resident at once (0 = all: one chunk)")
    ap.add_argument("--reps", type=int, default=5, help="timed repetitions after the warm-up; the median is reported")
    ap.add_argument("--cpu-keyframes", type=int, default=0, help="keyframes the CPU restatement runs (0 = all, -1 = skip it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "removert.json"))
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)  # torch's HIP context first, as in bench.py
    torch.zeros(1, device="cuda")
    import scaloam as S
    from scaloam import removert as rv
    import removert_scene
    remove_res, revert_res = (2.5, 2.0, 1.5), (5.0,)
    t0 = time.perf_counter()
    mp, scans, P, labels = removert_scene.corridor_session(a.keyframes, a.spacing, a.step, seed=7)
    gen_s = time.perf_counter() - t0
    n, K = mp.shape[0], len(scans)
    rm = S.Removert(n, a.max_keyframes or K, sum(s.shape[0] for s in scans), max_resolutions=4)
    set_ms, set_runs, _ = timed(lambda: rm.set_map(mp), a.reps)
    run_ms, run_runs, (mask, stats) = timed(lambda: rm.run(scans, P, remove_res, revert_res), a.reps)
    S.prof_reset()
    S.prof_enable(True)
    rm.set_map(mp)
    rm.run(scans, P, remove_res, revert_res)
    S.prof_enable(False)
    prof = S.prof_read_all()
    S.prof_reset()
    rm.close()
    phases = {name: float(sum(ms for k, (ms, _) in prof.items() if k.startswith(pre))) for name, pre in PHASES}
    out = {"metric": "dynamic-point removal from a merged keyframe map, ms per run", "unit": "ms", "value": run_ms,
           "session": {"keyframes": K, "spacing_m": a.spacing, "ray_step_deg": a.step, "map_points": n,
                       "points_per_scan": int(np.mean([s.shape[0] for s in scans])), "generation_s": gen_s,
                       "remove_res": remove_res, "revert_res": revert_res, "keyframes_resident": a.max_keyframes or K},
           "timed_repetitions": a.reps, "set_map_ms": set_ms, "set_map_ms_runs": set_runs, "run_ms": run_ms, "run_ms_runs": run_runs,
           "stats": stats, "labelled_points": int(labels.sum()), "labelled_found": int(mask[labels].sum()),
           "pairs_per_s_tested": stats["pairs_tested"] / (run_ms * 1e-3), "pairs_per_s_bruteforce_equivalent": stats["pairs_bruteforce"] / (run_ms * 1e-3),
           "device_ms_by_phase": phases, "device_ms_by_kernel": {k: ms for k, (ms, _) in sorted(prof.items()) if k.startswith("k_rv_")}}
    if a.cpu_keyframes >= 0:
        kc = a.cpu_keyframes or K
        t0 = time.perf_counter()
        ref = rv.remove_dynamic_points(mp, scans[:kc], P[:kc], remove_res, revert_res, keep_images=False)
        cpu_s = time.perf_counter() - t0
        out["cpu_restatement"] = {"keyframes": kc, "all_keyframes": kc == K, "wall_s": cpu_s, "margin_pixels": ref.margin,
                                  "mask_equals_device": bool(np.array_equal(ref.mask, mask)) if kc == K else None,
                                  "speedup_run_wall": cpu_s * 1e3 / run_ms if kc == K else None}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
