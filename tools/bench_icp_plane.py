#!/usr/bin/env python3
"""Point-to-plane against point-to-point ICP on one MI355X, on tools/bench_icp.py's scene: a keyframe against the 0.4 m submap of 51
synthetic keyframes, the source displaced by (0.3, -0.2); normals of the submap at k = 10, r = 0.8 by RadiusIndex.normals_self.  Side
by side: ms per alignment (host clouds and device-resident clouds), iterations, the recovered displacement, per-kernel device times
from the library's timers, and what the normals cost.  Writes the JSON to --out and prints it as one line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join("sc-a-loam_amd", "python"), os.path.join("tools", "synth")):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np  # noqa: E402


def timed(fn, reps):
    """(median ms, last result) of reps calls after one warm-up"""
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), ms, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_plane.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-corr-dist", type=float, default=150.0, help="the reference's 150 m; the refine and the tests use 2")
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)  # torch's HIP context first, as in bench.py
    torch.zeros(1, device="cuda")
    import scaloam as S
    import scansynth
    world = scansynth.World(scansynth.HDL64, 99)
    vg = S.VoxelGrid(max_points=8000000)
    frames = [np.hstack([world.scan(k), np.zeros((world.scan(k).shape[0], 1), np.float32)]) for k in range(51)]
    tgt = np.ascontiguousarray(vg.filter(np.concatenate(frames), 0.4), np.float32)
    src = np.ascontiguousarray(vg.filter(frames[60 % 51], 0.4), np.float32).copy()
    src[:, 0] += 0.3
    src[:, 1] -= 0.2
    idx = S.RadiusIndex(tgt.shape[0], tgt.shape[0])

    def normals():
        idx.set_index(tgt, 0.8)
        return idx.normals_self(10)[0]

    normals_ms, _, nc = timed(normals, 3)
    nc = np.ascontiguousarray(nc)
    icp = S.LoopICP(max_source=src.shape[0] + 16, max_target=tgt.shape[0] + 16, max_corr_dist=a.max_corr_dist)
    d_src, d_tgt, d_nc = (torch.from_numpy(x).cuda() for x in (src, tgt, nc))
    calls = {
        "point": (lambda: icp.align(src, tgt), lambda: icp.align_device(d_src.data_ptr(), src.shape[0], d_tgt.data_ptr(), tgt.shape[0])),
        "plane": (lambda: icp.align_plane(src, tgt, nc),
                  lambda: icp.align_plane_device(d_src.data_ptr(), src.shape[0], d_tgt.data_ptr(), d_nc.data_ptr(), tgt.shape[0])),
    }
    out = {}
    for name, (host, dev) in calls.items():
        ms, all_ms, r = timed(host, a.reps)
        dms, dall, rd = timed(dev, a.reps)
        S.prof_reset()
        S.prof_enable(True)
        host()
        S.prof_enable(False)
        prof = S.prof_read_all()
        out[name] = {"ms_per_alignment": ms, "ms_all": all_ms, "device_resident_ms_per_alignment": dms, "device_resident_ms_all": dall,
                     "device_equals_host_bitwise": bool(np.array_equal(r["T"], rd["T"]) and r["fitness"] == rd["fitness"]),
                     "iterations": r["iterations"], "state": r["state"], "converged": r["converged"], "n_correspondences": r["n_correspondences"],
                     "fitness": r["fitness"], "translation": r["T"][:3, 3].tolist(),
                     "translation_error_m": float(np.abs(r["T"][:3, 3] - np.array([-0.3, 0.2, 0.0])).max()),
                     "rotation_error": float(np.abs(r["T"][:3, :3] - np.eye(3)).max()),
                     "kernels": {k: {"launches": v[1], "avg_ms": v[0] / v[1]} for k, v in prof.items() if k.startswith("k_icp") and v[1]}}
        if name == "plane":
            out[name]["plane_fitness"] = r["plane_fitness"]
    res = {"metric": "point-to-plane ICP alignments/sec", "value": 1e3 / out["plane"]["ms_per_alignment"], "unit": "alignments/s",
           "n_source": int(src.shape[0]), "n_target": int(tgt.shape[0]), "max_corr_dist": a.max_corr_dist, "reps": a.reps,
           "normals": {"k": 10, "r": 0.8, "ms": normals_ms, "nan_share": float(np.isnan(nc[:, :3]).any(1).mean()),
                       "note": "set_index + normals_self from host records, once per target"},
           "point_to_point": out["point"], "point_to_plane": out["plane"],
           "note": "ms_per_alignment: host clouds (and normals) in, result out, median of reps; the true displacement is (-0.3, 0.2, 0)"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
