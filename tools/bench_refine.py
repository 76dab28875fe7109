#!/usr/bin/env python3
"""Multiview refine (scal_refine_*, BASELINE.json config #5's "global ICP refine") on one MI355X: K synthetic HDL-64 keyframes
along the generator's path (1 m apart on a 100 m circle, so K = 2000 passes every place three times), thinned at 0.4 m, poses
perturbed by a seeded few decimetres, cap 2 m.
  (a) scal_refine_run_device, rounds = 1
  (b) in the same process, the loop of K scal_icp_align_device calls on the same clouds (each frame against the concatenation of
      the others) - what the library could do before.  Where the whole loop is projected to take more than --loop-budget seconds it
      is run on the first --loop-sample frames only and the total is extrapolated (flagged in the output).
Wall times are the median of 5 after one warm-up.  Writes one JSON document (default profiles/refine.json) and prints it.
`--only-refine` runs (a) alone, for a separate run under rocprofv3 --kernel-trace --stats (the program goes after `--`).
`--plane` measures scal_refine_run_plane_device beside (a) on the smallest set of --ks instead and writes profiles/refine_plane.json."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join("sc-a-loam_amd", "python"), os.path.join("tools", "synth")):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np  # noqa: E402


def pose12(q_xyzw, t):
    x, y, z, w = q_xyzw
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return np.hstack([R, np.asarray(t).reshape(3, 1)])


def perturb(P, rng):
    th = rng.normal(0.0, 0.01)
    D = np.eye(4)
    D[:3, :3] = [[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]]
    D[:3, 3] = rng.normal(0.0, 0.15, 3) * (1.0, 1.0, 0.2)
    T = np.eye(4)
    T[:3] = P
    return (T @ D)[:3]   # a displacement in the keyframe's own frame


def median_ms(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), r


def nn_bytes_per_query(G, goff, sample=4000, seed=3):
    """what the first sweep's ring 1 reads for a query, from the index's own counts: 27 cell look-ups (8 B key + 8 B range) and 16 B
    per point of those cells (the query's own frame included: it is read and dropped)"""
    cells = np.floor(G[:, :3]).astype(np.int64)
    key = (cells[:, 0] + 2 ** 20) | ((cells[:, 1] + 2 ** 20) << 21) | ((cells[:, 2] + 2 ** 20) << 42)
    uk, cnt = np.unique(key, return_counts=True)
    rng = np.random.default_rng(seed)
    q = cells[rng.integers(0, G.shape[0], sample)]
    cand = np.zeros(sample, np.int64)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                k = (q[:, 0] + dx + 2 ** 20) | ((q[:, 1] + dy + 2 ** 20) << 21) | ((q[:, 2] + dz + 2 ** 20) << 42)
                j = np.searchsorted(uk, k)
                j[j >= uk.shape[0]] = 0
                cand += np.where(uk[j] == k, cnt[j], 0)
    return {"cells_occupied": int(uk.shape[0]), "points_per_occupied_cell": float(G.shape[0] / uk.shape[0]),
            "ring1_candidates_per_query": float(cand.mean()), "ring1_bytes_per_query": float(27 * 16 + 16 * cand.mean() + 16)}


def plane_set(S, torch, frames, clean, poses, K, out_path, gen_s):
    """--plane: the point-to-plane refine (scal_refine_run_plane_device) beside the point refine on the same K frames in the same
    process - sweeps per round, wall median of 5, the library's per-kernel times (a separate, profiled call each), the one-off cost
    of the K per-frame normals, the median translation error before and after one round"""
    fr = frames[:K]
    off = np.concatenate([[0], np.cumsum([f.shape[0] for f in fr])]).astype(np.int64)
    n = int(off[-1])
    d_loc = torch.from_numpy(np.ascontiguousarray(np.concatenate(fr), np.float32)).cuda()
    m = max(f.shape[0] for f in fr)
    idx = S.RadiusIndex(m, m)

    def all_normals():
        ncs = []
        for f in fr:
            idx.set_index(f, 0.8)
            ncs.append(idx.normals_self(10)[0].copy())
        return ncs
    ms_n, ncs = median_ms(all_normals)
    idx.close()
    d_nc = torch.from_numpy(np.ascontiguousarray(np.concatenate(ncs), np.float32)).cuda()
    rf = S.MultiviewRefine(K, n, max_corr_dist=2.0)
    runs = {"point": lambda: rf.refine_device(d_loc.data_ptr(), off, poses[:K], rounds=1),
            "plane": lambda: rf.refine_plane_device(d_loc.data_ptr(), d_nc.data_ptr(), off, poses[:K], rounds=1)}
    before = np.linalg.norm(poses[:K, [3, 7, 11]] - clean[:K, [3, 7, 11]], axis=1)
    out = {"metric": "multiview refine, point-to-plane beside point-to-point, ms per round", "unit": "ms", "sensor": "HDL-64 synthetic", "leaf_m": 0.4,
           "max_corr_dist_m": 2.0, "rounds": 1, "keyframes": K, "points": n, "generation_s": gen_s,
           "normals": {"k": 10, "r_m": 0.8, "ms_all_frames": ms_n, "ms_per_frame": ms_n / K,
                       "finite": int(sum(int(np.isfinite(c[:, :3]).all(1).sum()) for c in ncs))},
           "translation_error_m": {"before_median": float(np.median(before))}}
    for name, fn in runs.items():
        ms, (P, res, _) = median_ms(fn)
        its = np.array([r["iterations"] for r in res])
        after = np.linalg.norm(P[:, [3, 7, 11]] - clean[:K, [3, 7, 11]], axis=1)
        S.prof_reset()
        S.prof_enable(True)
        fn()
        S.prof_enable(False)
        kern = {k: {"ms": v[0], "launches": v[1]} for k, v in S.prof_read_all().items() if v[1]}
        S.prof_reset()
        out[name] = {"refine_ms": ms, "sweeps_per_round": int(its.max()) + 1, "iterations_max": int(its.max()), "iterations_sum": int(its.sum()),
                     "ms_per_sweep": ms / (int(its.max()) + 1), "accepted": int(sum(r["accepted"] for r in res)),
                     "converged": int(sum(r["converged"] for r in res)), "states": {str(s): int(c) for s, c in zip(*np.unique([r["state"] for r in res], return_counts=True))},
                     "translation_error_after_median_m": float(np.median(after)), "kernels": kern}
    rf.close()
    out["value"] = out["plane"]["refine_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[64, 512, 2000])
    ap.add_argument("--only-refine", action="store_true")
    ap.add_argument("--loop-budget", type=float, default=60.0)
    ap.add_argument("--loop-sample", type=int, default=16)
    ap.add_argument("--plane", action="store_true", help="the point-to-plane refine beside the point refine on the smallest set of --ks")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "refine_plane.json" if a.plane else "refine.json")
    if a.plane:
        a.ks = [min(a.ks)]
    import torch
    torch.cuda.set_device(0)  # torch's HIP context first, as in bench.py
    torch.zeros(1, device="cuda")
    import scaloam as S
    import scansynth
    kmax = max(a.ks)
    world = scansynth.World(scansynth.HDL64, 99)
    vg = S.VoxelGrid(max_points=400000)
    rng = np.random.default_rng(11)
    t0 = time.perf_counter()
    frames, clean, poses = [], [], []
    for k in range(kmax):
        xyz = world.scan(k)
        frames.append(vg.filter(np.hstack([xyz, np.zeros((xyz.shape[0], 1), np.float32)]), 0.4))
        P = pose12(*world.pose(k))
        clean.append(P.reshape(12))
        poses.append(perturb(P, rng).reshape(12))
        if k % 200 == 199:
            print(f"{k + 1} keyframes generated", file=sys.stderr, flush=True)
    vg.close()
    clean, poses = np.array(clean), np.array(poses)
    gen_s = time.perf_counter() - t0
    if a.plane:
        plane_set(S, torch, frames, clean, poses, kmax, a.out, gen_s)
        return
    out = {"metric": "multiview refine, keyframes/s", "unit": "keyframes/s", "sensor": "HDL-64 synthetic", "leaf_m": 0.4, "max_corr_dist_m": 2.0,
           "rounds": 1, "generation_s": gen_s, "sets": {}}
    for K in a.ks:
        fr = frames[:K]
        off = np.concatenate([[0], np.cumsum([f.shape[0] for f in fr])]).astype(np.int64)
        n = int(off[-1])
        d_loc = torch.from_numpy(np.ascontiguousarray(np.concatenate(fr), np.float32)).cuda()
        rf = S.MultiviewRefine(K, n, max_corr_dist=2.0)
        ms_a, (Pa, ra, _) = median_ms(lambda: rf.refine_device(d_loc.data_ptr(), off, poses[:K], rounds=1))
        its = np.array([r["iterations"] for r in ra])
        before = np.linalg.norm(poses[:K, [3, 7, 11]] - clean[:K, [3, 7, 11]], axis=1)
        after = np.linalg.norm(Pa[:, [3, 7, 11]] - clean[:K, [3, 7, 11]], axis=1)
        rec = {"keyframes": K, "points": n, "refine_ms": ms_a, "keyframes_per_s": K / (ms_a * 1e-3), "iterations_max": int(its.max()),
               "iterations_sum": int(its.sum()), "host_synchronisations": int(its.max()) + 2,
               "ms_per_iteration": ms_a / (int(its.max()) + 1), "accepted": int(sum(r["accepted"] for r in ra)),
               "converged": int(sum(r["converged"] for r in ra)),
               "translation_error_m": {"before_median": float(np.median(before)), "after_median": float(np.median(after))}}
        rf.close()
        if not a.only_refine:
            # (b): the moved frames, then frame by frame against the concatenation of the others
            mm = S.MapMerge(max_points=n + 1024, max_frame_points=16)
            mm.add_batch_device(d_loc.data_ptr(), off, poses[:K], 2.0)
            ng = mm.size()
            G = mm.download().copy()
            d_G = torch.from_numpy(G).cuda()
            mm.close()
            # the frames' sizes after the near-range rule (mm_keep's arithmetic)
            lens = [int((np.sqrt((f[:, 0].astype(np.float64) ** 2 + f[:, 1].astype(np.float64) ** 2) + f[:, 2].astype(np.float64) ** 2) > 2.0).sum())
                    for f in fr]
            goff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            assert goff[-1] == ng
            icp = S.LoopICP(max_source=int(max(lens)) + 16, max_target=ng + 16, max_corr_dist=2.0)

            def loop(count):
                res = []
                for f in range(count):
                    g0, g1 = int(goff[f]), int(goff[f + 1])
                    tgt = torch.cat([d_G[:g0], d_G[g1:]])
                    torch.cuda.synchronize()   # the alignment runs on the library's own stream
                    res.append(icp.align_device(d_G.data_ptr() + 16 * g0, lens[f], tgt.data_ptr(), ng - lens[f]))
                return res
            t0 = time.perf_counter()
            loop(min(K, 4))
            est = (time.perf_counter() - t0) / min(K, 4) * K
            if est * 6 <= a.loop_budget:
                ms_b, rb = median_ms(lambda: loop(K))
                rec["single_loop"] = {"ms": ms_b, "frames_run": K, "extrapolated": False}
            else:
                m = min(K, a.loop_sample)
                t0 = time.perf_counter()
                rb = loop(m)
                ms_b = (time.perf_counter() - t0) * 1e3 / m * K
                rec["single_loop"] = {"ms": ms_b, "frames_run": m, "extrapolated": True}
            rec["single_loop"]["iterations_sum"] = int(sum(r["iterations"] for r in rb))
            rec["single_loop"]["host_synchronisations_per_frame"] = float(np.mean([r["iterations"] + 1 for r in rb]))
            rec["single_loop"]["same_T_as_refine_bitwise"] = bool(all(np.array_equal(x["T"], y["T"]) for x, y in zip(ra, rb)))
            rec["speedup_over_single_loop"] = ms_b / ms_a
            icp.close()
            if K == min(a.ks):
                rec["nn_index"] = nn_bytes_per_query(G, goff)
                # the bit-for-bit flag at the reference's cap: every frame against the loop, 20 iterations at the most
                rf150 = S.MultiviewRefine(K, n, max_corr_dist=150.0, max_iterations=20)
                icp150 = S.LoopICP(max_source=int(max(lens)) + 16, max_target=ng + 16, max_corr_dist=150.0, max_iterations=20)
                _, r150, _ = rf150.refine_device(d_loc.data_ptr(), off, poses[:K], rounds=1)
                icp = icp150
                s150 = loop(K)
                rec["cap150_equals_single_loop_bitwise"] = bool(all(
                    np.array_equal(x["T"], y["T"]) and x["iterations"] == y["iterations"] and x["state"] == y["state"] for x, y in zip(r150, s150)))
                rf150.close(), icp150.close()
            del d_G
        out["sets"][str(K)] = rec
        out["value"] = rec["keyframes_per_s"]   # of the largest set run so far
        del d_loc
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:   # after every set: a later, larger one may be cut short
            json.dump(out, f, indent=1)
            f.write("\n")
        print(f"K = {K} done", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
