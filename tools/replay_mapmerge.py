#!/usr/bin/env python3
"""Replay of utils/python/makeMergedMap.py on the GPU: reads a session directory as the reference saves it (Scans/*.pcd +
optimized_poses.txt), merges the keyframes into the global frame (near-range removal 2 m) with scal_mapmerge_*, writes the map as
a binary PCD.  `--check` also runs the CPU oracle and compares bit for bit.  `--refine ROUNDS` first refines the poses with
scal_refine_* (every keyframe thinned at --refine-leaf and aligned against all the others, keyframe 0 held), writes them to
refined_poses.txt beside the session's optimized_poses.txt and merges with them; with `--refine-plane K[,R]` the refine uses the
point-to-plane metric (scal_refine_run_plane) on each thinned keyframe's own normals, the plane through a point's K nearest
neighbours within R (default 0.8 m) of its keyframe (scal_nbr_normals_self).  `--remove-dynamic` runs scal_removert_* on the merged map
where it lies in device memory, with the poses the merge used (the refined ones after --refine), reports the counts and writes the
static points beside the map as *_static.pcd - after VoxelGrid(--leaf) if a leaf is given.  `--radius-filter R,MIN` drops the isolated
returns before either map is written: a point stays iff more than MIN points of the merged map, itself included, lie within R
(scal_nbr_*, the map indexed where it lies in device memory; scaloam.nbr.radius_outlier_mask is the rule).  `--sor-filter
MEAN_K,STD_MUL[,R0]` drops the statistical outliers in the same place: a point stays iff the mean distance to its MEAN_K nearest
neighbours is at most the map's mean of that figure plus STD_MUL standard deviations (scaloam.nbr.statistical_outlier_mask on the
device: exact k-NN from scal_nbr_knn*, the search radius doubled from R0, default 0.5 m, until every list is full).  With both filters
each is computed on the whole merged map and a point has to pass both.  `--normals K[,R]` writes the map that was written - after the
filters - once more beside it as *_normals.pcd with normal_x normal_y normal_z curvature per point: the plane through each point's K
nearest neighbours within R (default 0.8 m) of the written map, scal_nbr_normals_self (scaloam.nbr.estimate_normals is the rule); the
normals are not oriented, and a point with fewer than 3 neighbours within R has NaN there."""
import argparse
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", os.path.join("sc-a-loam_amd", "python")):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("data_dir", help="session directory: Scans/*.pcd and optimized_poses.txt")
    ap.add_argument("--range", type=int, nargs=2, default=None, help="keyframe index range [a, b) like scan_idx_range_to_stack")
    ap.add_argument("--near", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--refine", type=int, default=0, metavar="ROUNDS", help="multiview refine of the poses before the merge")
    ap.add_argument("--refine-leaf", type=float, default=0.4)
    ap.add_argument("--max-corr", type=float, default=2.0)
    ap.add_argument("--remove-dynamic", action="store_true", help="remove the points other keyframes look through (scal_removert)")
    ap.add_argument("--remove-res", type=float, nargs="+", default=[2.5, 2.0, 1.5], help="remove resolutions, degrees per pixel")
    ap.add_argument("--revert-res", type=float, nargs="*", default=[5.0], help="revert resolutions, degrees per pixel (may be empty)")
    ap.add_argument("--leaf", type=float, default=0.0, help="VoxelGrid leaf for the static map (0 = none)")
    ap.add_argument("--radius-filter", default=None, metavar="R,MIN", help="keep a point iff more than MIN map points lie within R metres of it")
    ap.add_argument("--sor-filter", default=None, metavar="MEAN_K,STD_MUL[,R0]",
                    help="keep a point iff its mean distance to its MEAN_K nearest neighbours is within STD_MUL standard deviations of the map's mean")
    ap.add_argument("--normals", default=None, metavar="K[,R]", help="write *_normals.pcd: normals and curvature from the K nearest neighbours within R")
    ap.add_argument("--refine-plane", default=None, metavar="K[,R]",
                    help="with --refine: the point-to-plane metric on each thinned keyframe's own normals, K nearest neighbours within R")
    a = ap.parse_args()
    refine_plane = None
    if a.refine_plane:
        try:
            f = a.refine_plane.split(",")
            refine_plane = (int(f[0]), float(f[1]) if len(f) > 1 else 0.8)
            ok = len(f) in (1, 2) and 3 <= refine_plane[0] <= 64 and np.isfinite(refine_plane[1]) and refine_plane[1] > 0
        except (ValueError, IndexError):
            ok = False
        if not ok:
            ap.error("--refine-plane takes K[,R]: K in 3 .. 64, R > 0")
        if a.refine <= 0:
            ap.error("--refine-plane needs --refine ROUNDS")
    normals = None
    if a.normals:
        try:
            f = a.normals.split(",")
            normals = (int(f[0]), float(f[1]) if len(f) > 1 else 0.8)
            ok = len(f) in (1, 2) and 3 <= normals[0] <= 64 and np.isfinite(normals[1]) and normals[1] > 0
        except (ValueError, IndexError):
            ok = False
        if not ok:
            ap.error("--normals takes K[,R]: K in 3 .. 64, R > 0")
    sor = None
    if a.sor_filter:
        try:
            f = a.sor_filter.split(",")
            sor = (int(f[0]), float(f[1]), float(f[2]) if len(f) > 2 else 0.5)
            ok = len(f) in (2, 3) and 1 <= sor[0] <= 63 and np.isfinite(sor[1]) and np.isfinite(sor[2]) and sor[2] > 0
        except (ValueError, IndexError):
            ok = False
        if not ok:
            ap.error("--sor-filter takes MEAN_K,STD_MUL[,R0]: MEAN_K in 1 .. 63, STD_MUL finite, R0 > 0")
    import scaloam as S
    from scaloam import formats as F
    files = sorted(glob.glob(os.path.join(a.data_dir, "Scans", "*.pcd")))
    poses = F.read_poses(os.path.join(a.data_dir, "optimized_poses.txt"))
    lo, hi = a.range if a.range else (0, min(len(files), len(poses)))
    frames = [F.read_pcd(f) for f in files[lo:hi]]
    poses = np.asarray(poses[lo:hi], np.float64).reshape(-1, 12)
    if a.refine > 0:
        vg = S.VoxelGrid(max_points=max(f.shape[0] for f in frames))
        thin = [vg.filter(f, a.refine_leaf) for f in frames]
        rf = S.MultiviewRefine(len(thin), sum(t.shape[0] for t in thin) + 1, max_corr_dist=a.max_corr)
        fixed = np.zeros(len(thin), np.uint8)
        fixed[0] = 1
        if refine_plane:
            idx = S.RadiusIndex(max(t.shape[0] for t in thin), max(t.shape[0] for t in thin))
            ncs = []
            for t in thin:
                idx.set_index(t, refine_plane[1])
                ncs.append(idx.normals_self(refine_plane[0])[0].copy())
            idx.close()
            print(f"refine-plane: {sum(int(np.isfinite(n[:, 0]).sum()) for n in ncs)} of {sum(t.shape[0] for t in thin)} thinned points have a "
                  f"normal ({refine_plane[0]} nearest within {refine_plane[1]} m of their own keyframe)")
            poses, res, run = rf.refine_plane(thin, ncs, poses, fixed=fixed, rounds=a.refine, near_thres=a.near)
        else:
            poses, res, run = rf.refine(thin, poses, fixed=fixed, rounds=a.refine, near_thres=a.near)
        print(f"refine: {run} round(s), {sum(r['accepted'] for r in res)} of {len(res)} keyframes accepted in the last one")
        path = os.path.join(a.data_dir, "refined_poses.txt")
        F.write_poses(path, poses)
        print("written", path)
        vg.close(), rf.close()
    mm = S.MapMerge(max_points=sum(f.shape[0] for f in frames) + 1, max_frame_points=max(f.shape[0] for f in frames))
    for f, p in zip(frames, poses):
        mm.add(f, p, a.near)
    out = mm.download()
    print(f"{len(frames)} keyframes, {sum(f.shape[0] for f in frames)} points in, {out.shape[0]} points in the map")
    if a.check:
        import oracle_py as O
        ref = O.mapmerge(frames, poses, a.near)
        print("bit-exact vs oracle:", bool(ref.shape == out.shape and np.array_equal(ref.view(np.uint32), out.view(np.uint32))))
    keep = None
    if a.radius_filter:
        r, min_nb = a.radius_filter.split(",")
        idx = S.RadiusIndex(out.shape[0] + 1, 1)
        idx.set_index_device(mm, float(r))
        count, _ = idx.query_self()
        idx.close()
        keep = (count.astype(np.int64) > int(min_nb)) & np.isfinite(out[:, :3]).all(1)
        print(f"radius-filter: {int(keep.sum())} of {out.shape[0]} points have more than {int(min_nb)} points within {float(r)} m")
    if sor:
        from scaloam import nbr
        good = nbr.statistical_outlier_mask(out, sor[0], sor[1], sor[2], device=True)
        print(f"sor-filter: {int(good.sum())} of {out.shape[0]} points lie within {sor[1]} standard deviations of the mean {sor[0]}-neighbour distance")
        keep = good if keep is None else keep & good
    path = a.out or os.path.join(a.data_dir, f"map_{lo}_to_{hi}_with_intensity.pcd")
    F.write_pcd_binary(path, out if keep is None else out[keep])
    print("written", path)
    if normals:
        from scaloam import nbr
        kept = out if keep is None else out[keep]
        nc, _ = nbr.estimate_normals(kept, normals[0], normals[1], device=True)
        print(f"normals: {int(np.isfinite(nc[:, 0]).sum())} of {kept.shape[0]} points have at least 3 neighbours within {normals[1]} m")
        npath = os.path.splitext(path)[0] + "_normals.pcd"
        F.write_pcd_normals_binary(npath, kept, nc)
        print("written", npath)
    if a.remove_dynamic:
        n_res = len(a.remove_res) + len(a.revert_res)
        rm = S.Removert(out.shape[0] + 1, min(len(frames), 256), 256 * max(f.shape[0] for f in frames), max_resolutions=n_res,
                        min_res_deg=min(a.remove_res + a.revert_res + [1.0]))
        mask, st = rm.remove_device(mm, frames, poses, a.remove_res, a.revert_res)
        print(f"remove-dynamic: {st['dynamic']} of {st['points']} points dynamic; {st['pairs_tested']} of {st['pairs_bruteforce']} "
              f"(point, keyframe) pairs tested")
        static = rm.compact(0) if keep is None else out[keep & (mask == 0)]
        rm.close()
        if a.leaf > 0 and static.shape[0]:
            vg = S.VoxelGrid(max_points=static.shape[0])
            static = vg.filter(static, a.leaf)
            vg.close()
            print(f"VoxelGrid({a.leaf}): {static.shape[0]} points")
        path = os.path.splitext(path)[0] + "_static.pcd"
        F.write_pcd_binary(path, static)
        print("written", path)


if __name__ == "__main__":
    main()
