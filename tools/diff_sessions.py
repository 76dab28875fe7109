#!/usr/bin/env python3
"""What changed between two saved sessions that share a frame (scaloam.nbr.map_diff on the GPU: scal_nbr_* and scal_removert_*).
Reads two session directories as the reference saves them (Scans/*.pcd + optimized_poses.txt), merges each into its map
(near-range removal, VoxelGrid(--leaf)), and labels every point of either map against the other session: in both maps, missing from
the other map and never looked at by it, or missing although the other session's rays went through the place.  Writes, into --out-dir
(default: the new session's directory),
  diff_disappeared.pcd  points of the old map the new session saw through
  diff_appeared.pcd     points of the new map the old session saw through
  map_updated.pcd       the old map without the disappeared points, followed by the new map's points the old map does not hold
The sessions are taken as sharing a frame: --poses-new names the new session's poses in the old session's frame
(tools/relocalize_session.py is how to get them); by default the new session's own optimized_poses.txt is used."""
import argparse
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sc-a-loam_amd", "python"))
import numpy as np  # noqa: E402


def load(S, F, ses, poses_file, near, leaf):
    files = sorted(glob.glob(os.path.join(ses, "Scans", "*.pcd")))
    poses = np.asarray(F.read_poses(poses_file or os.path.join(ses, "optimized_poses.txt")), np.float64).reshape(-1, 12)
    k = min(len(files), poses.shape[0])
    scans, poses = [F.read_pcd(f) for f in files[:k]], poses[:k]
    mm = S.MapMerge(max_points=sum(s.shape[0] for s in scans) + 1, max_frame_points=max(s.shape[0] for s in scans))
    for s, p in zip(scans, poses):
        mm.add(s, p, near)
    mp = mm.downsample(leaf) if leaf > 0 else mm.download().copy()
    mm.close()
    return mp, scans, poses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("session_old")
    ap.add_argument("session_new")
    ap.add_argument("--poses-new", default=None, help="the new session's poses in the old session's frame (default: its own optimized_poses.txt)")
    ap.add_argument("--r", type=float, default=None, help="radius within which a point of the other map makes a point common (default 0.8)")
    ap.add_argument("--leaf", type=float, default=0.4, help="VoxelGrid leaf of both maps (0 = none)")
    ap.add_argument("--near", type=float, default=2.0)
    ap.add_argument("--remove-res", type=float, nargs="+", default=[2.5, 2.0, 1.5])
    ap.add_argument("--revert-res", type=float, nargs="*", default=[5.0])
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    import scaloam as S
    from scaloam import formats as F, nbr
    r = nbr.DEFAULT_RADIUS if a.r is None else a.r
    old_map, old_scans, old_poses = load(S, F, a.session_old, None, a.near, a.leaf)
    new_map, new_scans, new_poses = load(S, F, a.session_new, a.poses_new, a.near, a.leaf)
    kw = dict(remove_res=tuple(a.remove_res), revert_res=tuple(a.revert_res))
    l_old, s_old = nbr.map_diff(old_map, new_map, new_scans, new_poses, r, device=True, **kw)
    l_new, s_new = nbr.map_diff(new_map, old_map, old_scans, old_poses, r, device=True, **kw)
    print(f"old map: {old_map.shape[0]} points, {s_old['common']} common, {s_old['unobserved']} not observed by the new session, {s_old['changed']} disappeared")
    print(f"new map: {new_map.shape[0]} points, {s_new['common']} common, {s_new['unobserved']} newly explored, {s_new['changed']} appeared")
    out_dir = a.out_dir or a.session_new
    os.makedirs(out_dir, exist_ok=True)
    for name, pts in (("diff_disappeared.pcd", old_map[l_old == nbr.CHANGED]), ("diff_appeared.pcd", new_map[l_new == nbr.CHANGED]),
                      ("map_updated.pcd", nbr.update_map(old_map, l_old, new_map, l_new))):
        F.write_pcd_binary(os.path.join(out_dir, name), pts)
        print("written", os.path.join(out_dir, name), pts.shape[0], "points")


if __name__ == "__main__":
    main()
