#!/usr/bin/env python3
"""Relocalise scans against a session the pose-graph node saved (laserPosegraphOptimization.cpp:178-259, :695-700):

    relocalize_session.py <session_dir> <query.pcd | directory of .pcd> ...

<session_dir> holds Scans/NNNNNN.pcd (keyframe clouds in their local frames) and optimized_poses.txt (one 3x4 pose per keyframe); with
--scd the descriptors are reloaded from SCDs/NNNNNN.scd (saveScancontextAndKeys) instead of being rebuilt from the clouds.  Every
query goes through scal_reloc_query_batch; relocalized_poses.txt (in --out, default the current directory) gets one line per ACCEPTED
query in the pose files' own format, and a JSON summary with every query's record is printed."""
import argparse
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sc-a-loam_amd", "python"))
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("session_dir")
    ap.add_argument("queries", nargs="+", help=".pcd files or directories of them")
    ap.add_argument("--scd", action="store_true", help="reload SCDs/NNNNNN.scd instead of rebuilding the descriptors")
    ap.add_argument("--submap-half", type=int, default=0, help="keyframes either side of the candidate in the ICP target (0 = 25, -1 = none)")
    ap.add_argument("--no-yaw-guess", action="store_true", help="start ICP from the identity, as the reference's loop verification does")
    ap.add_argument("--out", default=".")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import scaloam as S
    from scaloam import formats
    scans = sorted(glob.glob(os.path.join(a.session_dir, "Scans", "*.pcd")))
    poses = formats.read_poses(os.path.join(a.session_dir, "optimized_poses.txt"))
    if not scans or len(scans) != poses.shape[0]:
        sys.exit(f"{a.session_dir}: {len(scans)} keyframe clouds under Scans/ but {poses.shape[0]} poses in optimized_poses.txt")
    files = []
    for q in a.queries:
        files += sorted(glob.glob(os.path.join(q, "*.pcd"))) if os.path.isdir(q) else [q]
    clouds = [formats.read_pcd(s) for s in scans]
    queries = [formats.read_pcd(f) for f in files]
    # the arena holds the filtered clouds (no larger than the raw ones); the work buffers one query or one submap before its filter
    h = 25 if a.submap_half == 0 else max(a.submap_half, 0)
    largest = max(c.shape[0] for c in clouds)
    work = max([q.shape[0] for q in queries] + [min(2 * h + 1, len(clouds)) * largest, 1])
    rl = S.Relocalizer(len(clouds), max(1, sum(c.shape[0] for c in clouds)), max_query_points=work, submap_half=a.submap_half,
                       no_yaw_guess=a.no_yaw_guess, device=a.device)
    for i, (c, P) in enumerate(zip(clouds, poses)):
        desc = formats.read_scd(os.path.join(a.session_dir, "SCDs", os.path.splitext(os.path.basename(scans[i]))[0] + ".scd")) if a.scd else None
        rl.add_keyframe(c, P, desc)
    res = rl.query_batch(queries)
    rl.close()
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "relocalized_poses.txt")
    with open(path, "w") as f:
        for r in res:
            if r["status"] == 1:
                f.write(formats.format_pose_line(r["pose12"]) + "\n")
    names = {0: "no place found", 1: "accepted", 2: "rejected by ICP"}
    print(json.dumps({"session": a.session_dir, "keyframes": len(clouds), "queries": len(files), "accepted": sum(r["status"] == 1 for r in res),
                      "rejected": sum(r["status"] == 2 for r in res), "no_place": sum(r["status"] == 0 for r in res), "poses_file": path,
                      "results": [dict(query=f, status=names[r["status"]], keyframe=r["sc"]["loop_id"], sc_distance=r["sc"]["min_dist"],
                                       yaw_rad=r["sc"]["yaw"], fitness=r["icp"]["fitness"] if r["status"] else None,
                                       iterations=r["icp"]["iterations"], pose12=[float(v) for v in r["pose12"]] if r["status"] else None)
                                  for f, r in zip(files, res)]}))


if __name__ == "__main__":
    main()
