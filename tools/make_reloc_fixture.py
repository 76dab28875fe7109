#!/usr/bin/env python3
"""Record the CPU oracle's answer to the premise of scal_reloc's yaw guess (tests/golden/reloc_premise_oracle.npz): golden KAIST03
keyframe 5 turned by 90 degrees about z, against keyframes 0 / 7 / 20 brought into keyframe 7's frame by their golden poses, all at
the 0.4 m leaf, with the reference's ICP settings and the identity as the start.  The run takes 100 iterations of a kd-tree ICP
(about a quarter of a minute), so the GPU test reads the record; tests/test_reloc_cpu.py repeats the run and holds the record to it.
Needs only the oracle (make -C oracle) and the golden files."""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "sc-a-loam_amd", "python"))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def turn(a, deg, ty=0.0):
    """the cloud turned by deg about z, then shifted by ty along y (f64, rounded to f32)"""
    th = np.deg2rad(deg)
    R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    o = a.copy()
    o[:, :3] = (a[:, :3].astype(np.float64) @ R.T + np.array([0.0, ty, 0.0])).astype(np.float32)
    return o


def apply34(M, a):
    """local2global's f32 arithmetic: ((m0 x + m1 y) + m2 z) + m3 per coordinate"""
    M = np.asarray(M, np.float32)
    x, y, z = a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()
    o = a.copy()
    for r in range(3):
        o[:, r] = ((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3]
    return o


def premise_clouds():
    """(source, target) on the CPU oracle: keyframe 5 turned by 90 degrees, and keyframes 0 / 7 / 20 in keyframe 7's frame, all at 0.4 m"""
    import oracle_py as O
    import scaloam as S
    from scaloam import formats
    poses = np.load(os.path.join(GOLDEN, "KAIST03_poses21.npy")).reshape(-1, 12).astype(np.float64)
    kf = {j: O.voxel_grid(np.load(os.path.join(GOLDEN, f"KAIST03_{j:06d}.npy")), 0.4)[0] for j in (0, 7, 20)}
    parts = [kf[j] if j == 7 else apply34(S.relative_transform(poses[7], poses[j]), kf[j]) for j in (0, 7, 20)]
    src, _ = O.voxel_grid(turn(formats.read_pcd(os.path.join(GOLDEN, "KAIST03_000005.pcd")), 90.0), 0.4)
    return src, O.voxel_grid(np.concatenate(parts), 0.4)[0]


def main():
    import oracle_py as O
    src, tgt = premise_clouds()
    r = O.icp_align(src, tgt)
    np.savez(os.path.join(GOLDEN, "reloc_premise_oracle.npz"), T=r["T"], fitness=r["fitness"], iterations=r["iterations"], state=r["state"],
             converged=r["converged"], n_src=src.shape[0], n_tgt=tgt.shape[0])
    print("identity start:", r["fitness"], r["iterations"], r["state"], src.shape, tgt.shape)


if __name__ == "__main__":
    main()
