#!/usr/bin/env python3
"""Convert a few of the reference's sample keyframe scans (data files, not source) into
small .npy fixtures under tests/golden/, and record the answers of the reference's vendored
nanoflann (oracle/_ref, built by oracle/Makefile) on the seeded inputs of the tests that pin the
oracle's ring-key search against it (tests/golden/ref_nanoflann_knn.npz).

Source data: /root/reference/utils/sample_data/{KAIST03,Seosan01}/Scans/*.pcd
(binary PCD, fields x y z intensity, float32; parse by POINTS, the files carry trailing pad bytes;
SURVEY.md section 4).  Run in the build container only; the GPU box has no /root/reference.
"""
import os, sys
import numpy as np

REF = "/root/reference/utils/sample_data"
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden")
KAIST03_STORED = (0, 5, 7, 20)  # keyframes stored whole (KAIST03_000005 as the reference's own .pcd)


def read_pcd(path):
    b = open(path, "rb").read()
    k = b.index(b"DATA binary\n") + len(b"DATA binary\n")
    hdr = b[:k].decode()
    n = int([l for l in hdr.splitlines() if l.startswith("POINTS")][0].split()[1])
    fields = [l for l in hdr.splitlines() if l.startswith("FIELDS")][0].split()[1:]
    assert fields == ["x", "y", "z", "intensity"], fields
    return np.frombuffer(b, dtype=np.float32, count=n * 4, offset=k).reshape(n, 4).copy()


def main():
    os.makedirs(OUT, exist_ok=True)
    picks = [("KAIST03", 0), ("KAIST03", 7), ("KAIST03", 20), ("Seosan01", 0), ("Seosan01", 11)]
    for ds, i in picks:
        a = read_pcd(f"{REF}/{ds}/Scans/{i:06d}.pcd")
        np.save(f"{OUT}/{ds}_{i:06d}.npy", a)
        print(ds, i, a.shape, a[:, :3].min(0), a[:, :3].max(0))
    # poses of the first 21 keyframes (KITTI 3x4 row-major, one line each)
    for ds in ("KAIST03", "Seosan01"):
        P = np.loadtxt(f"{REF}/{ds}/optimized_poses.txt")[:21]
        np.save(f"{OUT}/{ds}_poses21.npy", P)
    # the other 17 KAIST03 keyframes, only the points that decide the ring-id pin (test_all_kaist03_sample_scans_pin_ring_ids_and_order):
    # the OS1-64 scanID is monotone in the elevation angle, so a ring's lowest and highest points bound every point between them.
    # Per keyframe: the 32 points nearest each ring's lower and upper edge, the 32 nearest the sensor (minimum-range filter) and a
    # seeded 2 % sample, in file order, with their positions in the file and round(intensity) (= the scanID the reference stored).
    rng = np.random.default_rng(2103)
    edges = {}
    for i in range(21):
        if i in KAIST03_STORED:
            continue
        a = read_pcd(f"{REF}/KAIST03/Scans/{i:06d}.pcd")
        x = a[:, :3].astype(np.float64)
        ang = np.degrees(np.arctan(x[:, 2] / np.hypot(x[:, 0], x[:, 1])))
        ring = np.round(a[:, 3]).astype(np.int64)
        keep = [np.argsort(np.linalg.norm(x, axis=1))[:32], np.flatnonzero(rng.uniform(size=a.shape[0]) < 0.02)]
        for r in np.unique(ring):
            idx = np.flatnonzero(ring == r)
            order = idx[np.argsort(ang[idx], kind="stable")]
            keep += [order[:32], order[-32:]]
        sel = np.unique(np.concatenate(keep))
        edges[f"{i:06d}_index"] = sel.astype(np.int32)
        edges[f"{i:06d}_xyz"] = a[sel, :3].copy()
        edges[f"{i:06d}_ring"] = ring[sel].astype(np.uint8)
        edges[f"{i:06d}_n"] = np.int64(a.shape[0])
    np.savez_compressed(f"{OUT}/KAIST03_ring_edges.npz", **edges)
    nanoflann_vectors()


def nanoflann_vectors():
    """The same seeded inputs as tests/test_oracle_cpu.py's two nanoflann tests, answered by oracle/_ref."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_py as O
    assert O.ref_lib() is not None, "oracle/_ref not built (make -C oracle where the reference is present)"
    rng = np.random.default_rng(401)
    keys = rng.uniform(0.03, 4.4, (5000, 20)).astype(np.float32)
    q = rng.uniform(0.03, 4.4, (64, 20)).astype(np.float32)
    knn_idx, knn_d = O.ref_ringkey_knn(keys, q, 3)
    # detectLoopClosureID's tree: rebuilt every 30 queries from all keys but the newest 30
    rng = np.random.default_rng(9)
    m = O.SCManager()
    descs = [rng.uniform(-2, 18, (20, 60)) * (rng.uniform(size=(20, 60)) < 0.5) for _ in range(95)]
    keys, detect_cand = [], np.full((95, 3), -1, np.int32)
    size_at_rebuild, counter = 0, 0
    for i, d in enumerate(descs):
        m.saveScancontextAndKeys(d)
        keys.append(m.get(i)[1])
        if i + 1 < 31:
            continue
        if counter % 30 == 0:
            size_at_rebuild = i + 1
        counter += 1
        n_tree = size_at_rebuild - 30
        detect_cand[i, :min(3, n_tree)] = O.ref_ringkey_knn(np.stack(keys[:n_tree]), keys[i][None, :], 3)[0][0][:min(3, n_tree)]
    np.savez_compressed(f"{OUT}/ref_nanoflann_knn.npz", knn_idx=knn_idx, knn_d=knn_d, detect_cand=detect_cand)


if __name__ == "__main__":
    main()
