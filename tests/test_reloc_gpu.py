"""Relocalisation against a stored session (scal_reloc_*, csrc/reloc.hip) and the pieces it is made of: the between-session ScanContext
search, the cross-session distance blocks, ICP with an initial guess.

Yardsticks: the reference's own nanoflann (where oracle/_ref is built) and its numpy restatement for the ring-key search, O.sc_distance /
O.sc_distance_full for the descriptor distances (1e-12), O.icp_align for the alignment (1e-9), O.voxel_grid for the filters (bit-equal),
and - for the object itself - the same chain rebuilt outside it from S.VoxelGrid, S.SCManager and S.LoopICP, bit for bit.
Clouds are the golden KAIST03 keyframes 0 / 7 / 20, KAIST03_000005.pcd and the two Seosan01 keyframes."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
YAWS = (0.0, 90.0, 180.0, -120.0, 93.0)
TY = 0.3  # lateral offset of every end-to-end query [m]


# ------------------------------------------------------------------------------------------------------------------ helpers
def _random_descs(rng, n, revisit_every=7):
    """Descriptors with the statistics of real ones (occupancy ~0.5, heights -2.8..18) plus shifted revisits."""
    out = []
    for i in range(n):
        if i >= 40 and i % revisit_every == 0:
            j = int(rng.integers(0, i - 35))
            d = np.roll(out[j], int(rng.integers(0, 60)), axis=1) + rng.normal(0, 0.05, (20, 60)) * (out[j] != 0)
        else:
            d = rng.uniform(-2.0, 18.0, (20, 60)) * (rng.uniform(size=(20, 60)) < 0.5)
            d[:, rng.integers(0, 60, 3)] = 0.0  # empty sectors
        out.append(d)
    return out


def _turn4(deg, ty=0.0):
    th = np.deg2rad(deg)
    M = np.eye(4)
    M[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
    M[1, 3] = ty
    return M


def _turn(a, deg, ty=0.0):
    """the cloud turned by deg about z, then shifted by ty along y"""
    M = _turn4(deg, ty)
    o = a.copy()
    o[:, :3] = (a[:, :3].astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    return o


def _apply34(M, a):
    """k_icp_apply / local2global: ((m0 x + m1 y) + m2 z) + m3 per coordinate, every operation rounded to f32"""
    M = np.asarray(M, np.float32)
    x, y, z = a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()
    o = a.copy()
    for r in range(3):
        o[:, r] = ((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3]
    return o


def _P4(p):
    M = np.eye(4)
    M[:3] = np.asarray(p, np.float64).reshape(3, 4)
    return M


def _pose_error(T, want):
    ang = np.degrees(np.arccos(np.clip((np.trace(T[:3, :3] @ want[:3, :3].T) - 1) / 2, -1, 1)))
    return float(np.linalg.norm(T[:3, 3] - want[:3, 3])), float(ang)


def _nn_fitness(cloud, tgt):
    """getFitnessScore of a cloud as it stands: mean squared distance to the exact nearest target point, the distance in the f32
    arithmetic of FLANN's L2_Simple ((dx dx + dy dy) + dz dz), the mean in f64"""
    t = np.ascontiguousarray(tgt[:, :3], np.float32)
    best = np.empty(cloud.shape[0], np.float32)
    for i in range(0, cloud.shape[0], 256):
        c = cloud[i:i + 256, :3].astype(np.float32)
        dx, dy, dz = c[:, None, 0] - t[None, :, 0], c[:, None, 1] - t[None, :, 1], c[:, None, 2] - t[None, :, 2]
        best[i:i + 256] = ((dx * dx + dy * dy) + dz * dz).min(1)
    return float(best.astype(np.float64).sum() / cloud.shape[0])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    """two result records (nested dicts of numbers and arrays), bit for bit"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, float):
        return isinstance(b, float) and np.float64(a).tobytes() == np.float64(b).tobytes()
    return type(a) is type(b) and a == b


def _icp_same(a, b):
    return all(_same(a[k], b[k]) for k in ("converged", "iterations", "state", "n_correspondences", "fitness", "T"))


def _ring_keys(O, descs):
    """eig2stdvec of makeRingkeyFromScancontext: row means in double, cast to float"""
    return np.stack([O.sc_keys(d)[0] for d in descs]).astype(np.float32)


def _key_dists(keys, q):
    """nanoflann L2_Adaptor<float>: five groups of four, f32"""
    diff = (q[None, :] - keys).astype(np.float32)
    sq = (diff * diff).astype(np.float32)
    acc = np.zeros(keys.shape[0], np.float32)
    for g in range(0, 20, 4):
        acc = (acc + (((sq[:, g] + sq[:, g + 1]) + sq[:, g + 2]) + sq[:, g + 3])).astype(np.float32)
    return acc


def _between_expected(O, db, keys, q, qkey, thres=0.2):
    """detectLoopClosureIDBetweenSession for one query, from the oracle's pieces"""
    acc = _key_dists(keys, qkey)
    order = np.lexsort((np.arange(keys.shape[0]), acc))[:3]
    cand = np.zeros(3, np.int64)  # unfilled KNN slots keep the caller's zero
    cand[:len(order)] = order
    best, shift, nn = 10000000.0, 0, 0
    sc, sh = [], []
    for c in cand:
        d, s = O.sc_distance(q, db[int(c)])
        sc.append(d), sh.append(s)
        if d < best:
            best, shift, nn = d, s, int(c)
    yaw = np.float32(np.float64(np.float32(shift * 6.0)) * np.pi / 180.0)
    return dict(cand=cand, n_real=len(order), sorted_keyd=np.sort(acc), cand_sc=np.array(sc), cand_shift=np.array(sh), min_dist=best, nn_idx=nn,
                nn_shift=shift, loop_id=nn if best < thres else -1, yaw=yaw)


def _check_between(got, want):
    assert np.array_equal(got["cand"], want["cand"]), (got["cand"], want["cand"])
    assert got["nn_idx"] == want["nn_idx"] and got["loop_id"] == want["loop_id"] and got["nn_shift"] == want["nn_shift"]
    assert np.float32(got["yaw"]).tobytes() == np.float32(want["yaw"]).tobytes()
    assert abs(got["min_dist"] - want["min_dist"]) <= 1e-12
    assert np.abs(got["cand_sc"] - want["cand_sc"]).max() <= 1e-12 and np.array_equal(got["cand_shift"], want["cand_shift"])


# ------------------------------------------------------------------------------------------------- 1. between-session search
def test_between_session_search_matches_the_reference_kdtree(O, S):
    rng = np.random.default_rng(2024)
    db = _random_descs(rng, 48)
    queries = []
    for _ in range(20):  # revisits: shifted, noisy copies of database entries
        j = int(rng.integers(0, 48))
        queries.append(np.roll(db[j], int(rng.integers(0, 60)), axis=1) + rng.normal(0, 0.05, (20, 60)) * (db[j] != 0))
    queries += _random_descs(rng, 45, revisit_every=10**9)  # fresh places
    for k in range(5):  # large empty sectors, the last one nearly blind
        d = rng.uniform(-2.0, 18.0, (20, 60)) * (rng.uniform(size=(20, 60)) < 0.5)
        d[:, 10:10 + 10 * (k + 1)] = 0.0
        queries.append(d)
    order = rng.permutation(70)
    queries = [queries[i] for i in order]
    keys, qkeys = _ring_keys(O, db), _ring_keys(O, queries)
    want = [_between_expected(O, db, keys, q, k) for q, k in zip(queries, qkeys)]
    # a tie between the 3rd and 4th nearest key (or inside the three) would let two correct searches disagree: none here
    for w in want:
        assert np.all(np.diff(w["sorted_keyd"][:4]) > 0)
    # The expected candidates are nanoflann's: the compiled reference library wherever oracle/_ref is built (that needs the reference's
    # sources; a checkout without them has only the restatement, which tests/test_oracle_cpu.py pins to nanoflann's stored answers)
    ref = O.ref_ringkey_knn(keys, qkeys, 3)
    if ref is not None:
        assert np.array_equal(ref[0], np.stack([w["cand"] for w in want]))
    assert sum(w["loop_id"] >= 0 for w in want) >= 15 and sum(w["loop_id"] < 0 for w in want) >= 40
    gm = S.SCManager(max_radius=80.0, dist_thres=0.2, max_keyframes=64)
    with pytest.raises(S.ScalError) as e:  # empty database
        gm.detect_between(queries[:1])
    assert e.value.code == S.E_STATE
    # databases of one and two entries: the unfilled KNN slots are index 0
    for n in (1, 2):
        gm.saveScancontextAndKeys(db[n - 1])
        for q, k in zip(queries[:6], qkeys[:6]):
            w = _between_expected(O, db[:n], keys[:n], q, k)
            assert w["n_real"] == n and np.all(w["cand"][n:] == 0)
            if ref is not None:  # nanoflann fills only the first n slots: the rest of the zero-initialised output stays 0
                assert np.array_equal(O.ref_ringkey_knn(keys[:n], k[None, :], 3)[0][0], w["cand"])
            _check_between(gm.detect_between([q])[0], w)
    for d in db[2:]:
        gm.saveScancontextAndKeys(d)
    got = gm.detect_between(queries)
    for g, w in zip(got, want):
        _check_between(g, w)
    # the records depend neither on nq nor on the chunking (one launch set per 64 queries)
    for nq in (1, 64, 65):
        part = gm.detect_between(queries[:nq])
        assert len(part) == nq and all(_same(a, b) for a, b in zip(part, got))
    # device-resident queries
    flat = np.stack([np.asarray(q).T.reshape(-1) for q in queries])
    t = torch.from_numpy(flat).cuda()
    torch.cuda.synchronize()
    dev = gm.detect_between_device(t.data_ptr(), 70)
    assert all(_same(a, b) for a, b in zip(dev, got))
    assert gm.size() == 48  # nothing was inserted
    sh = S.SCManager(max_keyframes=8, n_shards=2, shard=0)
    with pytest.raises(S.ScalError) as e:
        sh.detect_between(queries[:1])
    assert e.value.code == S.E_ARG
    sh.close(), gm.close()


# ------------------------------------------------------------------------------------------------- 2. cross-session blocks
def test_cross_session_matrix_and_topk(O, S):
    rng = np.random.default_rng(77)
    descs = _random_descs(rng, 58)
    descs[40] = np.roll(descs[3], 11, axis=1)  # a revisit across the two sessions
    descs[50][:, 5:50] = 0.0
    A, B, AB = S.SCManager(max_keyframes=64), S.SCManager(max_keyframes=32), S.SCManager(max_keyframes=64)
    for d in descs[:37]:
        A.saveScancontextAndKeys(d)
    for d in descs[37:]:
        B.saveScancontextAndKeys(d)
    for d in descs:
        AB.saveScancontextAndKeys(d)
    blocks = {}
    for mode in (0, 1, 2, 3):
        D, Sh = A.cross_matrix(B, 0, 21, 0, 37, mode)
        Dw, Sw = AB.distance_matrix(37, 58, 0, 37, mode)
        assert D.tobytes() == Dw.tobytes() and np.array_equal(Sh, Sw), mode
        Dr, Sr = A.cross_matrix(B, 3, 20, 5, 30, mode)  # ragged sub-ranges
        Dv, Sv = AB.distance_matrix(40, 57, 5, 30, mode)
        assert Dr.tobytes() == Dv.tobytes() and np.array_equal(Sr, Sv), mode
        D1, S1 = A.cross_matrix(B, 20, 21, 36, 37, mode)
        assert D1.tobytes() == Dw[20:21, 36:37].tobytes() and np.array_equal(S1, Sw[20:21, 36:37]), mode
        blocks[mode] = (D, Sh)
    for mode in (0, 1, 2):  # the revisit: B's entry 3 is A's entry 3 turned by 11 sectors
        assert blocks[mode][0][3, 3] <= 1e-12 and blocks[mode][1][3, 3] == 11
    for q, j in [(0, 0), (3, 3), (13, 36), (20, 1), (7, 7), (12, 30)]:
        full = O.sc_distance_full(descs[37 + q], descs[j])
        full = np.where(np.isnan(full), 1e300, full)
        assert abs(blocks[1][0][q, j] - full.min()) <= 1e-12 and blocks[1][1][q, j] == int(np.argmin(full))
    # the same context on both sides is the in-database block
    Ds, Ss = AB.cross_matrix(AB, 37, 58, 0, 37, 2)
    assert Ds.tobytes() == blocks[2][0].tobytes() and np.array_equal(Ss, blocks[2][1])
    D2, S2 = blocks[2]
    for k in (1, 3, 16):
        idx, dist, shift = A.cross_search(B, 0, 21, k, 2)
        assert idx.shape == (21, k)
        for r in range(21):
            o = np.argsort(D2[r], kind="stable")[:k]
            assert np.array_equal(idx[r], o) and dist[r].tobytes() == D2[r][o].tobytes() and np.array_equal(shift[r], S2[r][o]), (k, r)
    idx, dist, shift = A.cross_search(B, 4, 9, 3, 1)  # a sub-range of queries, vector-ALU mode
    for r in range(5):
        o = np.argsort(blocks[1][0][4 + r], kind="stable")[:3]
        assert np.array_equal(idx[r], o) and dist[r].tobytes() == blocks[1][0][4 + r][o].tobytes()
    tiny = S.SCManager(max_keyframes=4)  # fewer entries than k: the rest is empty
    tiny.saveScancontextAndKeys(descs[0]), tiny.saveScancontextAndKeys(descs[1])
    idx, dist, shift = tiny.cross_search(B, 0, 2, 3, 2)
    assert np.all(idx[:, 2] == -1) and np.all(dist[:, 2] == 10000000) and np.all(idx[:, :2] >= 0)
    sharded = S.SCManager(max_keyframes=8, n_shards=2, shard=0)
    sharded.saveScancontextAndKeys(descs[0])
    bad = [lambda: A.cross_matrix(sharded, 0, 1, 0, 1, 0), lambda: sharded.cross_matrix(B, 0, 1, 0, 1, 0), lambda: A.cross_matrix(B, 0, 22, 0, 37, 2),
           lambda: A.cross_matrix(B, 0, 21, 0, 38, 2), lambda: A.cross_matrix(B, 5, 4, 0, 37, 2), lambda: A.cross_matrix(B, -1, 4, 0, 37, 2),
           lambda: A.cross_matrix(B, 0, 4, 0, 37, 4), lambda: A.cross_search(B, 0, 22, 3, 2), lambda: A.cross_search(B, 0, 21, 17, 2),
           lambda: A.cross_search(B, 0, 21, 0, 2), lambda: A.cross_search(sharded, 0, 1, 1, 2)]
    for f in bad:
        with pytest.raises(S.ScalError) as e:
            f()
        assert e.value.code == S.E_ARG
    D, Sh = A.cross_matrix(B, 0, 21, 0, 37, 2)  # still working
    assert D.tobytes() == D2.tobytes()
    for m in (A, B, AB, tiny, sharded):
        m.close()


# ------------------------------------------------------------------------------------------------- shared clouds
@pytest.fixture(scope="module")
def clouds(S, golden):
    from scaloam import formats
    vg = S.VoxelGrid()
    raw = {("K", i): golden(f"KAIST03_{i:06d}.npy") for i in (0, 7, 20)}
    raw.update({("S", i): golden(f"Seosan01_{i:06d}.npy") for i in (0, 11)})
    pk = golden("KAIST03_poses21.npy").reshape(-1, 12).astype(np.float64)
    ps = golden("Seosan01_poses21.npy").reshape(-1, 12).astype(np.float64).copy()
    ps[:, 3] += 1000.0  # the second place, a kilometre away
    names = [("K", 0), ("K", 7), ("K", 20), ("S", 0), ("S", 11)]
    poses = [pk[0], pk[7], pk[20], ps[0], ps[11]]
    q5 = formats.read_pcd(os.path.join(GOLDEN, "KAIST03_000005.pcd"))
    stored = [vg.filter(raw[n], 0.4) for n in names]  # what a session keeps of each keyframe
    yield dict(vg=vg, raw=[raw[n] for n in names], poses=poses, stored=stored, q5=q5, p5=pk[5])
    vg.close()


def _session(S, clouds, n=5, **kw):
    args = dict(max_keyframes=8, max_points=100000, max_query_points=70000, submap_half=1)
    args.update(kw)
    rl = S.Relocalizer(**args)
    for j in range(n):
        assert rl.add_keyframe(clouds["raw"][j], clouds["poses"][j]) == j
    return rl


# ------------------------------------------------------------------------------------------------- 3. ICP with a guess
@pytest.fixture(scope="module")
def icp_case(S, clouds):
    """the turned keyframe 5 against keyframe 7, both at the 0.4 m leaf, and G = Rz(-90 deg) as the relocaliser builds it"""
    vg = clouds["vg"]
    src = vg.filter(_turn(clouds["q5"], 90.0), 0.4)
    tgt = clouds["stored"][1]
    G = S.yaw_guess(np.float32(np.float64(np.float32(15 * 6.0)) * np.pi / 180.0))
    icp = S.LoopICP(max_source=40000, max_target=40000)
    yield dict(src=src, tgt=tgt, G=G, icp=icp, pre=_apply34(G[:3], src))
    icp.close()


def test_icp_null_and_identity_guess_are_todays_path(S, icp_case):
    c = icp_case
    plain = c["icp"].align(c["src"], c["tgt"])
    ident = c["icp"].align(c["src"], c["tgt"], guess=np.eye(4))
    assert _icp_same(plain, ident)
    r = S.ICPResult()
    s, t = c["src"], c["tgt"]
    f32p = C.POINTER(C.c_float)
    assert S.lib().scal_icp_align_guess(c["icp"].h, s.ctypes.data_as(f32p), s.shape[0], t.ctypes.data_as(f32p), t.shape[0], None, C.byref(r)) == S.OK
    null = dict(converged=bool(r.converged), iterations=r.iterations, state=r.state, n_correspondences=r.n_correspondences, fitness=r.fitness,
                T=np.array(r.T[:]).reshape(4, 4))
    assert _icp_same(plain, null)
    assert plain["iterations"] > 1


def test_icp_guess_equals_a_premoved_source(O, S, icp_case):
    """Iterations, state and correspondences of align(src, tgt, G) are those of align(G src, tgt): the working cloud has the same bits in
    both.  T_guess and T_plain G are two f32 product chains (four half-ulp roundings per product): |T_guess - T_plain G| <= iterations *
    2^-22 * max(1, max|T|).  The fitness moves the ORIGINAL source by the composed T_guess, a cloud that differs from the plain run's
    by rounding, so the two fitness values are not the same number; the guessed one is held to what it is defined as - the mean squared
    nearest-neighbour distance of T_guess applied to the source - computed independently (numpy, 1e-9 relative) and bit for bit
    through the device's fitness sweep of the replayed cloud."""
    c = icp_case
    src, tgt, G, pre, icp = c["src"], c["tgt"], c["G"], c["pre"], c["icp"]
    # the device's pre-move is numpy's, bit for bit: after it every source point coincides with a point of the target `pre`
    exact = S.LoopICP(max_source=40000, max_target=40000, max_corr_dist=1e-30, max_iterations=1)
    assert exact.align(src, pre, guess=G)["n_correspondences"] == src.shape[0]
    assert exact.align(src, pre)["n_correspondences"] < src.shape[0] // 100
    exact.close()
    plain = icp.align(pre, tgt)
    guess = icp.align(src, tgt, guess=G)
    print("plain", plain["iterations"], plain["state"], plain["n_correspondences"], plain["fitness"])
    print("guess", guess["iterations"], guess["state"], guess["n_correspondences"], guess["fitness"])
    for k in ("converged", "iterations", "state", "n_correspondences"):
        assert plain[k] == guess[k], k
    want = plain["T"] @ G.astype(np.float64)
    E = plain["iterations"] * 2.0 ** -22 * max(1.0, np.abs(guess["T"]).max())
    print("T diff", np.abs(guess["T"] - want).max(), "bound", E)
    assert np.abs(guess["T"] - want).max() <= E
    # the fitness is that of the ORIGINAL source moved by T_guess: replayed here in k_icp_apply's order, then held to two references -
    # numpy's exact nearest neighbours (1e-9), and the device's own fitness sweep over the replayed cloud (bit for bit: a context whose
    # cap admits no correspondence stops at once with the identity, and its fitness is the uncapped sweep of its input)
    moved = _apply34(guess["T"][:3].astype(np.float32), src)
    want_fit = _nn_fitness(moved, tgt)
    print("fitness", guess["fitness"], "numpy", want_fit, "plain", plain["fitness"])
    assert abs(guess["fitness"] - want_fit) <= 1e-9 * want_fit
    sweep = S.LoopICP(max_source=40000, max_target=40000, max_corr_dist=1e-30, max_iterations=1)
    rs = sweep.align(moved, tgt)
    sweep.close()
    assert rs["state"] == 5 and rs["n_correspondences"] < 3 and np.array_equal(rs["T"], np.eye(4))
    assert np.float64(rs["fitness"]).tobytes() == np.float64(guess["fitness"]).tobytes()
    ro = O.icp_align(pre, tgt)
    assert ro["iterations"] == plain["iterations"] == guess["iterations"] and ro["state"] == plain["state"]
    assert abs(plain["fitness"] - ro["fitness"]) <= 1e-9 * ro["fitness"]
    assert np.abs(plain["T"] - ro["T"]).max() <= 1e-9


def test_icp_guess_premise(S, clouds, golden):
    """The 90 degree query against the three-keyframe submap around keyframe 7.  The oracle from the identity (the record of
    tools/make_reloc_fixture.py, held to a live run by tests/test_reloc_cpu.py): fitness 22.6, 26.5 m off.  The device from the guess:
    fitness 0.271, 0.021 m / 0.10 degrees off the golden relative pose."""
    vg, poses, stored = clouds["vg"], clouds["poses"], clouds["stored"]
    src = vg.filter(_turn(clouds["q5"], 90.0), 0.4)
    tgt = vg.filter(np.concatenate([stored[j] if j == 1 else _apply34(S.relative_transform(poses[1], poses[j]), stored[j]) for j in (0, 1, 2)]), 0.4)
    want = np.linalg.inv(_P4(poses[1])) @ _P4(clouds["p5"]) @ np.linalg.inv(_turn4(90.0))
    rec = golden("reloc_premise_oracle.npz")
    assert int(rec["n_src"]) == src.shape[0] and int(rec["n_tgt"]) == tgt.shape[0] == 32853
    assert float(rec["fitness"]) > 1.0 and np.linalg.norm(rec["T"][:3, 3] - want[:3, 3]) > 10.0
    icp = S.LoopICP(max_source=40000, max_target=40000)
    G = S.yaw_guess(np.float32(np.float64(np.float32(15 * 6.0)) * np.pi / 180.0))
    r = icp.align(src, tgt, guess=G)
    dt, da = _pose_error(r["T"], want)
    print("guess:", r["fitness"], r["iterations"], dt, da)
    assert r["converged"] and r["fitness"] <= 0.3 and dt <= 0.1 and da <= 0.5
    icp.close()


def test_icp_bad_guess_is_refused_and_the_context_survives(S, icp_case):
    c = icp_case
    before = c["icp"].align(c["src"], c["tgt"], guess=c["G"])
    for bad in ((0, 3, np.nan), (2, 2, np.inf), (3, 3, 0.0), (3, 1, 0.5)):
        g = c["G"].copy()
        g[bad[0], bad[1]] = bad[2]
        with pytest.raises(S.ScalError) as e:
            c["icp"].align(c["src"], c["tgt"], guess=g)
        assert e.value.code == S.E_ARG
    assert _icp_same(before, c["icp"].align(c["src"], c["tgt"], guess=c["G"]))


# ------------------------------------------------------------------------------------------------- 4. end to end
@pytest.fixture(scope="module")
def session(S, clouds):
    rl = _session(S, clouds)
    yield rl
    rl.close()


@pytest.fixture(scope="module")
def queries(clouds):
    return [_turn(clouds["q5"], yaw, TY) for yaw in YAWS]


@pytest.fixture(scope="module")
def singles(session, queries):
    return [session.query(q) for q in queries]


def test_reloc_finds_the_turned_keyframe(clouds, singles):
    for yaw, r in zip(YAWS, singles):
        want = _P4(clouds["p5"]) @ np.linalg.inv(_turn4(yaw, TY))
        dt, da = _pose_error(_P4(r["pose12"]), want)
        print(yaw, r["status"], r["sc"]["nn_idx"], r["sc"]["min_dist"], r["sc"]["nn_shift"], r["icp"]["fitness"], r["icp"]["iterations"], dt, da)
        assert r["status"] == 1 and r["sc"]["nn_idx"] == 1 and r["sc"]["loop_id"] == 1
        assert dt <= 0.1 and da <= 0.5


def test_reloc_stages_equal_the_chain_rebuilt_outside(O, S, clouds, session, queries, singles):
    vg, poses, stored = clouds["vg"], clouds["poses"], clouds["stored"]
    db = session.sc()
    assert db.size() == 5 and session.size() == 5
    gm = S.SCManager()
    for j in range(5):  # the stored descriptors are those of the filtered clouds
        o, _ = O.voxel_grid(clouds["raw"][j], 0.4)
        assert np.array_equal(_bits(stored[j]), _bits(o))
        assert db.get(j)[0].tobytes() == gm.makeScancontext(stored[j]).tobytes()
    icp = S.LoopICP(max_source=70000, max_target=70000)
    for q, r in zip(queries, singles):
        src = vg.filter(q, 0.4)
        o, _ = O.voxel_grid(q, 0.4)
        assert np.array_equal(_bits(src), _bits(o)) and r["n_src"] == src.shape[0]
        found = db.detect_between([gm.makeScancontext(src)])[0]  # the query's descriptor, built outside, gives the same search record
        assert _same(found, r["sc"])
        c = r["sc"]["loop_id"]
        parts = [stored[j] if j == c else _apply34(S.relative_transform(poses[c], poses[j]), stored[j]) for j in (c - 1, c, c + 1)]
        tgt = vg.filter(np.concatenate(parts), 0.4)
        assert r["n_tgt"] == tgt.shape[0]
        ref = icp.align(src, tgt, guess=S.yaw_guess(r["sc"]["yaw"]))
        assert _icp_same(ref, r["icp"])  # fitness and T depend on every bit of both clouds
        assert np.abs(_P4(r["pose12"]) - _P4(poses[c]) @ r["icp"]["T"]).max() <= 1e-9
    icp.close(), gm.close()


def test_reloc_without_the_yaw_guess(S, clouds, queries, singles):
    rl = _session(S, clouds, no_yaw_guess=True)
    res = [rl.query(q) for q in queries[:4]]
    for yaw, r, s in zip(YAWS, res, singles):
        print(yaw, r["status"], r["icp"]["fitness"], r["icp"]["iterations"])
        assert _same(r["sc"], s["sc"]) and r["n_src"] == s["n_src"] and r["n_tgt"] == s["n_tgt"]
    assert res[0]["status"] == 1 and _same(res[0], singles[0])  # shift 0: the guess is the identity anyway
    for r in res[1:]:
        assert r["status"] == 2 and (not r["icp"]["converged"] or r["icp"]["fitness"] > 0.3)
    rl.close()


def test_reloc_other_place_and_candidate_alone(S, clouds, queries):
    rl = _session(S, clouds, n=3, submap_half=-1)  # KAIST03 only, the candidate keyframe's cloud as the whole target
    r = rl.query(clouds["raw"][4])  # a Seosan01 keyframe
    print("other place:", r["sc"]["min_dist"])
    assert r["status"] == 0 and r["sc"]["loop_id"] == -1 and r["sc"]["min_dist"] >= 0.2 and r["n_tgt"] == 0
    assert r["n_src"] == clouds["stored"][4].shape[0]
    assert not r["icp"]["converged"] and r["icp"]["iterations"] == 0 and r["icp"]["state"] == 0 and r["icp"]["fitness"] == 0.0
    assert not r["icp"]["T"].any() and not r["pose12"].any()
    r = rl.query(queries[1])
    vg = clouds["vg"]
    tgt = vg.filter(clouds["stored"][1], 0.4)
    icp = S.LoopICP(max_source=70000, max_target=70000)
    ref = icp.align(vg.filter(queries[1], 0.4), tgt, guess=S.yaw_guess(r["sc"]["yaw"]))
    assert r["sc"]["loop_id"] == 1 and r["n_tgt"] == tgt.shape[0] and _icp_same(ref, r["icp"])
    icp.close(), rl.close()


@pytest.mark.parametrize("empty_at", (0, 2), ids=("first_of_the_window", "behind_the_candidate"))
def test_reloc_submap_entries_that_share_a_dst(S, clouds, queries, empty_at):
    """A stored keyframe without points gives the submap's gather table an entry that shares its dst with the next one (or with the
    sentinel): gather_find has to take the LAST entry with dst <= i.  Keyframes 0 / 7 / 20 with one of the candidate's neighbours empty,
    submap_half = 1, the 90 degree query: n_tgt and the whole ICP record against the chain rebuilt outside from the non-empty parts."""
    vg, poses, stored = clouds["vg"], clouds["poses"], clouds["stored"]
    gm = S.SCManager()
    far = gm.makeScancontext(stored[3])  # the empty keyframe is stored with another place's descriptor: the search is left alone
    rl = S.Relocalizer(max_keyframes=4, max_points=100000, max_query_points=70000, submap_half=1)
    for j in range(3):
        if j == empty_at:
            assert rl.add_keyframe(np.zeros((0, 4), np.float32), poses[j], desc=far) == j
        else:
            assert rl.add_keyframe(clouds["raw"][j], poses[j]) == j
    r = rl.query(queries[1])
    assert r["sc"]["loop_id"] == 1 and r["sc"]["nn_idx"] == 1
    parts = [stored[j] if j == 1 else _apply34(S.relative_transform(poses[1], poses[j]), stored[j]) for j in range(3) if j != empty_at]
    src, tgt = vg.filter(queries[1], 0.4), vg.filter(np.concatenate(parts), 0.4)
    icp = S.LoopICP(max_source=70000, max_target=70000)
    ref = icp.align(src, tgt, guess=S.yaw_guess(r["sc"]["yaw"]))
    print(empty_at, r["status"], r["n_tgt"], tgt.shape[0], r["icp"]["fitness"], ref["fitness"], r["icp"]["iterations"], ref["iterations"])
    assert r["n_src"] == src.shape[0] and r["n_tgt"] == tgt.shape[0]
    assert _icp_same(ref, r["icp"])  # fitness and T depend on every bit of both clouds
    icp.close(), gm.close(), rl.close()


def test_reloc_batch_equals_single_calls_and_repeats(clouds, session, queries, singles):
    extra = [clouds["raw"][4], np.zeros((0, 4), np.float32), clouds["raw"][0][:5000]]
    every = list(queries) + extra
    one = list(singles) + [session.query(q) for q in extra]
    assert one[5]["status"] == 1 and one[5]["sc"]["loop_id"] == 4  # the Seosan01 keyframe finds itself (submap: keyframes 3 and 4)
    assert one[6]["status"] == 0 and one[6]["n_src"] == 0          # an empty cloud finds nothing
    batch = session.query_batch(every)
    assert len(batch) == len(every)
    for k, (a, b) in enumerate(zip(batch, one)):
        assert _same(a, b), k
    again = [session.query(q) for q in queries]  # two runs, bit for bit
    assert all(_same(a, b) for a, b in zip(again, singles))
    assert all(_same(a, b) for a, b in zip(session.query_batch(every), batch))
    assert session.query_batch([]) == []


def test_reloc_supplied_descriptor_is_used_as_given(S, clouds):
    from scaloam import formats
    gm = S.SCManager()
    d = formats.read_scd(formats.scd_text(gm.makeScancontext(clouds["stored"][1])))  # a descriptor as SCDs/NNNNNN.scd holds it: 3 digits
    assert d.shape == (20, 60) and not np.array_equal(d, gm.makeScancontext(clouds["stored"][1]))
    rl = S.Relocalizer(max_keyframes=4, max_points=40000, max_query_points=70000)
    assert rl.add_keyframe(clouds["raw"][0], clouds["poses"][0]) == 0
    assert rl.add_keyframe(clouds["raw"][1], clouds["poses"][1], desc=d) == 1
    db = rl.sc()
    assert db.get(1)[0].tobytes() == d.tobytes()
    assert db.get(0)[0].tobytes() == gm.makeScancontext(clouds["stored"][0]).tobytes()
    gm.close(), rl.close()


def test_reloc_capacity_errors_leave_the_context_usable(S, clouds, queries):
    raw, poses, stored = clouds["raw"], clouds["poses"], clouds["stored"]

    def refused(f, code):
        with pytest.raises(S.ScalError) as e:
            f()
        assert e.value.code == code, e.value

    # the arena: keyframe 7 does not fit behind keyframe 0
    rl = S.Relocalizer(max_keyframes=4, max_points=stored[0].shape[0] + 100, max_query_points=70000)
    refused(lambda: rl.query(raw[0]), S.E_STATE)  # nothing stored yet
    assert rl.add_keyframe(raw[0], poses[0]) == 0
    refused(lambda: rl.add_keyframe(raw[1], poses[1]), S.E_CAPACITY)
    assert rl.size() == 1 and rl.sc().size() == 1  # nothing was stored
    bad = np.array(poses[1]).copy()
    bad[7] = np.nan
    refused(lambda: rl.add_keyframe(raw[1][:100], bad), S.E_ARG)
    assert rl.add_keyframe(raw[1][:50], poses[1]) == 1  # a small one still fits
    r = rl.query(raw[0])
    assert r["status"] == 1 and r["sc"]["loop_id"] == 0 and r["sc"]["min_dist"] <= 1e-12
    rl.close()
    # the database
    rl = S.Relocalizer(max_keyframes=1, max_points=100000, max_query_points=70000)
    assert rl.add_keyframe(raw[0], poses[0]) == 0
    refused(lambda: rl.add_keyframe(raw[1], poses[1]), S.E_CAPACITY)
    assert rl.size() == 1 and rl.sc().size() == 1
    assert rl.query(raw[0])["status"] == 1
    rl.close()
    # the query size, and the submap that does not fit the work buffers
    rl = S.Relocalizer(max_keyframes=4, max_points=100000, max_query_points=40000, submap_half=1)
    for j in range(3):
        assert rl.add_keyframe(raw[j], poses[j]) == j
    assert raw[3].shape[0] > 40000
    refused(lambda: rl.query(raw[3]), S.E_TOO_MANY)
    refused(lambda: rl.add_keyframe(raw[3], poses[3]), S.E_TOO_MANY)
    refused(lambda: rl.query_batch([raw[0], raw[3]]), S.E_TOO_MANY)
    assert sum(s.shape[0] for s in stored[:3]) > 40000
    refused(lambda: rl.query(queries[0]), S.E_CAPACITY)  # candidate 1: keyframes 0, 1 and 2
    refused(lambda: rl.query_batch([raw[0], queries[0]]), S.E_CAPACITY)
    r = rl.query(raw[0])  # candidate 0: keyframes 0 and 1 fit
    assert r["status"] == 1 and r["sc"]["loop_id"] == 0 and r["n_tgt"] > stored[0].shape[0]
    assert rl.size() == 3
    rl.close()
