"""scaloam.icp_point, the CPU restatement of scal_icp_align* (point-to-point ICP; csrc/icp.hip, icp_dev.hpp, icp_host.hpp), on its
own: the layout of the 17 sums against a plain loop, Horn's closed form against the oracle's bit for bit, whole alignments against
the oracle's pcl::IterativeClosestPoint restatement (O.icp_align) in every convergence state, the guess.
tests/test_icp_point_gpu.py holds the device to this module bit for bit and takes its scenes from here."""
import ctypes as C

import numpy as np
import pytest

DBL_MAX = float(np.finfo(np.float64).max)
FIELDS = ("T", "iterations", "state", "converged", "n_correspondences", "fitness")


@pytest.fixture(scope="module")
def P():
    from scaloam import icp_point
    return icp_point


def cloud(xyz):
    a = np.zeros((len(xyz), 4), np.float32)
    a[:, :3] = xyz
    return a


def rot(axis, th):
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def rigid(axis, th, t):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = rot(axis, th), t
    return M


def same_result(a, b):
    """the six fields of two align results, bit for bit"""
    for k in FIELDS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (k, a[k], b[k])
    return True


def f32_d2(src, tgt):
    """[n_src, n_tgt] f32 squared distances in the dense sweep's arithmetic"""
    d = None
    for k in range(3):
        e = src[:, None, k] - tgt[None, :, k]
        d = e * e if d is None else d + e * e
    assert d.dtype == np.float32
    return d


def tie_free(src, tgt):
    """for every query the smallest f32 squared distance is taken by one target point only"""
    d = f32_d2(src, tgt)
    return bool(((d == d.min(1)[:, None]).sum(1) == 1).all())


def blob_scene():
    """(target, the target turned by 0.05 rad, the same with 0.05 m of noise): 400 points, sigma 4 m"""
    rng = np.random.default_rng(3)
    xyz = rng.standard_normal((400, 3)) * 4.0
    R = rot([0.3, -0.5, 1.0], 0.05)
    return cloud(xyz), cloud(xyz @ R.T), cloud(xyz @ R.T + rng.standard_normal((400, 3)) * 0.05)


def turned_blob(noise):
    """(source, target) of blob_scene"""
    tgt, turned, noisy = blob_scene()
    return (noisy if noise else turned), tgt


def few_scene(n_near, collinear=False):
    """(source of 150 + n_near points, target of 300): n_near source points lie 0.2 m from a target point of their own, the other 150
    more than 50 m from every target point, so a cap of 1 m leaves exactly n_near correspondences"""
    rng = np.random.default_rng(17)
    t = rng.uniform(-6.0, 6.0, (300, 3))
    if collinear:
        t[:3] = np.array([[1.0, 2.0, -1.0]]) + np.array([[-2.0], [0.5], [3.0]]) * np.array([[0.6, 0.0, 0.8]])
    far = rng.uniform(-6.0, 6.0, (150, 3)) + np.array([80.0, 0.0, 0.0])
    near = t[:n_near] + np.array([0.0, 0.2, 0.0])
    order = rng.permutation(150 + n_near)
    return cloud(np.concatenate([near, far])[order]), cloud(t)


def dyadic_scene():
    """coordinates that are multiples of 1/16 below 64 in magnitude: every term of the 17 sums and every partial sum is exact"""
    rng = np.random.default_rng(23)
    t = rng.integers(-1000, 1001, (700, 3)) / 16.0
    s = t[:500] + rng.integers(-6, 7, (500, 3)) / 16.0
    return cloud(s), cloud(t)


# name -> (scene, settings, the state and the iteration count the oracle reports)
STATE_CASES = {
    "transformation_epsilon": (lambda: turned_blob(noise=False), {}, 2, 3),
    "relative_mse": (lambda: turned_blob(noise=True), dict(transformation_epsilon=0.0, fitness_epsilon=1e-2), 4, 3),
    "absolute_mse": (lambda: turned_blob(noise=True), dict(transformation_epsilon=0.0, fitness_epsilon=0.0), 3, 12),
    "iteration_cap": (lambda: turned_blob(noise=True), dict(max_iterations=2), 1, 2),
}


def oracle_align(O, src, tgt, **kw):
    return O.icp_align(src, tgt, max_corr=kw.get("max_corr_dist", 150.0), max_iter=kw.get("max_iterations", 100),
                       trans_eps=kw.get("transformation_epsilon", 1e-6), fit_eps=kw.get("fitness_epsilon", 1e-6))


def agrees_with_oracle(r, ro):
    assert (r["state"], r["iterations"], r["converged"]) == (ro["state"], ro["iterations"], ro["converged"]), (r, ro)
    assert np.abs(r["T"] - ro["T"]).max() <= 1e-9, (r["T"], ro["T"])
    assert abs(r["fitness"] - ro["fitness"]) <= 1e-9 * abs(ro["fitness"]), (r["fitness"], ro["fitness"])
    return True


def test_sums_layout_against_a_plain_loop(P):
    """Small integers as coordinates: every term and every partial sum is an integer below 2^53, so any summation order gives the
    same bits and a plain loop pins what each of the 17 entries holds."""
    rng = np.random.default_rng(11)
    g = np.arange(9)
    tgt = cloud(np.stack([m.reshape(-1) for m in np.meshgrid(g, g - 4, 2 * g, indexing="ij")], 1))
    tgt = tgt[rng.permutation(tgt.shape[0])]
    src = tgt[rng.permutation(tgt.shape[0])[:300]].copy()
    src[:, :3] += rng.integers(-2, 3, (300, 3)).astype(np.float32)
    src[17, 0] = np.nan                                 # source points that take no part
    src[18, 2] = np.inf
    src[40, :3] += 50                                   # one beyond the cap
    src[41, :3] = (11, 0, 4)                            # one exactly on it, 3 from the lattice's face: kept
    tgt[7, 1] = np.nan                                  # a target point that is nobody's neighbour
    max2 = 9.0
    want = np.zeros(17)
    n_edge = 0
    T64 = tgt[:, :3].astype(np.float64)
    ok = np.isfinite(T64).all(1)
    for p in src[:, :3].astype(np.float64):
        if not np.isfinite(p).all():
            continue
        d2 = np.where(ok, ((p[None, :] - np.where(ok[:, None], T64, 0.0)) ** 2).sum(1), np.inf)
        j = int(np.argmin(d2))                          # the first of equal distances: the lowest index
        if d2[j] > max2:
            continue
        n_edge += d2[j] == max2
        q = T64[j]
        want[0] += 1.0
        want[1:4] += p
        want[4:7] += q
        want[7:16] += np.outer(q, p).reshape(9)
        want[16] += d2[j]
    got = P.sweep_sums(src, tgt, np.float32(max2))
    assert got.shape == (17,) and got.dtype == np.float64
    assert 250 < want[0] <= 297.0 and n_edge >= 1
    assert np.array_equal(got, want)
    # the strict comparison would lose the points on the cap
    assert P.sweep_sums(src, tgt, np.nextafter(np.float32(max2), np.float32(0)))[0] == want[0] - n_edge


def sums_of(p, q):
    s = np.zeros(17)
    s[0] = p.shape[0]
    s[1:4], s[4:7] = p.sum(0), q.sum(0)
    s[7:16] = (q[:, :, None] * p[:, None, :]).sum(0).reshape(9)
    return s


def oracle_transform(O, sums):
    L = O.lib()
    f64p = C.POINTER(C.c_double)
    L.orc_icp_transform_from_sums.argtypes = [f64p, f64p]
    L.orc_icp_transform_from_sums.restype = None
    s, T = np.ascontiguousarray(sums[:16], np.float64), np.zeros(16)
    L.orc_icp_transform_from_sums(s.ctypes.data_as(f64p), T.ctypes.data_as(f64p))
    return T.reshape(4, 4)


def test_transform_from_sums_equals_the_oracle(P, O):
    rng = np.random.default_rng(29)
    kinds = {"random": 0, "planar": 0, "collinear": 0}
    for trial in range(330):
        kind = "collinear" if trial % 11 == 10 else "planar" if trial % 5 == 4 else "random"
        n = int(rng.integers(3, 400))
        p = rng.uniform(-5.0, 5.0, (n, 3))
        if kind == "planar":
            p[:, 2] = 0.0
            p = p @ rot(rng.standard_normal(3), rng.uniform(0, 3.0)).T
        if kind == "collinear":
            p = rng.uniform(-5.0, 5.0, (n, 1)) * rng.standard_normal((1, 3)) + rng.uniform(-2.0, 2.0, (1, 3))
        q = p @ rot(rng.standard_normal(3), rng.uniform(0, 0.5)).T + rng.uniform(-1.0, 1.0, 3)
        if trial % 3:
            q = q + rng.standard_normal((n, 3)) * 0.02 * (1.0 if kind == "random" else np.array([1.0, 1.0, 0.0]) if kind == "planar" else 0.0)
        s = sums_of(p, q)
        T, To = P.transform_from_sums(s), oracle_transform(O, s)
        assert T.dtype == np.float32 and T.shape == (4, 4)
        if kind == "collinear":                          # the rotation about the line is free: any answer, but a finite one
            assert np.isfinite(T).all() and np.isfinite(To).all()
        else:
            assert np.array_equal(T.astype(np.float64), To), (trial, kind, T, To)
        # both move the centroid onto the centroid
        mp, mq = s[1:4] / s[0], s[4:7] / s[0]
        for M in (T.astype(np.float64), To):
            assert np.abs(M[:3, :3] @ mp + M[:3, 3] - mq).max() <= 1e-5, (trial, kind)
            assert np.array_equal(M[3], [0, 0, 0, 1])
        kinds[kind] += 1
    assert kinds == {"random": 240, "planar": 60, "collinear": 30}


@pytest.mark.parametrize("name", list(STATE_CASES))
def test_align_reaches_every_state_as_the_oracle_does(P, O, name):
    scene, kw, state, iterations = STATE_CASES[name]
    src, tgt = scene()
    assert 150 <= src.shape[0] <= 700 and 150 <= tgt.shape[0] <= 700 and tie_free(src, tgt)
    ro = oracle_align(O, src, tgt, **kw)
    print(name, "oracle: state", ro["state"], "iterations", ro["iterations"], "fitness", ro["fitness"])
    assert (ro["state"], ro["iterations"], ro["converged"]) == (state, iterations, True)
    r = P.align(src, tgt, **kw)
    assert agrees_with_oracle(r, ro) and r["n_correspondences"] == src.shape[0]


def test_align_with_too_few_correspondences(P, O):
    src, tgt = few_scene(2)
    assert tie_free(src, tgt) and (f32_d2(src, tgt).min(1) <= 1.0).sum() == 2
    ro = oracle_align(O, src, tgt, max_corr_dist=1.0)
    assert (ro["state"], ro["iterations"], ro["converged"]) == (5, 0, False)
    r = P.align(src, tgt, max_corr_dist=1.0)
    assert agrees_with_oracle(r, ro)
    assert r["n_correspondences"] == 2 and np.array_equal(r["T"], np.eye(4)) and 1000.0 < r["fitness"] < DBL_MAX
    # one more and the alignment runs
    src, tgt = few_scene(3)
    ro = oracle_align(O, src, tgt, max_corr_dist=1.0)
    assert ro["state"] != 5 and ro["iterations"] >= 1
    assert agrees_with_oracle(P.align(src, tgt, max_corr_dist=1.0), ro)


def test_align_on_three_collinear_correspondences(P, O):
    src, tgt = few_scene(3, collinear=True)
    assert tie_free(src, tgt) and (f32_d2(src, tgt).min(1) <= 1.0).sum() == 3
    t3 = tgt[:3, :3].astype(np.float64)
    assert np.linalg.matrix_rank(t3 - t3.mean(0), tol=1e-5) == 1
    ro = oracle_align(O, src, tgt, max_corr_dist=1.0)
    print("collinear, oracle: state", ro["state"], "iterations", ro["iterations"])
    r = P.align(src, tgt, max_corr_dist=1.0)
    assert np.isfinite(ro["T"]).all() and ro["iterations"] >= 1 and ro["converged"]
    assert agrees_with_oracle(r, ro) and r["n_correspondences"] >= 3


def test_align_on_dyadic_coordinates_equals_the_oracle(P, O):
    src, tgt = dyadic_scene()
    assert tie_free(src, tgt)
    assert np.array_equal(src[:, :3] * 16, np.round(src[:, :3] * 16)) and np.abs(np.concatenate([src, tgt])[:, :3]).max() < 64
    ro = oracle_align(O, src, tgt, max_iterations=1)
    r = P.align(src, tgt, max_iterations=1)
    assert (ro["state"], ro["iterations"]) == (1, 1) and agrees_with_oracle(r, ro)
    assert np.array_equal(r["T"], ro["T"])            # the sums are exact in any order, the closed form is the same operations


def f32_product(T, G):
    """T * G as icp_host_accumulate multiplies: f32, ((t0 g0 + t1 g1) + t2 g2) + t3 g3"""
    T, G = np.asarray(T, np.float32), np.asarray(G, np.float32)
    return np.stack([((T[r, 0] * G[0] + T[r, 1] * G[1]) + T[r, 2] * G[2]) + T[r, 3] * G[3] for r in range(4)])


def test_guess(P):
    from scaloam import icp_plane
    tgt, _, noisy = blob_scene()
    G = rigid([0.2, 1.0, -0.4], 0.1, [0.3, -0.1, 0.05]).astype(np.float32)
    moved = icp_plane.transform(G, noisy)
    # one iteration: F = T1 * G, with T1 the increment of the moved cloud's own alignment
    a, b = P.align(noisy, tgt, guess=G, max_iterations=1), P.align(moved, tgt, max_iterations=1)
    assert np.array_equal(a["T"], f32_product(b["T"], G).astype(np.float64)) and not np.array_equal(a["T"], b["T"])
    assert (a["state"], a["iterations"], a["n_correspondences"]) == (b["state"], b["iterations"], b["n_correspondences"]) == (1, 1, 400)
    # the whole alignment walks the moved cloud's increments T1, T2, ..: F = Tn * (.. * (T1 * G)), every product in f32.  (F' * G with
    # F' the moved cloud's own result is another order of the same products and differs in the last bits.)
    a, b = P.align(noisy, tgt, guess=G), P.align(moved, tgt)
    assert (a["state"], a["iterations"], a["n_correspondences"]) == (b["state"], b["iterations"], b["n_correspondences"])
    assert a["iterations"] >= 2
    F, Fb, cur = G, np.eye(4, dtype=np.float32), moved
    for _ in range(a["iterations"]):
        Tk = P.align(cur, tgt, max_iterations=1)["T"].astype(np.float32)      # one iteration from the identity: F = Tk
        F, Fb, cur = f32_product(Tk, F), f32_product(Tk, Fb), icp_plane.transform(Tk, cur)
    assert np.array_equal(a["T"], F.astype(np.float64)) and np.array_equal(b["T"], Fb.astype(np.float64))
    assert np.abs(a["T"] - f32_product(b["T"], G)).max() <= (a["iterations"] + 1) * 8 * 2.0 ** -24
    # no guess, None and the identity are one call
    none = P.align(noisy, tgt)
    assert same_result(none, P.align(noisy, tgt, None)) and same_result(none, P.align(noisy, tgt, np.eye(4)))
    assert not np.array_equal(none["T"], a["T"])
    bad, nan = np.eye(4), np.eye(4)
    bad[3, 3] = 2.0
    nan[0, 3] = np.nan
    for guess in (bad, nan, np.eye(3)):
        with pytest.raises(ValueError):
            icp_plane._check_guess(guess)
        with pytest.raises(ValueError):
            P.align(noisy, tgt, guess)


def test_empty_clouds(P):
    tgt, src, _ = blob_scene()
    empty = np.zeros((0, 4), np.float32)
    for s, t in ((empty, tgt), (src, empty), (empty, empty)):
        r = P.align(s, t)
        assert r["state"] == 5 and not r["converged"] and r["iterations"] == 0 and r["n_correspondences"] == 0
        assert np.array_equal(r["T"], np.eye(4)) and r["fitness"] == DBL_MAX
    # a source of NaN only: no query has a key, the fitness stays DBL_MAX
    r = P.align(np.full((5, 4), np.nan, np.float32), tgt)
    assert r["state"] == 5 and r["n_correspondences"] == 0 and r["fitness"] == DBL_MAX
