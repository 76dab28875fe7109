"""scal_nbr_knn* and the k-NN half of scaloam/nbr.py without a GPU: the restatement's two candidate paths against each other on the
inputs tests/test_knn_gpu.py compares the device with, the order (d2, input position) on a hand-made tie case, the escalation to
unbounded k-NN against brute force, the statistical outlier rule on a hand-made cloud, the argument checks that precede the device."""
import ctypes as C
import functools
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _scene_tool():
    spec = importlib.util.spec_from_file_location("mapdiff_scene", os.path.join(ROOT, "tools", "mapdiff_scene.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@functools.lru_cache(maxsize=None)
def _inputs(r):
    return _scene_tool().radius_inputs(r)


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _same(got, want):
    return (got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[0].shape == want[0].shape == got[1].shape == want[1].shape
            and np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1])))


def tie_case():
    """index: the origin, six records at exactly 0.5 along the axes in shuffled order, an exact duplicate of one of them; the query
    is the origin.  Returns (I, q, the expected order of positions)"""
    I = np.array([[0, 0.5, 0, 1], [0, 0, -0.5, 2], [0.5, 0, 0, 3], [0, 0, 0, 4], [-0.5, 0, 0, 5], [0, 0, 0.5, 6], [0, -0.5, 0, 7],
                  [0, 0, -0.5, 8]], np.float32)
    return I, np.zeros((1, 4), np.float32), [3, 0, 1, 2, 4, 5, 6, 7]


@pytest.mark.parametrize("r", [0.5, 1.0])
@pytest.mark.parametrize("k", [1, 5, 20, 64])
def test_brute_force_equals_the_tree_path(S, r, k):
    from scaloam import nbr
    I, Q = _inputs(r)
    assert I.shape[0] == 3661 and Q.shape[0] == 2615
    b = nbr.knn_within(I, Q, k, r, path="brute")
    t = nbr.knn_within(I, Q, k, r, path="tree")
    assert b[0].shape == (Q.shape[0], k) and _same(b, t)
    full = b[0][:, -1] >= 0
    assert full.any() and (~full).any()                      # both classes of query: full rows and short ones
    assert np.array_equal(b[0] < 0, np.isposinf(b[1])) and not np.isnan(b[1]).any()
    assert (np.diff((b[0] >= 0).astype(int), axis=1) <= 0).all()           # padding only behind the entries
    # rows ascend in (d2, position), every entry is a candidate, and the lengths are the radius counts
    key = (_bits(b[1]).astype(np.uint64) << np.uint64(32)) | b[0].astype(np.uint32)
    assert (np.diff(key.astype(object), axis=1)[b[0][:, 1:] >= 0] > 0).all() if k > 1 else True
    r2 = np.float32(np.float32(r) * np.float32(r))
    assert (b[1][b[0] >= 0] <= r2).all()
    count, min_d2 = nbr.radius_counts(I, Q, r)
    assert np.array_equal((b[0] >= 0).sum(1), np.minimum(count, k)) and np.array_equal(_bits(b[1][:, 0]), _bits(min_d2))
    bad = ~np.isfinite(Q[:, :3]).all(1)
    assert bad.sum() == 9 and (b[0][bad] == -1).all()
    # d2 is the header's formula of the pair named by idx
    qi, s = np.nonzero(b[0] >= 0)
    assert np.array_equal(_bits(nbr._d2(Q[qi, :3], I[b[0][qi, s], :3])), _bits(b[1][qi, s]))


def test_ties_follow_the_input_position(S):
    from scaloam import nbr
    I, q, order = tie_case()
    for path in ("brute", "tree"):
        for k in range(1, 11):
            idx, d2 = nbr.knn_within(I, q, k, 0.5, path=path)
            want = (order + [-1] * k)[:k]
            assert list(idx[0]) == want, (path, k)
            assert list(d2[0]) == [0.0 if p == 3 else 0.25 if p >= 0 else np.inf for p in want]
    # a reversed index reverses the positions of the six, the duplicates included: position decides, not arrival
    idx, _ = nbr.knn_within(I[::-1], q, 8, 0.5)
    assert list(idx[0]) == [4, 0, 1, 2, 3, 5, 6, 7]
    # just under the radius the six are no candidates
    idx, d2 = nbr.knn_within(I, q, 3, 0.49999997)
    assert list(idx[0]) == [3, -1, -1] and list(d2[0]) == [0.0, np.inf, np.inf]


def _unbounded(I, Q, k):
    """brute-force k-NN of every finite query over all finite index records, order (d2, position)"""
    from scaloam import nbr
    fi, fq = np.isfinite(I[:, :3]).all(1), np.isfinite(Q[:, :3]).all(1)
    pos = np.flatnonzero(fi)
    idx, d2 = np.full((Q.shape[0], k), -1, np.int32), np.full((Q.shape[0], k), np.inf, np.float32)
    for a in range(0, Q.shape[0], 512):
        d = nbr._d2(Q[a:a + 512, None, :3], I[None, fi, :3])
        with np.errstate(invalid="ignore"):
            order = np.lexsort((np.broadcast_to(pos, d.shape), d), axis=1)[:, :k]
        idx[a:a + 512, :order.shape[1]] = pos[order]
        d2[a:a + 512, :order.shape[1]] = np.take_along_axis(d, order, 1)
    idx[~fq], d2[~fq] = -1, np.inf
    return idx, d2


def test_escalation_is_exact_unbounded_knn(S):
    from scaloam import nbr
    I, Q = _inputs(0.5)
    k = 20
    want = _unbounded(I, Q, k)
    idx, d2, levels = nbr.knn(I, Q, k, 0.25)
    assert levels > 1 and _same((idx, d2), want)
    idx, d2, levels = nbr.knn(I, Q, 1, 0.25)
    assert levels > 1 and _same((idx, d2), (want[0][:, :1], want[1][:, :1]))
    # r_max: the rows left short are exactly those whose k-th neighbour lies beyond the last radius used
    idx, d2, levels = nbr.knn(I, Q, k, 0.25, r_max=1.5)
    assert levels == 3                                            # 0.25, 0.5, 1.0; 2.0 passes r_max
    short = idx[:, -1] < 0
    fq = np.isfinite(Q[:, :3]).all(1)
    assert np.array_equal(short[fq], (want[1][:, -1] > np.float32(1.0))[fq]) and short[fq].any() and (~short).any()
    assert _same((idx[~short], d2[~short]), (want[0][~short], want[1][~short]))
    last = nbr.knn_within(I, Q, k, 1.0)
    assert _same((idx[short], d2[short]), (last[0][short], last[1][short]))
    # fewer finite records than k: the rows stay padded and the loop ends
    few = I[:8]
    idx, d2, levels = nbr.knn(few, Q[:50], 12, 0.25)
    n_fin = int(np.isfinite(few[:, :3]).all(1).sum())
    fq = np.isfinite(Q[:50, :3]).all(1)
    assert ((idx >= 0).sum(1)[fq] == n_fin).all() and _same((idx, d2), _unbounded(few, Q[:50], 12))
    # the self query: the point itself (or an exact duplicate before it) comes first
    idx, d2, _ = nbr.knn(I, None, 3, 0.25)
    fi = np.isfinite(I[:, :3]).all(1)
    assert (d2[fi, 0] == 0).all() and (idx[fi, 0] <= np.flatnonzero(fi)).all() and (idx[~fi] == -1).all()
    assert np.array_equal(_bits(I[idx[fi, 0], :3]), _bits(I[fi, :3]))


def sor_cloud():
    cluster = np.array([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1], [0.1, 0.1, 0], [0.1, 0, 0.1]], float)
    pair = np.array([[3, 0, 0], [3.2, 0, 0]], float)
    single = np.array([[-20, 5, 0]], float)
    cloud = np.concatenate([cluster, pair, single, [[np.nan, 0, 0]]], 0)
    return np.concatenate([cloud, np.ones((cloud.shape[0], 1))], 1).astype(np.float32)


def test_statistical_outlier_mask_on_a_hand_made_cloud(S):
    """mean_k = 2: the cluster's mean distances are 0.1 to 0.13, the pair's (0.2 + 3) / 2 = 1.6, the lone point's 20.5; over the nine
    valid points mean = 2.7 and the standard deviation 6.7"""
    from scaloam import nbr
    cloud = sor_cloud()
    idx, d2, _ = nbr.knn(cloud, None, 3, 0.25)
    dist = np.sqrt(d2[:9, 1:].astype(np.float64)).mean(1)
    assert dist[:6].max() < 0.15 and 1.5 < dist[6:8].min() and dist[6:8].max() < 1.7 and 20 < dist[8] < 21
    mean, std = dist.mean(), dist.std(ddof=1)
    assert 2.6 < mean < 2.8 and 6.5 < std < 6.9
    assert list(nbr.statistical_outlier_mask(cloud, 2, 1.0, 0.25)) == [True] * 8 + [False, False]      # thr about 9.4
    assert list(nbr.statistical_outlier_mask(cloud, 2, -0.3, 0.25)) == [True] * 6 + [False] * 4       # thr about 0.7
    assert list(nbr.statistical_outlier_mask(cloud, 2, 3.0, 0.25)) == [True] * 9 + [False]            # thr about 23
    # r_max below the lone point's distance: its row stays short, it is dropped and leaves the statistics
    m = nbr.statistical_outlier_mask(cloud, 2, 1.0, 0.25, r_max=5.0)
    d8 = dist[:8]
    thr = d8.mean() + d8.std(ddof=1)
    assert list(m) == list(d8 <= thr) + [False, False] and list(m) == [True] * 6 + [False] * 4
    # more neighbours asked for than the cloud has: nothing is valid
    assert not nbr.statistical_outlier_mask(cloud, 9, 1.0, 0.25).any()
    assert nbr.statistical_outlier_mask(np.zeros((0, 4), np.float32), 2, 1.0, 0.25).shape == (0,)


def test_restatement_argument_checks(S):
    from scaloam import nbr
    p = np.zeros((3, 4), np.float32)
    for k in (0, -1, 65, 2.5):
        with pytest.raises(ValueError):
            nbr.knn_within(p, p, k, 0.5)
        with pytest.raises(ValueError):
            nbr.knn(p, p, k, 0.5)
    for r in (0.0, -1.0, float("nan"), float("inf"), 1e-60, 1e60):
        with pytest.raises(ValueError):
            nbr.knn_within(p, p, 1, r)
        with pytest.raises(ValueError):
            nbr.knn(p, p, 1, r)
    with pytest.raises(ValueError):
        nbr.knn_within(p, p, 1, 0.5, path="grid")
    with pytest.raises(ValueError):
        nbr.knn(p, p, 1, 0.5, r_max=0.25)
    for mean_k in (0, 64, -3, 1.5):
        with pytest.raises(ValueError):
            nbr.statistical_outlier_mask(p, mean_k, 1.0, 0.5)
    for std_mul in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            nbr.statistical_outlier_mask(p, 2, std_mul, 0.5)
    assert nbr.MAX_K == S.NBR_MAX_K == 64


def test_knn_argument_checks_and_no_device(S):
    L = S.lib()
    i32p, f32p = C.POINTER(C.c_int), C.POINTER(C.c_float)
    q, idx, d2 = np.zeros((4, 4), np.float32), np.zeros((4, 64), np.int32), np.zeros((4, 64), np.float32)
    pq, pi, pd = q.ctypes.data_as(f32p), idx.ctypes.data_as(i32p), d2.ctypes.data_as(f32p)
    # null contexts are refused before anything touches a device
    assert L.scal_nbr_knn(None, pq, 4, 5, pi, pd) == S.E_ARG and b"scal_nbr_knn" in L.scal_last_error()
    assert L.scal_nbr_knn_device(None, None, 0, 5, None, None) == S.E_ARG
    assert L.scal_nbr_knn_self(None, 5, pi, pd) == S.E_ARG and b"scal_nbr_knn_self" in L.scal_last_error()
    if S.device_count() < 1:
        with pytest.raises(S.ScalError) as e:
            S.RadiusIndex(100, 100).knn(q, 5)
        assert e.value.code == S.E_NO_DEVICE
        from scaloam import nbr
        with pytest.raises(S.ScalError) as e:
            nbr.knn(q, q, 2, 0.5, device=True)
        assert e.value.code == S.E_NO_DEVICE
        with pytest.raises(S.ScalError) as e:
            nbr.statistical_outlier_mask(q, 2, 1.0, 0.5, device=True)
        assert e.value.code == S.E_NO_DEVICE


def test_sor_filter_tool_without_a_device(S, tmp_path):
    """tools/replay_mapmerge.py --sor-filter: a malformed argument is refused; without a device the tool says so (SCAL_E_NO_DEVICE)
    and writes nothing (with one, tests/test_knn_gpu.py compares what it writes)"""
    from scaloam import formats
    X, _ = _scene_tool().two_sessions(2.0, 0)
    ses = tmp_path / "old"
    (ses / "Scans").mkdir(parents=True)
    for k, s in enumerate(X["scans"]):
        formats.write_pcd_binary(str(ses / "Scans" / f"{k:06d}.pcd"), s)
    formats.write_poses(str(ses / "optimized_poses.txt"), X["poses"])
    tool = [sys.executable, os.path.join(ROOT, "tools", "replay_mapmerge.py"), str(ses)]
    out = tmp_path / "map.pcd"
    for bad in ("10", "0,1.0", "64,1.0", "10,nan", "10,1.0,0"):
        r = subprocess.run(tool + ["--out", str(out), "--sor-filter", bad], capture_output=True, text=True)
        assert r.returncode != 0 and "--sor-filter" in r.stderr and not out.exists(), bad
    if S.device_count() < 1:
        r = subprocess.run(tool + ["--out", str(out), "--sor-filter", "10,1.0"], capture_output=True, text=True)
        assert r.returncode != 0 and "error -7" in r.stderr and not out.exists()
