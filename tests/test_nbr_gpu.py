"""scal_nbr_* on the device against the CPU restatement (scaloam/nbr.py): counts and min_d2 bit for bit on the inputs
tools/mapdiff_scene.py names (tests/test_nbr_cpu.py holds the restatement's two paths to each other on the same inputs, and the map
diff inputs to Removert's margin condition); sizes, saturation, permutations, the self query, the device inputs and outputs,
chunking, every error code; the outlier filter and the map diff, device against restatement and against ground truth."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
RADII = [0.5, 0.3, 0.7, 1.0, 1e-3]


@functools.lru_cache(maxsize=None)
def _scene_tool():
    spec = importlib.util.spec_from_file_location("mapdiff_scene", os.path.join(ROOT, "tools", "mapdiff_scene.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@functools.lru_cache(maxsize=None)
def _inputs(r):
    return _scene_tool().radius_inputs(r)


@functools.lru_cache(maxsize=None)
def _reference(r):
    from scaloam import nbr
    I, Q = _inputs(r)
    return nbr.radius_counts(I, Q, r)


def _same(got, want):
    return (got[0].dtype == np.uint16 and got[0].shape == want[0].shape and np.array_equal(got[0], want[0])
            and got[1].shape == want[1].shape and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)))


def _index(S, I, r, nq):
    idx = S.RadiusIndex(max(I.shape[0], 1), max(nq, 1))
    idx.set_index(I, r)
    return idx


@pytest.mark.parametrize("r", RADII)
def test_counts_and_min_d2_equal_the_restatement(S, r):
    I, Q = _inputs(r)
    idx = _index(S, I, r, Q.shape[0])
    got = idx.query(Q)
    assert _same(got, _reference(r))
    st = idx.stats()
    assert st["work_items"] > 0 and int(got[0].astype(np.int64).sum()) <= st["pairs_tested"] < I.shape[0] * Q.shape[0]
    if r == 0.5:   # a pair at exactly r counts: the query at the origin has the index record at (0.5, 0, 0)
        q0 = np.flatnonzero((Q[:, :3] == 0).all(1))
        assert q0.size and (got[1][q0] == 0).all()
        lone = S.RadiusIndex(4, 4)
        lone.set_index(np.array([[0, 0, 0, 0]], np.float32), 0.5)
        assert _same(lone.query(np.array([[0.5, 0, 0, 0], [0.50000006, 0, 0, 0]], np.float32)),
                     (np.array([1, 0], np.uint16), np.array([0.25, np.inf], np.float32)))


@pytest.mark.parametrize("nq", [0, 1, 63, 64, 65, 257])
def test_query_sizes(S, nq):
    from scaloam import nbr
    I, Q = _inputs(0.5)
    idx = _index(S, I, 0.5, 300)
    # the clump's surroundings first: one cell with many queries, so 63 / 64 / 65 straddle a wave
    near = np.argsort(np.abs(Q[:, :3] - np.array([0.5, 1.5, -0.5], np.float32)).max(1), kind="stable")[:nq]
    for q in (Q[:nq], Q[near]):
        got = idx.query(q)
        assert got[0].shape == (nq,) and got[1].shape == (nq,)
        assert _same(got, nbr.radius_counts(I, q, 0.5))


def test_index_sizes_zero_and_one(S):
    from scaloam import nbr
    _, Q = _inputs(0.5)
    idx = S.RadiusIndex(10, Q.shape[0])
    idx.set_index(np.zeros((0, 4), np.float32), 0.5)
    c, d = idx.query(Q)
    assert not c.any() and np.isposinf(d).all()
    c, d = idx.query_self()
    assert c.shape == (0,) and d.shape == (0,) and idx.stats() == dict(pairs_tested=0, work_items=0)
    one = np.array([[0.25, -0.25, 0.125, 7.0]], np.float32)
    idx.set_index(one, 0.5)
    assert _same(idx.query(Q), nbr.radius_counts(one, Q, 0.5))
    assert _same(idx.query_self(), (np.array([1], np.uint16), np.array([0], np.float32)))
    idx.set_index(np.array([[np.nan, 0, 0, 0]], np.float32), 0.5)       # an index of one record that is not finite
    c, d = idx.query(Q)
    assert not c.any() and np.isposinf(d).all()
    assert _same(idx.query_self(), (np.array([0], np.uint16), np.array([np.inf], np.float32)))


def test_counts_saturate(S):
    """70,000 records inside a ball of diameter r / 2, self query: by the definition every count is 65535 and every min_d2 is 0"""
    rng = np.random.default_rng(5)
    r, n = 0.5, 70000
    d = rng.normal(size=(n, 3))
    d *= (rng.uniform(0, 1, (n, 1)) ** (1 / 3)) * (r / 4) / np.linalg.norm(d, axis=1, keepdims=True)
    P = np.concatenate([d + np.array([0.6, 0.6, 0.6]), np.zeros((n, 1))], 1).astype(np.float32)
    assert np.linalg.norm(P[:, :3].astype(np.float64) - 0.6, axis=1).max() < r / 4 + 1e-6
    idx = _index(S, P, r, 1)
    c, d2 = idx.query_self()
    assert c.shape == (n,) and (c == 65535).all() and (d2 == 0).all()
    assert idx.stats()["pairs_tested"] == n * n


def test_permutations(S):
    I, Q = _inputs(0.7)
    want = _reference(0.7)
    rng = np.random.default_rng(11)
    pi, pq = rng.permutation(I.shape[0]), rng.permutation(Q.shape[0])
    assert _same(_index(S, I[pi], 0.7, Q.shape[0]).query(Q), want)
    assert _same(_index(S, I, 0.7, Q.shape[0]).query(Q[pq]), (want[0][pq], want[1][pq]))


def test_query_self_equals_query_of_the_index(S):
    from scaloam import nbr
    I, _ = _inputs(0.3)
    idx = _index(S, I, 0.3, I.shape[0])
    own = idx.query_self()
    assert _same(own, idx.query(I)) and _same(own, nbr.radius_counts(I, I, 0.3))
    assert _same(_index(S, I, 0.3, 1).query_self(), own)       # a self query is not bound by max_query_points


def test_a_second_index_and_radius_on_one_context(S):
    I, Q = _inputs(0.5)
    I2, Q2 = _inputs(1.0)
    idx = S.RadiusIndex(max(I.shape[0], I2.shape[0]), max(Q.shape[0], Q2.shape[0]))
    idx.set_index(I, 0.5)
    assert _same(idx.query(Q), _reference(0.5))
    idx.set_index(I2[:1500], 1.0)
    from scaloam import nbr
    assert _same(idx.query(Q2), nbr.radius_counts(I2[:1500], Q2, 1.0))
    idx.set_index(I, 0.5)
    assert _same(idx.query(Q), _reference(0.5))


def test_chunked_queries_equal_one_call(S):
    I, Q = _inputs(1.0)
    want = _reference(1.0)
    whole = _index(S, I, 1.0, Q.shape[0])
    assert _same(whole.query(Q), want)
    for cap in (1000, 257, 64):
        idx = _index(S, I, 1.0, cap)
        assert _same(idx.query(Q), want), cap
        assert idx.stats()["pairs_tested"] == whole.stats()["pairs_tested"], cap


def test_device_index_input_and_device_outputs(S):
    """the points a MapMerge holds on the device as the index, against the same points downloaded; queries and outputs in device memory"""
    import torch
    from scaloam import nbr
    scans = [np.load(os.path.join(GOLDEN, f"KAIST03_{k:06d}.npy")).astype(np.float32) for k in (0, 7, 20)]
    P = np.load(os.path.join(GOLDEN, "KAIST03_poses21.npy")).reshape(-1, 12).astype(np.float64)[[0, 7, 20]]
    mm = S.MapMerge(max_points=200000, max_frame_points=50000)
    for s, p in zip(scans, P):
        mm.add(s, p, near_thres=2.0)
    pts = mm.download()
    Q = pts[::37].copy()
    Q[:, :3] += np.float32(0.05)
    idx_d, idx_h = S.RadiusIndex(pts.shape[0], Q.shape[0]), S.RadiusIndex(pts.shape[0], Q.shape[0])
    idx_d.set_index_device(mm, 0.5)
    idx_h.set_index(pts, 0.5)
    want = nbr.radius_counts(pts, Q, 0.5)
    got_h = idx_h.query(Q)
    st = idx_h.stats()
    assert _same(idx_d.query(Q), got_h) and _same(got_h, want) and idx_d.stats() == st and st["work_items"] > 0
    assert _same(idx_d.query_self(), idx_h.query_self())
    dq = torch.from_numpy(Q).cuda()
    dc = torch.zeros(Q.shape[0], dtype=torch.int16, device="cuda")
    dd = torch.zeros(Q.shape[0], dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    idx_d.query_device(dq.data_ptr(), Q.shape[0], dc.data_ptr(), dd.data_ptr())
    assert _same((dc.cpu().numpy().view(np.uint16), dd.cpu().numpy()), want) and idx_d.stats() == st
    # either output may be left out
    dc.zero_(), dd.zero_()
    torch.cuda.synchronize()
    idx_d.query_device(dq.data_ptr(), Q.shape[0], None, dd.data_ptr())
    assert not dc.cpu().numpy().any() and np.array_equal(dd.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    L = S.lib()
    cnt = np.zeros(Q.shape[0], np.uint16)
    assert L.scal_nbr_query(idx_h.h, Q.ctypes.data_as(C.POINTER(C.c_float)), Q.shape[0], cnt.ctypes.data_as(C.POINTER(C.c_ushort)), None) == S.OK
    assert np.array_equal(cnt, want[0])
    assert L.scal_nbr_query_self(idx_h.h, None, None) == S.OK


def test_error_codes(S):
    L = S.lib()
    I, Q = _inputs(0.5)
    for bad in ((0, 10), (10, 0), (-1, 10)):
        with pytest.raises(S.ScalError) as e:
            S.RadiusIndex(*bad)
        assert e.value.code == S.E_ARG
    idx = S.RadiusIndex(100, 50)
    f32p, u16p = C.POINTER(C.c_float), C.POINTER(C.c_ushort)
    cnt, d2 = np.zeros(200, np.uint16), np.zeros(200, np.float32)
    pq = Q[:200].ctypes.data_as(f32p)
    # before any set_index
    assert L.scal_nbr_query(idx.h, pq, 10, cnt.ctypes.data_as(u16p), d2.ctypes.data_as(f32p)) == S.E_STATE
    assert L.scal_nbr_query_self(idx.h, cnt.ctypes.data_as(u16p), d2.ctypes.data_as(f32p)) == S.E_STATE
    assert L.scal_nbr_query_device(idx.h, pq, 10, None, None) == S.E_STATE
    for r in (0.0, -0.5, float("nan"), float("inf"), 1e-60, 1e60):
        with pytest.raises(S.ScalError) as e:
            idx.set_index(I[:100], r)
        assert e.value.code == S.E_ARG, r
        assert L.scal_nbr_set_index_device(idx.h, pq, 10, r) == S.E_ARG
    assert L.scal_nbr_query_self(idx.h, None, None) == S.E_STATE        # a refused set_index sets nothing
    with pytest.raises(S.ScalError) as e:
        idx.set_index(I[:101], 0.5)
    assert e.value.code == S.E_CAPACITY
    assert L.scal_nbr_set_index(idx.h, None, 5, 0.5) == S.E_ARG and L.scal_nbr_set_index(idx.h, pq, -1, 0.5) == S.E_ARG
    idx.set_index(I[:100], 0.5)
    assert L.scal_nbr_query(idx.h, pq, 51, cnt.ctypes.data_as(u16p), d2.ctypes.data_as(f32p)) == S.E_CAPACITY
    assert L.scal_nbr_query_device(idx.h, pq, 51, None, None) == S.E_CAPACITY
    assert L.scal_nbr_query(idx.h, None, 5, None, None) == S.E_ARG and L.scal_nbr_query(idx.h, pq, -1, None, None) == S.E_ARG
    assert L.scal_nbr_stats(idx.h, None, None) == S.E_ARG
    assert L.scal_nbr_query(idx.h, pq, 50, cnt.ctypes.data_as(u16p), d2.ctypes.data_as(f32p)) == S.OK   # and the context still works
    from scaloam import nbr
    assert _same((cnt[:50], d2[:50]), nbr.radius_counts(I[:100], Q[:50], 0.5))


def test_radius_outlier_mask_on_the_golden_scans(S):
    from scaloam import nbr
    scan = np.load(os.path.join(GOLDEN, "KAIST03_000000.npy")).astype(np.float32)
    want = nbr.radius_outlier_mask(scan, 0.5, 2)
    got = nbr.radius_outlier_mask(scan, 0.5, 2, device=True)
    assert got.dtype == bool and np.array_equal(got, want) and 0 < want.sum() < scan.shape[0]
    gx, gy, _, _ = _scene_tool().golden_pair(GOLDEN)
    merged = np.concatenate([gx, gy], 0)                            # keyframes 0, 7 and 20 moved by their golden poses
    want = nbr.radius_outlier_mask(merged, 0.5, 2)
    assert np.array_equal(nbr.radius_outlier_mask(merged, 0.5, 2, device=True), want) and 0 < want.sum() < merged.shape[0]


def test_map_diff_on_the_constructed_scene(S):
    from scaloam import nbr
    ms = _scene_tool()
    X, Y = ms.two_sessions(1.0, ms.SCENE_SEED)
    lx, sx = nbr.map_diff(X["map"], Y["map"], Y["scans"], Y["poses"], device=True)
    ly, sy = nbr.map_diff(Y["map"], X["map"], X["scans"], X["poses"], device=True)
    rx, tx = nbr.map_diff(X["map"], Y["map"], Y["scans"], Y["poses"])
    ry, ty = nbr.map_diff(Y["map"], X["map"], X["scans"], X["poses"])
    assert tx["margin"] > 1e-9 and ty["margin"] > 1e-9
    assert np.array_equal(lx, rx) and np.array_equal(ly, ry)
    assert np.array_equal(lx, X["labels"]) and np.array_equal(ly, Y["labels"])
    for dev, ref in ((sx, tx), (sy, ty)):
        assert all(dev[k] == ref[k] for k in ("common", "unobserved", "changed", "candidates")) and dev["margin"] is None
        assert dev["removert"]["dynamic"] == ref["removert"]["dynamic"] == ref["changed"]
    up = nbr.update_map(X["map"], lx, Y["map"], ly)
    assert up.shape[0] == (X["what"] == ms.STATIC).sum() + (X["what"] == ms.OBJ_B).sum() + (Y["what"] == ms.OBJ_C).sum()


def test_map_diff_on_the_golden_pair(S):
    from scaloam import nbr
    gx, gy, scans, poses = _scene_tool().golden_pair(GOLDEN)
    ref, rst = nbr.map_diff(gx, gy, scans, poses)
    assert rst["margin"] > 1e-9
    got, gst = nbr.map_diff(gx, gy, scans, poses, device=True)
    assert np.array_equal(got, ref) and gst["changed"] == rst["changed"] > 0 and gst["unobserved"] == rst["unobserved"] > 0
