"""scal_nbr_knn* on the device against the CPU restatement (scaloam/nbr.py knn_within): idx and the d2 bits equal on the inputs
tools/mapdiff_scene.py names (tests/test_knn_cpu.py holds the restatement's two paths to each other on the same inputs); the tie
order, sizes, a cell streamed in batches, permutations, the self query, chunking, device buffers, the radius query beside it, every
error code; the escalation and the statistical outlier filter, device against restatement."""
import ctypes as C
import functools
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@functools.lru_cache(maxsize=None)
def _scene_tool():
    spec = importlib.util.spec_from_file_location("mapdiff_scene", os.path.join(ROOT, "tools", "mapdiff_scene.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@functools.lru_cache(maxsize=None)
def _cpu_cases():
    spec = importlib.util.spec_from_file_location("test_knn_cpu", os.path.join(ROOT, "tests", "test_knn_cpu.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@functools.lru_cache(maxsize=None)
def _inputs(r):
    return _scene_tool().radius_inputs(r)


@functools.lru_cache(maxsize=None)
def _reference(r):
    """knn_within at k = 64; a smaller k is its first columns"""
    from scaloam import nbr
    I, Q = _inputs(r)
    return nbr.knn_within(I, Q, 64, r)


def _ref(r, k):
    idx, d2 = _reference(r)
    return idx[:, :k], d2[:, :k]


def _same(got, want):
    return (got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[0].shape == want[0].shape == got[1].shape == want[1].shape
            and np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)))


def _index(S, I, r, nq):
    idx = S.RadiusIndex(max(I.shape[0], 1), max(nq, 1))
    idx.set_index(I, r)
    return idx


@pytest.mark.parametrize("r", [0.5, 1.0])
@pytest.mark.parametrize("k", [1, 5, 20, 63, 64])
def test_rows_equal_the_restatement(S, r, k):
    I, Q = _inputs(r)
    want = _ref(r, k)
    full = want[0][:, -1] >= 0
    assert full.any() and (~full).any()
    idx = _index(S, I, r, Q.shape[0])
    got = idx.knn(Q, k)
    assert _same(got, want)
    st = idx.stats()
    assert st["work_items"] > 0 and int((got[0] >= 0).sum()) <= st["pairs_tested"] < I.shape[0] * Q.shape[0]
    idx.query(Q)
    assert idx.stats() == st          # the same front end: the radius query tests the same pairs in the same work items


def test_a_small_radius(S):
    from scaloam import nbr
    I, Q = _inputs(1e-3)
    want = nbr.knn_within(I, Q, 5, 1e-3)
    assert (want[0][:, 0] >= 0).any() and (want[0][:, -1] < 0).any()
    assert _same(_index(S, I, 1e-3, Q.shape[0]).knn(Q, 5), want)


def test_ties_follow_the_input_position(S):
    I, q, order = _cpu_cases().tie_case()
    idx = _index(S, I, 0.5, 1)
    for k in range(1, 11):
        got, d2 = idx.knn(q, k)
        want = (order + [-1] * k)[:k]
        assert list(got[0]) == want, k
        assert list(d2[0]) == [0.0 if p == 3 else 0.25 if p >= 0 else np.inf for p in want]
    got, _ = _index(S, I[::-1].copy(), 0.5, 1).knn(q, 8)
    assert list(got[0]) == [4, 0, 1, 2, 3, 5, 6, 7]


@pytest.mark.parametrize("nq", [0, 1, 63, 64, 65, 257])
def test_query_sizes(S, nq):
    from scaloam import nbr
    I, Q = _inputs(0.5)
    idx = _index(S, I, 0.5, 300)
    # the clump's surroundings: one cell with many queries, so 63 / 64 / 65 straddle a wave
    near = np.argsort(np.abs(Q[:, :3] - np.array([0.5, 1.5, -0.5], np.float32)).max(1), kind="stable")[:nq]
    for q, ref in ((Q[:nq], _ref(0.5, 20)), (Q[near], None)):
        got = idx.knn(q, 20)
        assert got[0].shape == (nq, 20) and got[1].shape == (nq, 20)
        assert _same(got, (ref[0][:nq], ref[1][:nq]) if ref else nbr.knn_within(I, q, 20, 0.5))


def test_index_sizes_zero_and_one(S):
    from scaloam import nbr
    _, Q = _inputs(0.5)
    idx = S.RadiusIndex(10, Q.shape[0])
    idx.set_index(np.zeros((0, 4), np.float32), 0.5)
    i, d = idx.knn(Q, 3)
    assert i.shape == (Q.shape[0], 3) and (i == -1).all() and np.isposinf(d).all()
    i, d = idx.knn_self(3)
    assert i.shape == (0, 3) and d.shape == (0, 3) and idx.stats() == dict(pairs_tested=0, work_items=0)
    one = np.array([[0.25, -0.25, 0.125, 7.0]], np.float32)
    idx.set_index(one, 0.5)
    got = idx.knn(Q, 3)
    assert _same(got, nbr.knn_within(one, Q, 3, 0.5)) and (got[0][:, 0] == 0).any() and (got[0][:, 1:] == -1).all()
    assert _same(idx.knn_self(2), (np.array([[0, -1]], np.int32), np.array([[0, np.inf]], np.float32)))
    idx.set_index(np.array([[np.nan, 0, 0, 0]], np.float32), 0.5)       # an index of one record that is not finite
    i, d = idx.knn(Q, 3)
    assert (i == -1).all() and np.isposinf(d).all()
    assert _same(idx.knn_self(2), (np.array([[-1, -1]], np.int32), np.array([[np.inf, np.inf]], np.float32)))


def test_one_cell_of_300_records_is_streamed_in_batches(S):
    """300 records in one cell (batches of 64, 64, 64, 64 and 44), k = 64: the nearest 64 come from every batch"""
    from scaloam import nbr
    rng = np.random.default_rng(3)
    I = np.concatenate([rng.uniform(0.05, 0.95, (300, 3)), np.zeros((300, 1))], 1).astype(np.float32)     # cell (0, 0, 0) at r = 0.5: width 1
    I[17], I[250] = I[5], I[5]                                                                             # duplicates across batches
    Q = np.concatenate([rng.uniform(0.0, 1.0, (70, 3)), np.zeros((70, 1))], 1).astype(np.float32)
    want = nbr.knn_within(I, Q, 64, 0.5)
    assert (want[0][:, -1] >= 0).any() and (want[0].max(1) >= 256).any()
    idx = _index(S, I, 0.5, 70)
    assert _same(idx.knn(Q, 64), want)
    assert idx.stats()["pairs_tested"] == 300 * 70
    assert _same(idx.knn_self(64), nbr.knn_within(I, I, 64, 0.5))


def test_permutations(S):
    I, Q = _inputs(1.0)
    want = _ref(1.0, 20)
    rng = np.random.default_rng(11)
    pi, pq = rng.permutation(I.shape[0]), rng.permutation(Q.shape[0])
    got = _index(S, I, 1.0, Q.shape[0]).knn(Q[pq], 20)
    assert _same(got, (want[0][pq], want[1][pq]))
    # a permuted index changes idx only through the positions: the records named are the same wherever no tie is reordered
    from scaloam import nbr
    gi, gd = _index(S, I[pi], 1.0, Q.shape[0]).knn(Q, 20)
    assert _same((gi, gd), nbr.knn_within(I[pi], Q, 20, 1.0))
    assert np.array_equal(gd.view(np.uint32), want[1].view(np.uint32))
    back = np.where(gi >= 0, pi[np.maximum(gi, 0)], -1)
    untied = np.ones(gd.shape, bool)
    untied[:, 1:] &= gd[:, 1:] != gd[:, :-1]
    untied[:, :-1] &= gd[:, :-1] != gd[:, 1:]
    untied[:, -1] = False                       # the last entry may tie with a record behind the row
    assert untied.sum() > untied.size // 2 and np.array_equal(back[untied], want[0][untied])


def test_knn_self_equals_knn_of_the_index(S):
    from scaloam import nbr
    I, _ = _inputs(0.5)
    idx = _index(S, I, 0.5, I.shape[0])
    own = idx.knn_self(11)
    assert _same(own, idx.knn(I, 11)) and _same(own, nbr.knn_within(I, I, 11, 0.5))
    fin = np.isfinite(I[:, :3]).all(1)
    assert (own[1][fin, 0] == 0).all() and (own[0][fin, 0] <= np.flatnonzero(fin)).all() and (own[0][~fin] == -1).all()
    assert _same(_index(S, I, 0.5, 1).knn_self(11), own)       # a self query is not bound by max_query_points


def test_chunked_queries_equal_one_call(S):
    I, Q = _inputs(1.0)
    want = _ref(1.0, 20)
    whole = _index(S, I, 1.0, Q.shape[0])
    assert _same(whole.knn(Q, 20), want)
    idx = _index(S, I, 1.0, 100)
    assert _same(idx.knn(Q, 20), want)
    assert idx.stats()["pairs_tested"] == whole.stats()["pairs_tested"]


def test_device_buffers(S):
    import torch
    I, Q = _inputs(0.5)
    want = _ref(0.5, 20)
    idx = _index(S, I, 0.5, Q.shape[0])
    dq = torch.from_numpy(Q).cuda()
    di = torch.zeros((Q.shape[0], 20), dtype=torch.int32, device="cuda")
    dd = torch.zeros((Q.shape[0], 20), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    idx.knn_device(dq.data_ptr(), Q.shape[0], 20, di.data_ptr(), dd.data_ptr())
    assert _same((di.cpu().numpy(), dd.cpu().numpy()), want)
    di.zero_(), dd.zero_()       # either output may be left out
    torch.cuda.synchronize()
    idx.knn_device(dq.data_ptr(), Q.shape[0], 20, None, dd.data_ptr())
    assert not di.cpu().numpy().any() and np.array_equal(dd.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    L = S.lib()
    only = np.zeros((Q.shape[0], 20), np.int32)
    assert L.scal_nbr_knn(idx.h, Q.ctypes.data_as(C.POINTER(C.c_float)), Q.shape[0], 20, only.ctypes.data_as(C.POINTER(C.c_int)), None) == S.OK
    assert np.array_equal(only, want[0])
    assert L.scal_nbr_knn_self(idx.h, 20, None, None) == S.OK


def test_radius_query_beside_knn_and_a_new_radius(S):
    from scaloam import nbr
    I, Q = _inputs(0.5)
    I2, Q2 = _inputs(1.0)
    idx = S.RadiusIndex(max(I.shape[0], I2.shape[0]), max(Q.shape[0], Q2.shape[0]))
    idx.set_index(I, 0.5)
    before = idx.query(Q)
    assert _same(idx.knn(Q, 64), _ref(0.5, 64))
    after = idx.query(Q)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
    want = nbr.radius_counts(I, Q, 0.5)
    assert np.array_equal(after[0], want[0]) and np.array_equal(after[1].view(np.uint32), want[1].view(np.uint32))
    idx.set_index(I2, 1.0)                                     # a new index and radius: the k-NN call uses them
    assert _same(idx.knn(Q2, 5), _ref(1.0, 5))
    idx.set_index(I, 0.5)
    assert _same(idx.knn(Q, 5), _ref(0.5, 5))


def test_error_codes(S):
    L = S.lib()
    I, Q = _inputs(0.5)
    idx = S.RadiusIndex(100, 50)
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int)
    ri, rd = np.zeros((200, 64), np.int32), np.zeros((200, 64), np.float32)
    pq, pi, pd = Q[:200].ctypes.data_as(f32p), ri.ctypes.data_as(i32p), rd.ctypes.data_as(f32p)
    # before any set_index
    assert L.scal_nbr_knn(idx.h, pq, 10, 5, pi, pd) == S.E_STATE
    assert L.scal_nbr_knn_self(idx.h, 5, pi, pd) == S.E_STATE
    assert L.scal_nbr_knn_device(idx.h, pq, 10, 5, None, None) == S.E_STATE
    for k in (0, -1, 65):            # the argument comes before the state
        assert L.scal_nbr_knn(idx.h, pq, 10, k, pi, pd) == S.E_ARG and L.scal_nbr_knn_self(idx.h, k, pi, pd) == S.E_ARG
        assert L.scal_nbr_knn_device(idx.h, pq, 10, k, None, None) == S.E_ARG
    idx.set_index(I[:100], 0.5)
    for k in (0, -1, 65):
        assert L.scal_nbr_knn(idx.h, pq, 10, k, pi, pd) == S.E_ARG and L.scal_nbr_knn_self(idx.h, k, pi, pd) == S.E_ARG
        assert L.scal_nbr_knn_device(idx.h, pq, 10, k, None, None) == S.E_ARG
        with pytest.raises(S.ScalError) as e:
            idx.knn(Q[:10], k)
        assert e.value.code == S.E_ARG
    assert L.scal_nbr_knn(idx.h, None, 5, 5, pi, pd) == S.E_ARG and L.scal_nbr_knn(idx.h, pq, -1, 5, pi, pd) == S.E_ARG
    assert L.scal_nbr_knn_device(idx.h, None, 5, 5, None, None) == S.E_ARG
    assert L.scal_nbr_knn(idx.h, pq, 51, 5, pi, pd) == S.E_CAPACITY
    assert L.scal_nbr_knn_device(idx.h, pq, 51, 5, None, None) == S.E_CAPACITY
    assert L.scal_nbr_knn(idx.h, pq, 50, 64, pi, pd) == S.OK                       # and the context still works
    from scaloam import nbr
    assert _same((ri[:50], rd[:50]), nbr.knn_within(I[:100], Q[:50], 64, 0.5))


def test_escalation_and_statistical_filter_equal_the_restatement(S):
    from scaloam import nbr
    I, Q = _inputs(0.5)
    want = nbr.knn(I, Q, 20, 0.25)
    got = nbr.knn(I, Q, 20, 0.25, device=True)
    assert got[2] == want[2] > 1 and _same(got[:2], want[:2])
    want = nbr.knn(I, None, 11, 0.25, r_max=1.5)
    got = nbr.knn(I, None, 11, 0.25, r_max=1.5, device=True)
    assert got[2] == want[2] == 3 and _same(got[:2], want[:2]) and (want[0][:, -1] < 0).any()
    cloud = _cpu_cases().sor_cloud()
    for mul, keep in ((1.0, 8), (-0.3, 6)):
        m = nbr.statistical_outlier_mask(cloud, 2, mul, 0.25, device=True)
        assert m.dtype == bool and np.array_equal(m, nbr.statistical_outlier_mask(cloud, 2, mul, 0.25)) and m.sum() == keep
    m = nbr.statistical_outlier_mask(I, 10, 1.0, 0.25, device=True)
    assert np.array_equal(m, nbr.statistical_outlier_mask(I, 10, 1.0, 0.25)) and 0 < m.sum() < I.shape[0]


def test_statistical_filter_on_the_golden_map(S):
    from scaloam import nbr
    gx, _, _, _ = _scene_tool().golden_pair(GOLDEN)
    assert gx.shape[0] == 73260
    want = nbr.statistical_outlier_mask(gx, 10, 1.0, 0.25)
    got = nbr.statistical_outlier_mask(gx, 10, 1.0, 0.25, device=True)
    assert np.array_equal(got, want) and 0 < want.sum() < gx.shape[0]


def test_sor_filter_tool(S, tmp_path):
    """tools/replay_mapmerge.py --sor-filter writes merged[mask], alone and beside --radius-filter"""
    from scaloam import formats, nbr
    X, _ = _scene_tool().two_sessions(1.0, 0)
    ses = tmp_path / "old"
    (ses / "Scans").mkdir(parents=True)
    for k, s in enumerate(X["scans"]):
        formats.write_pcd_binary(str(ses / "Scans" / f"{k:06d}.pcd"), s)
    formats.write_poses(str(ses / "optimized_poses.txt"), X["poses"])
    tool = [sys.executable, os.path.join(ROOT, "tools", "replay_mapmerge.py"), str(ses)]
    plain, sor, both = tmp_path / "map.pcd", tmp_path / "map_sor.pcd", tmp_path / "map_both.pcd"
    runs = [subprocess.run(tool + ["--out", str(plain)], capture_output=True, text=True),
            subprocess.run(tool + ["--out", str(sor), "--sor-filter", "8,1.0"], capture_output=True, text=True),
            subprocess.run(tool + ["--out", str(both), "--sor-filter", "8,1.0,0.25", "--radius-filter", "0.5,2"], capture_output=True, text=True)]
    assert all(r.returncode == 0 for r in runs), [r.stderr for r in runs]
    merged = formats.read_pcd(str(plain))
    keep = nbr.statistical_outlier_mask(merged, 8, 1.0, 0.5)
    assert 0 < keep.sum() < merged.shape[0]
    assert np.array_equal(formats.read_pcd(str(sor)).view(np.uint32), merged[keep].view(np.uint32))
    keep2 = nbr.statistical_outlier_mask(merged, 8, 1.0, 0.25) & nbr.radius_outlier_mask(merged, 0.5, 2)
    assert np.array_equal(formats.read_pcd(str(both)).view(np.uint32), merged[keep2].view(np.uint32))
