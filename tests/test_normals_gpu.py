"""scal_nbr_normals* on the device against the CPU restatement (scaloam/nbr.py normals_within; tests/test_normals_cpu.py holds that to
numpy.linalg.eigh): the bits of nc and dist equal on the inputs tools/mapdiff_scene.py names, NaN rows included; the viewpoint, sizes,
a cell streamed in batches, permutations, the self query, chunking, device buffers, other calls and a new index in between, the
statistics, every error code, the two uses in scaloam.nbr, the golden map and the tool."""
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
NAN = 0x7FC00000
VIEWPOINT = (0.5, -0.25, 40.0)


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
def _rows(r):
    """knn_within at k = 64 (a smaller k is its first columns): the neighbour search is done once per radius"""
    from scaloam import nbr
    I, Q = _inputs(r)
    return nbr.knn_within(I, Q, 64, r)[0]


@functools.lru_cache(maxsize=None)
def _ref(r, k, viewpoint=None):
    from scaloam import nbr
    I, Q = _inputs(r)
    return nbr.fit_rows(I, Q, _rows(r)[:, :k], viewpoint)


def _same(got, want):
    return (got[0].dtype == np.float32 and got[1].dtype == np.float32 and got[0].shape == want[0].shape and got[1].shape == want[1].shape
            and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)))


def _index(S, I, r, nq):
    idx = S.RadiusIndex(max(I.shape[0], 1), max(nq, 1))
    idx.set_index(I, r)
    return idx


def _all_nan(got, n):
    return got[0].shape == (n, 4) and got[1].shape == (n,) and (got[0].view(np.uint32) == NAN).all() and (got[1].view(np.uint32) == NAN).all()


def test_the_reference_is_the_restatement():
    """_ref shares one neighbour search among the tests; it is normals_within"""
    from scaloam import nbr
    I, Q = _inputs(0.5)
    assert _same(_ref(0.5, 20, VIEWPOINT), nbr.normals_within(I, Q, 20, 0.5, viewpoint=VIEWPOINT))


@pytest.mark.parametrize("r", [0.5, 1.0])
@pytest.mark.parametrize("k", [3, 5, 20, 63, 64])
def test_bits_equal_the_restatement(S, r, k):
    I, Q = _inputs(r)
    want = _ref(r, k)
    none = want[1].view(np.uint32) == NAN
    assert none.any() and (~none).sum() > 2000 and (want[0].view(np.uint32)[none] == NAN).all()
    idx = _index(S, I, r, Q.shape[0])
    got = idx.normals(Q, k)
    bad = np.flatnonzero((got[0].view(np.uint32) != want[0].view(np.uint32)).any(1) | (got[1].view(np.uint32) != want[1].view(np.uint32)))
    print("rows that differ:", bad.size, "of", Q.shape[0], bad[:5], got[0][bad[:5]], want[0][bad[:5]], got[1][bad[:5]], want[1][bad[:5]])
    assert _same(got, want)
    st = idx.stats()
    idx.knn(Q, k)
    assert idx.stats() == st and st["work_items"] > 0       # the same front end as the k-NN call


@pytest.mark.parametrize("r,k", [(0.5, 5), (1.0, 20), (1.0, 64)])
def test_with_a_viewpoint(S, r, k):
    I, Q = _inputs(r)
    want = _ref(r, k, VIEWPOINT)
    assert not _same(want, _ref(r, k))
    idx = _index(S, I, r, Q.shape[0])
    assert _same(idx.normals(Q, k, viewpoint=VIEWPOINT), want)
    assert _same(idx.normals(Q, k), _ref(r, k))             # and no viewpoint again afterwards


@pytest.mark.parametrize("nq", [0, 1, 63, 64, 65, 257])
def test_query_sizes(S, nq):
    from scaloam import nbr
    I, Q = _inputs(0.5)
    idx = _index(S, I, 0.5, 300)
    near = np.argsort(np.abs(Q[:, :3] - np.array([0.5, 1.5, -0.5], np.float32)).max(1), kind="stable")[:nq]     # the clump: one cell, many queries
    want = _ref(0.5, 20)
    got = idx.normals(Q[:nq], 20)
    assert got[0].shape == (nq, 4) and got[1].shape == (nq,) and _same(got, (want[0][:nq], want[1][:nq]))
    assert _same(idx.normals(Q[near], 20), (want[0][near], want[1][near]))


def test_small_indexes(S):
    from scaloam import nbr
    _, Q = _inputs(0.5)
    idx = S.RadiusIndex(10, Q.shape[0])
    idx.set_index(np.zeros((0, 4), np.float32), 0.5)
    assert _all_nan(idx.normals(Q, 3), Q.shape[0])
    got = idx.normals_self(3)
    assert got[0].shape == (0, 4) and got[1].shape == (0,) and idx.stats() == dict(pairs_tested=0, work_items=0)
    pts = np.array([[0.5, 1.5, -0.5, 7.0], [0.625, 1.5, -0.4375, 1.0], [0.5, 1.625, -0.5, 2.0]], np.float32)      # where the queries are dense
    for n in (1, 2):
        idx.set_index(pts[:n], 0.5)
        assert _all_nan(idx.normals(Q, 3), Q.shape[0]) and _all_nan(idx.normals_self(5), n)
    idx.set_index(pts, 0.5)
    want = nbr.normals_within(pts, Q, 3, 0.5)
    assert np.isfinite(want[1]).any() and _same(idx.normals(Q, 3), want)
    own = idx.normals_self(4)
    assert np.isfinite(own[0]).all() and _same(own, nbr.normals_within(pts, pts, 4, 0.5))
    dup = np.repeat(pts[:1], 3, 0)                          # C = 0: no rotation
    idx.set_index(dup, 0.5)
    nc, dist = idx.normals_self(3)
    assert nc.view(np.uint32).tolist() == [[0x3F800000, 0, 0, 0]] * 3 and dist.view(np.uint32).tolist() == [0] * 3
    idx.set_index(np.array([[np.nan, 0, 0, 0]] * 3, np.float32), 0.5)
    assert _all_nan(idx.normals(Q, 3), Q.shape[0]) and _all_nan(idx.normals_self(3), 3)


def test_one_cell_of_300_records_is_streamed_in_batches(S):
    from scaloam import nbr
    rng = np.random.default_rng(3)
    I = np.concatenate([rng.uniform(0.05, 0.95, (300, 3)), np.zeros((300, 1))], 1).astype(np.float32)     # cell (0, 0, 0) at r = 0.5: width 1
    I[17], I[250] = I[5], I[5]
    Q = np.concatenate([rng.uniform(0.0, 1.0, (70, 3)), np.zeros((70, 1))], 1).astype(np.float32)
    idx = _index(S, I, 0.5, 70)
    want = nbr.normals_within(I, Q, 64, 0.5)
    assert np.isfinite(want[1]).all() and _same(idx.normals(Q, 64), want)
    assert idx.stats()["pairs_tested"] == 300 * 70
    assert _same(idx.normals_self(64, viewpoint=(0.5, 0.5, 9.0)), nbr.normals_within(I, I, 64, 0.5, viewpoint=(0.5, 0.5, 9.0)))


def test_permutations(S):
    from scaloam import nbr
    I, Q = _inputs(1.0)
    want = _ref(1.0, 20)
    rng = np.random.default_rng(11)
    pi, pq = rng.permutation(I.shape[0]), rng.permutation(Q.shape[0])
    assert _same(_index(S, I, 1.0, Q.shape[0]).normals(Q[pq], 20), (want[0][pq], want[1][pq]))
    got = _index(S, I[pi], 1.0, Q.shape[0]).normals(Q, 20)
    assert _same(got, nbr.normals_within(I[pi], Q, 20, 1.0))
    # the sums run in row order, and a row's order changes with the positions only where two of its d2 are equal: rows without a tie
    # among their 20 entries and the next one hold the same records in the same order
    d2 = nbr.knn_within(I, Q, 21, 1.0)[1]
    untied = (d2[:, 1:] != d2[:, :-1]).all(1)
    assert untied.sum() > Q.shape[0] // 2 and _same((got[0][untied], got[1][untied]), (want[0][untied], want[1][untied]))


def test_normals_self_equals_normals_of_the_index(S):
    from scaloam import nbr
    I, _ = _inputs(0.5)
    idx = _index(S, I, 0.5, I.shape[0])
    own = idx.normals_self(11, viewpoint=VIEWPOINT)
    assert _same(own, idx.normals(I, 11, viewpoint=VIEWPOINT)) and _same(own, nbr.normals_within(I, I, 11, 0.5, viewpoint=VIEWPOINT))
    assert _same(_index(S, I, 0.5, 1).normals_self(11, viewpoint=VIEWPOINT), own)       # a self query is not bound by max_query_points


def test_chunked_queries_equal_one_call(S):
    I, Q = _inputs(1.0)
    want = _ref(1.0, 20, VIEWPOINT)
    whole = _index(S, I, 1.0, Q.shape[0])
    assert _same(whole.normals(Q, 20, viewpoint=VIEWPOINT), want)
    idx = _index(S, I, 1.0, 100)
    assert _same(idx.normals(Q, 20, viewpoint=VIEWPOINT), want)
    assert idx.stats()["pairs_tested"] == whole.stats()["pairs_tested"]


def test_device_buffers(S):
    import torch
    I, Q = _inputs(0.5)
    want = _ref(0.5, 20)
    idx = _index(S, I, 0.5, Q.shape[0])
    dq = torch.from_numpy(Q).cuda()
    dn = torch.zeros((Q.shape[0], 4), dtype=torch.float32, device="cuda")
    dd = torch.zeros(Q.shape[0], dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    idx.normals_device(dq.data_ptr(), Q.shape[0], 20, dn.data_ptr(), dd.data_ptr())
    assert _same((dn.cpu().numpy(), dd.cpu().numpy()), want)
    dn.zero_(), dd.zero_()
    torch.cuda.synchronize()
    idx.normals_device(dq.data_ptr(), Q.shape[0], 20, None, dd.data_ptr())
    assert not dn.cpu().numpy().any() and np.array_equal(dd.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    dd.zero_()
    torch.cuda.synchronize()
    idx.normals_device(dq.data_ptr(), Q.shape[0], 20, dn.data_ptr(), None, viewpoint=VIEWPOINT)
    assert not dd.cpu().numpy().any() and np.array_equal(dn.cpu().numpy().view(np.uint32), _ref(0.5, 20, VIEWPOINT)[0].view(np.uint32))
    L = S.lib()
    f32p = C.POINTER(C.c_float)
    only = np.zeros((Q.shape[0], 4), np.float32)
    assert L.scal_nbr_normals(idx.h, Q.ctypes.data_as(f32p), Q.shape[0], 20, None, only.ctypes.data_as(f32p), None) == S.OK
    assert np.array_equal(only.view(np.uint32), want[0].view(np.uint32))
    only = np.zeros(Q.shape[0], np.float32)
    assert L.scal_nbr_normals(idx.h, Q.ctypes.data_as(f32p), Q.shape[0], 20, None, None, only.ctypes.data_as(f32p)) == S.OK
    assert np.array_equal(only.view(np.uint32), want[1].view(np.uint32))
    assert L.scal_nbr_normals_self(idx.h, 20, None, None, None) == S.OK


def test_other_calls_and_a_new_index_in_between(S):
    """the position table belongs to the index: a radius query and a k-NN call leave it alone, a new index refills it"""
    from scaloam import nbr
    I, Q = _inputs(0.5)
    I2, Q2 = _inputs(1.0)
    idx = S.RadiusIndex(max(I.shape[0], I2.shape[0]), max(Q.shape[0], Q2.shape[0]))
    idx.set_index(I, 0.5)
    assert _same(idx.normals(Q, 20), _ref(0.5, 20))
    count = idx.query(Q)
    rows = idx.knn(Q, 20)
    assert np.array_equal(rows[0], _rows(0.5)[:, :20]) and np.array_equal(count[0], nbr.radius_counts(I, Q, 0.5)[0])
    assert _same(idx.normals(Q, 20), _ref(0.5, 20))
    idx.set_index(I2, 1.0)
    assert _same(idx.normals(Q2, 5), _ref(1.0, 5))
    rng = np.random.default_rng(5)
    back = I[rng.permutation(I.shape[0])]                    # the same records at other positions: a stale table would name the wrong ones
    idx.set_index(back, 0.5)
    assert _same(idx.normals(Q, 20), nbr.normals_within(back, Q, 20, 0.5))
    idx.set_index(I, 0.5)
    assert _same(idx.normals_self(5), nbr.normals_within(I, I, 5, 0.5))


def test_error_codes(S):
    L = S.lib()
    I, Q = _inputs(0.5)
    idx = S.RadiusIndex(100, 50)
    f32p = C.POINTER(C.c_float)
    rn, rd = np.zeros((200, 4), np.float32), np.zeros(200, np.float32)
    pq, pn, pd = Q[:200].ctypes.data_as(f32p), rn.ctypes.data_as(f32p), rd.ctypes.data_as(f32p)
    assert L.scal_nbr_normals(idx.h, pq, 10, 5, None, pn, pd) == S.E_STATE
    assert L.scal_nbr_normals_self(idx.h, 5, None, pn, pd) == S.E_STATE
    assert L.scal_nbr_normals_device(idx.h, pq, 10, 5, None, None, None) == S.E_STATE
    for ready in (False, True):
        if ready:
            idx.set_index(I[:100], 0.5)
        for k in (2, 1, 0, -1, 65):          # the argument comes before the state
            assert L.scal_nbr_normals(idx.h, pq, 10, k, None, pn, pd) == S.E_ARG and L.scal_nbr_normals_self(idx.h, k, None, pn, pd) == S.E_ARG
            assert L.scal_nbr_normals_device(idx.h, pq, 10, k, None, None, None) == S.E_ARG
    for k in (2, 65):
        with pytest.raises(S.ScalError) as e:
            idx.normals(Q[:10], k)
        assert e.value.code == S.E_ARG
        with pytest.raises(S.ScalError) as e:
            idx.normals_self(k)
        assert e.value.code == S.E_ARG
    assert L.scal_nbr_normals(None, pq, 10, 5, None, pn, pd) == S.E_ARG and L.scal_nbr_normals_self(None, 5, None, pn, pd) == S.E_ARG
    assert L.scal_nbr_normals(idx.h, None, 5, 5, None, pn, pd) == S.E_ARG and L.scal_nbr_normals(idx.h, pq, -1, 5, None, pn, pd) == S.E_ARG
    assert L.scal_nbr_normals_device(idx.h, None, 5, 5, None, None, None) == S.E_ARG
    assert L.scal_nbr_normals(idx.h, pq, 51, 5, None, pn, pd) == S.E_CAPACITY
    assert L.scal_nbr_normals_device(idx.h, pq, 51, 5, None, None, None) == S.E_CAPACITY
    assert L.scal_nbr_normals(idx.h, pq, 50, 64, None, pn, pd) == S.OK                # and the context still works
    from scaloam import nbr
    assert _same((rn[:50], rd[:50]), nbr.normals_within(I[:100], Q[:50], 64, 0.5))


def test_estimate_normals_and_point_to_plane_on_the_device(S):
    from scaloam import nbr
    I, Q = _inputs(0.5)
    assert _same(nbr.estimate_normals(I, 11, 0.5, viewpoint=VIEWPOINT, device=True), nbr.estimate_normals(I, 11, 0.5, viewpoint=VIEWPOINT))
    got, want = nbr.point_to_plane(I, Q, 11, 0.5, device=True), nbr.point_to_plane(I, Q, 11, 0.5)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1]) and got[1].dtype == bool
    assert nbr.residual_stats(*got) == nbr.residual_stats(*want)


def test_the_golden_map(S):
    from scaloam import nbr
    gx, _, _, _ = _scene_tool().golden_pair(GOLDEN)
    assert gx.shape[0] == 73260
    want = nbr.estimate_normals(gx, 10, 0.8)
    got = nbr.estimate_normals(gx, 10, 0.8, device=True)
    fit = want[1].view(np.uint32) != NAN
    assert 0.9 * gx.shape[0] < fit.sum() <= gx.shape[0] and _same(got, want)


def test_normals_tool(S, tmp_path):
    """tools/replay_mapmerge.py --normals writes the map once more with normals and curvature, after the filters"""
    from scaloam import formats, nbr
    X, _ = _scene_tool().two_sessions(1.0, 0)
    ses = tmp_path / "old"
    (ses / "Scans").mkdir(parents=True)
    for k, s in enumerate(X["scans"]):
        formats.write_pcd_binary(str(ses / "Scans" / f"{k:06d}.pcd"), s)
    formats.write_poses(str(ses / "optimized_poses.txt"), X["poses"])
    tool = [sys.executable, os.path.join(ROOT, "tools", "replay_mapmerge.py"), str(ses)]
    out = tmp_path / "map.pcd"
    r = subprocess.run(tool + ["--out", str(out), "--radius-filter", "0.5,2", "--normals", "10,0.6"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    kept = formats.read_pcd(str(out))
    path = str(tmp_path / "map_normals.pcd")
    assert np.array_equal(formats.read_pcd(path).view(np.uint32), kept.view(np.uint32))
    xyzi, nc = formats.read_pcd_normals(path)
    want = nbr.estimate_normals(kept, 10, 0.6)[0]
    assert np.array_equal(xyzi.view(np.uint32), kept.view(np.uint32)) and np.array_equal(nc.view(np.uint32), want.view(np.uint32))
    assert np.isfinite(nc).any()
    assert subprocess.run(tool + ["--out", str(out), "--normals", "2"], capture_output=True, text=True).returncode == 2
