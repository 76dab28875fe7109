"""scal_icp_align_plane* on the device against its CPU restatement scaloam.icp_plane (include/scaloam_hip.h):
every comparison is bit for bit.  Scenes: the room corner of tests/test_icp_plane_cpu.py and the golden KAIST03 keyframes thinned at
0.4 m with normals from RadiusIndex.normals_self(10) at r = 0.8."""
import ctypes as C

import numpy as np
import pytest

from test_icp_plane_cpu import CORNER_TOL, DBL_MAX, corner_scene, motion, moved, planes, same_result

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    from scaloam import icp_plane
    return icp_plane


@pytest.fixture(scope="module")
def corner():
    return corner_scene()


@pytest.fixture(scope="module")
def corner_ref(P, corner):
    tgt, nc, mv, _ = corner
    return P.align_plane(mv[::3], tgt, nc, max_corr_dist=2.0)


@pytest.fixture(scope="module")
def pair(S, golden):
    """(source, target, normals): keyframe 7 against 0 + 20, all thinned at 0.4 m; the target is large enough for the cell grid"""
    vg = S.VoxelGrid()
    src = vg.filter(golden("KAIST03_000007.npy"), 0.4).copy()
    tgt = np.concatenate([vg.filter(golden("KAIST03_000000.npy"), 0.4), vg.filter(golden("KAIST03_000020.npy"), 0.4)]).astype(np.float32)
    vg.close()
    idx = S.RadiusIndex(tgt.shape[0], tgt.shape[0])
    idx.set_index(tgt, 0.8)
    nc, _ = idx.normals_self(10)
    idx.close()
    assert tgt.shape[0] >= 8192                      # 4 * ICP_TC: the cell grid is built
    nan = np.isnan(nc[:, :3]).any(1).mean()
    assert 0.02 < nan < 0.5                          # NaN normals are an ordinary part of this target
    return src, tgt, nc.copy()


@pytest.fixture(scope="module")
def pair_ref(P, pair):
    src, tgt, nc = pair
    return P.align_plane(src, tgt, nc, max_corr_dist=2.0, max_iterations=12)


def ctx(S, **kw):
    kw.setdefault("max_source", 100000)
    kw.setdefault("max_target", 400000)
    kw.setdefault("max_corr_dist", 2.0)
    return S.LoopICP(**kw)


def test_one_sweep_at_every_block_shape(S, P, corner):
    tgt, nc, mv, _ = corner
    # the three lattices interleaved, each walked with a stride: every prefix of six points or more spans all three planes
    order = (np.arange(3)[None, :] * 576 + (np.arange(576)[:, None] * 37) % 576).reshape(-1)
    icp = ctx(S, max_iterations=1)
    for n in (1, 5, 6, 63, 64, 65, 255, 256, 257, 1025):   # partial waves, partial workgroups, one partial and several
        src = mv[order[:n]]
        got, want = icp.align_plane(src, tgt, nc), P.align_plane(src, tgt, nc, max_corr_dist=2.0, max_iterations=1)
        assert np.array_equal(got["first_eq"], want["first_eq"]), n
        assert got["n_correspondences"] == want["n_correspondences"] == n and np.array_equal(got["T"], want["T"]), n
        assert same_result(got, want)
        assert (got["state"], got["iterations"]) == ((5, 0) if n < 6 else (1, 1)), n
    icp.close()


def test_whole_alignment_of_the_corner(S, corner, corner_ref):
    tgt, nc, mv, M = corner
    icp = ctx(S)
    got = icp.align_plane(mv[::3], tgt, nc)
    icp.close()
    assert same_result(got, corner_ref)
    assert got["state"] == 2 and np.abs(got["T"] - np.linalg.inv(M)).max() <= CORNER_TOL


def test_whole_alignment_of_the_golden_pair(S, pair, pair_ref):
    src, tgt, nc = pair
    icp = ctx(S, max_iterations=12)
    got = icp.align_plane(src, tgt, nc)
    icp.close()
    print("golden pair:", {k: got[k] for k in ("iterations", "state", "n_correspondences", "fitness", "plane_fitness")})
    assert same_result(got, pair_ref)
    assert got["iterations"] >= 2 and 6 <= got["n_correspondences"] < src.shape[0]


def test_search_modes_agree(S, pair, pair_ref):
    src, tgt, nc = pair
    far = src.copy()
    far[:, 0] += 30.0                                # most queries unresolved by the grid at first: the dense-sweep list path
    grid, dense = ctx(S, max_iterations=12), ctx(S, max_iterations=12)
    dense.set_search(0)
    assert same_result(grid.align_plane(src, tgt, nc), pair_ref) and same_result(dense.align_plane(src, tgt, nc), pair_ref)
    for x in (grid, dense):
        x.close()
    grid, dense = ctx(S, max_iterations=6, max_corr_dist=150.0), ctx(S, max_iterations=6, max_corr_dist=150.0)
    dense.set_search(0)
    rg, rd = grid.align_plane(far, tgt, nc), dense.align_plane(far, tgt, nc)
    assert same_result(rg, rd) and rg["iterations"] >= 1 and rg["n_correspondences"] > 6
    for x in (grid, dense):
        x.close()


def test_duplicated_target_points_resolve_to_the_lowest_index(S, P, pair):
    src, tgt, nc = pair
    extra = np.array([[5000.0, -3000.0, 40.0, 0.0], [np.nan, 1.0, 2.0, 0.0]], np.float32)
    odd = np.concatenate([tgt, tgt[:500], extra]).astype(np.float32)
    up = np.tile(np.array([0, 0, 1, 0], np.float32), (502, 1))
    side = np.tile(np.array([1, 0, 0, 0], np.float32), (502, 1))
    nc_up, nc_side = np.concatenate([nc, up]), np.concatenate([nc, side])
    want = P.align_plane(src, odd, nc_up, max_corr_dist=2.0, max_iterations=6)
    for mode in (1, 0):
        icp = ctx(S, max_iterations=6)
        icp.set_search(mode)
        a, b = icp.align_plane(src, odd, nc_up), icp.align_plane(src, odd, nc_side)
        # the copies' normals are never read: the original, at the lower index, wins every equal distance
        assert same_result(a, want) and same_result(b, want)
        # and it is the index that decides: the same two sets of normals the other way round change the result
        first = nc_up.copy()
        first[:500] = side[:500]
        c = icp.align_plane(src, odd, first)
        assert not np.array_equal(c["first_eq"], a["first_eq"])
        icp.close()


def test_host_and_device_pointers_agree(S, pair, pair_ref):
    import torch
    src, tgt, nc = pair
    assert np.isnan(nc).any()                        # NaN normals are dropped on the device path as on the host path
    d_src, d_tgt, d_nc = (torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in (src, tgt, nc))
    icp = ctx(S, max_iterations=12)
    got = icp.align_plane_device(d_src.data_ptr(), src.shape[0], d_tgt.data_ptr(), d_nc.data_ptr(), tgt.shape[0])
    assert same_result(got, pair_ref)
    g = np.eye(4, dtype=np.float32)
    g[:3, 3] = [0.2, -0.1, 0.05]
    assert same_result(icp.align_plane_device(d_src.data_ptr(), src.shape[0], d_tgt.data_ptr(), d_nc.data_ptr(), tgt.shape[0], g),
                       icp.align_plane(src, tgt, nc, g))
    icp.close()


def test_degenerate_and_short_systems_leave_the_context_usable(S, P, corner, corner_ref):
    tgt, nc, mv, _ = corner
    icp = ctx(S)
    for normals in ([(0, 0, 1)], [(0.3, -0.2, -1), (0.5, 0.7, 0.1)]):
        t2, n2 = planes(normals)
        src = moved(t2, motion())[::3]
        got = icp.align_plane(src, t2, n2)
        assert got["state"] == 6 and got["iterations"] == 0 and not got["converged"] and np.array_equal(got["T"], np.eye(4))
        assert same_result(got, P.align_plane(src, t2, n2, max_corr_dist=2.0))
        assert same_result(icp.align_plane(mv[::3], tgt, nc), corner_ref)
    got = icp.align_plane(mv[::3], tgt, np.full_like(nc, np.nan))
    assert got["state"] == 5 and got["n_correspondences"] == 0 and got["plane_fitness"] == DBL_MAX and got["fitness"] < DBL_MAX
    assert same_result(got, P.align_plane(mv[::3], tgt, np.full_like(nc, np.nan), max_corr_dist=2.0))
    empty = np.zeros((0, 4), np.float32)
    assert same_result(icp.align_plane(empty, tgt, nc), P.align_plane(empty, tgt, nc, max_corr_dist=2.0))
    assert same_result(icp.align_plane(mv[::3], tgt, nc), corner_ref)
    icp.close()


def test_alternating_with_point_to_point_on_one_context(S, P, corner, corner_ref):
    tgt, nc, mv, _ = corner
    src = mv[::3]
    fresh = ctx(S)
    point_ref = fresh.align(src, tgt)                # a context that never aligns by planes
    fresh.close()
    icp = ctx(S)
    before = icp.align(src, tgt)
    for _ in range(2):
        assert same_result(icp.align_plane(src, tgt, nc), corner_ref)
        after = icp.align(src, tgt)
        assert same_result(after, before) and same_result(after, point_ref)
    # a target of another size, its records at other positions: no normal of the earlier call may survive
    order = np.random.default_rng(3).permutation(tgt.shape[0])[:1500]
    t2, n2 = tgt[order], nc[order]
    got = icp.align_plane(src, t2, n2)
    other = ctx(S)
    assert same_result(got, other.align_plane(src, t2, n2))
    other.close()
    assert same_result(got, P.align_plane(src, t2, n2, max_corr_dist=2.0))
    assert same_result(icp.align_plane(src, tgt, nc), corner_ref)
    icp.close()


def test_register_on_the_device_equals_the_cpu(P, pair, pair_ref):
    src, tgt, _ = pair
    dev = P.register(tgt, src, device=True, max_corr_dist=2.0, max_iterations=12)
    cpu = P.register(tgt, src, device=False, max_corr_dist=2.0, max_iterations=12)
    assert same_result(dev, cpu) and same_result(dev, pair_ref)


def test_argument_checks_match_point_to_point(S, corner, corner_ref):
    tgt, nc, mv, _ = corner
    src = np.ascontiguousarray(mv[::3])
    f32p = C.POINTER(C.c_float)
    p = lambda a: a.ctypes.data_as(f32p)
    L = S.lib()
    icp = ctx(S, max_source=600, max_target=2000)
    r, rp = S.ICPResult(), S.ICPPlaneResult()
    assert L.scal_icp_align(icp.h, p(src), src.shape[0], None, tgt.shape[0], C.byref(r)) == S.E_ARG
    assert L.scal_icp_align_plane(icp.h, p(src), src.shape[0], p(tgt), None, tgt.shape[0], None, C.byref(rp)) == S.E_ARG
    assert L.scal_icp_align_plane(icp.h, p(src), src.shape[0], None, p(nc), tgt.shape[0], None, C.byref(rp)) == S.E_ARG
    assert L.scal_icp_align_plane(icp.h, p(src), src.shape[0], p(tgt), p(nc), tgt.shape[0], None, None) == S.E_ARG
    big_s, big_t = np.zeros((601, 4), np.float32), np.zeros((2001, 4), np.float32)
    assert L.scal_icp_align(icp.h, p(big_s), 601, p(tgt), tgt.shape[0], C.byref(r)) == S.E_TOO_MANY
    assert L.scal_icp_align_plane(icp.h, p(big_s), 601, p(tgt), p(nc), tgt.shape[0], None, C.byref(rp)) == S.E_TOO_MANY
    assert L.scal_icp_align_plane(icp.h, p(src), src.shape[0], p(big_t), p(big_t), 2001, None, C.byref(rp)) == S.E_TOO_MANY
    bad = np.eye(4, dtype=np.float32)
    bad[3, 3] = 2.0
    with pytest.raises(S.ScalError) as e:
        icp.align_plane(src, tgt, nc, bad)
    assert e.value.code == S.E_ARG
    assert same_result(icp.align_plane(src, tgt, nc), corner_ref)
    icp.close()
