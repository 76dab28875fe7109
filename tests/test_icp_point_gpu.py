"""scal_icp_align* (point-to-point ICP; csrc/icp.hip, icp_dev.hpp, icp_host.hpp) on the device against its CPU restatement
scaloam.icp_point: T, iterations, state, converged, n_correspondences and fitness are compared bit for bit - both sides perform the
same IEEE operations in the same order.  The scenes are synthetic and small, chosen for the places where the kernels take another
path: the dense sweep's query tiles (ICP_QT = 1024) and target chunks (ICP_TC = 2048), partial waves and workgroups of the
reduction, the cell grid's threshold (4 * ICP_TC = 8192 target points), its rings and its unresolved list, equal distances across
cells and chunks, the distance cap, non-finite records, the guess, every convergence state, one context used again and again."""
import numpy as np
import pytest

from test_icp_point_cpu import DBL_MAX, STATE_CASES, blob_scene, cloud, f32_d2, few_scene, rigid, rot, same_result

pytestmark = pytest.mark.gpu

ICP_TC, GRID_MIN = 2048, 8192


@pytest.fixture(scope="module")
def P():
    from scaloam import icp_point
    return icp_point


def ctx(S, **kw):
    kw.setdefault("max_source", 2048)
    kw.setdefault("max_target", 16384)
    return S.LoopICP(**kw)


def device(S, src, tgt, guess=None, search=1, **kw):
    """one alignment on a context of its own"""
    icp = ctx(S, **kw)
    icp.set_search(search)
    r = icp.align(src, tgt, guess)
    icp.close()
    return r


def first_sweep(src, tgt):
    """(f32 squared distance, target index) of every query's key in the restatement's first sweep"""
    from scaloam import icp_plane
    keys = icp_plane.nearest_keys(src, tgt)
    assert (keys != icp_plane._NO_KEY).all()
    return (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)


@pytest.mark.parametrize("n_tgt", [1, 3, 2047, 2048, 2049, 4097])
def test_one_sweep_at_every_block_shape_of_the_dense_path(S, P, n_tgt):
    rng = np.random.default_rng(100 + n_tgt)
    tgt = cloud(rng.uniform(-10.0, 10.0, (n_tgt, 3)))
    # the sources sit beside target points spread over every chunk, the first of them beside the chunks' first and last records
    edge = [n_tgt - 1, min(ICP_TC - 1, n_tgt - 1), min(ICP_TC, n_tgt - 1), min(2 * ICP_TC - 1, n_tgt - 1), min(2 * ICP_TC, n_tgt - 1), 0]
    beside = np.concatenate([edge, (np.arange(1025) * 997) % n_tgt]).astype(np.int64)
    all_src = cloud(tgt[beside, :3] + rng.normal(0.0, 0.02, (beside.shape[0], 3)))
    n_chunks = (n_tgt + ICP_TC - 1) // ICP_TC
    icp = ctx(S, max_iterations=1)
    for n_src in (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025):   # partial waves, workgroups and query tiles
        src = all_src[:n_src]
        want = P.align(src, tgt, max_iterations=1)
        if n_src >= 63:
            assert set(first_sweep(src, tgt)[1] // ICP_TC) == set(range(n_chunks))
        got = icp.align(src, tgt)
        assert same_result(got, want), (n_tgt, n_src)
        assert (got["state"], got["iterations"]) == ((5, 0) if n_src < 3 else (1, 1)) and got["n_correspondences"] == n_src
    icp.close()


def cube_scene():
    """(700 source points, 8193 target points): uniform in a 20 m cube, the sources beside target points, turned and noisy"""
    rng = np.random.default_rng(41)
    t = rng.uniform(0.0, 20.0, (GRID_MIN + 1, 3))
    pick = rng.permutation(GRID_MIN - 1)[:700]
    pick[:2] = GRID_MIN - 1, GRID_MIN                        # the two records at the threshold are somebody's neighbour
    c = np.array([10.0, 10.0, 10.0])
    s = (t[pick] - c) @ rot([0.2, -0.3, 1.0], 0.03).T + c + np.array([0.15, -0.1, 0.05]) + rng.normal(0.0, 0.05, (700, 3))
    return cloud(s), cloud(t)


@pytest.fixture(scope="module")
def cube():
    return cube_scene()


def test_grid_threshold(S, P, cube):
    src, tgt = cube
    seen = []
    for n_tgt in (GRID_MIN - 1, GRID_MIN, GRID_MIN + 1):      # dense only below 4 * ICP_TC, the cell grid from there on
        want = P.align(src, tgt[:n_tgt], max_iterations=6)
        assert want["iterations"] >= 3 and want["n_correspondences"] == 700
        for search in (1, 0):
            assert same_result(device(S, src, tgt[:n_tgt], search=search, max_iterations=6), want), (n_tgt, search)
        seen.append(want["T"])
    assert not np.array_equal(seen[0], seen[2])               # the two records at the threshold take part


def sparse_scene():
    """8192 uniform target points in a 64 m cube (the grid's cells grow to 1.1 m: 64 / 1.0 + 2 cells a side do not fit 2^18), 1000
    queries uniform in the same cube and 24 placed 10 m outside it"""
    rng = np.random.default_rng(7)
    t = rng.uniform(0.0, 64.0, (GRID_MIN, 3))
    q = rng.uniform(0.0, 64.0, (1000, 3))
    out = rng.uniform(0.0, 64.0, (24, 3))
    out[np.arange(24), np.arange(24) % 3] = np.where(np.arange(24) % 2 == 0, -10.0, 74.0)
    return cloud(np.concatenate([q, out])[rng.permutation(1024)]), cloud(t)


@pytest.fixture(scope="module")
def sparse():
    return sparse_scene()


@pytest.mark.parametrize("iters", [1, 5])
def test_sparse_target_rings_and_unresolved_list(S, P, sparse, iters):
    src, tgt = sparse
    # the premise, before the GPU is touched: ring 1 settles below 0.95 * 1.1 m, ring 2 below 1.95 * 1.1 m, ring 3 below 2.95 * 1.1 m
    # (3.245 m), and what lies beyond goes through the unresolved list to the dense sweep
    d = np.sqrt(first_sweep(src, tgt)[0].astype(np.float64))
    counts = [int(((d >= a) & (d < b)).sum()) for a, b in ((0.0, 1.0), (1.2, 2.0), (2.3, 3.0), (3.6, np.inf))]
    print("sparse scene: queries in [0, 1), [1.2, 2), [2.3, 3), beyond 3.6 m:", counts)
    assert counts[0] >= 20 and counts[1] >= 20 and counts[2] >= 20 and counts[3] >= 5 + 24
    want = P.align(src, tgt, max_iterations=iters)
    assert want["iterations"] == iters and want["n_correspondences"] == 1024
    for search in (1, 0):
        assert same_result(device(S, src, tgt, search=search, max_iterations=iters), want), search


def lattice_scene():
    """(500 queries, the 21 x 21 x 19 integer lattice in shuffled order): with the grid's 1 m cells every target point sits on a cell
    boundary; 300 queries at cell centres (eight target points at d^2 = 0.75, in eight cells) and 200 at face centres (four at 0.5)"""
    rng = np.random.default_rng(53)
    g = np.stack([m.reshape(-1) for m in np.meshgrid(np.arange(21), np.arange(21), np.arange(19), indexing="ij")], 1).astype(np.float64)
    tgt = cloud(g[rng.permutation(g.shape[0])])
    centre = np.stack([rng.integers(0, 20, 300), rng.integers(0, 20, 300), rng.integers(0, 18, 300)], 1) + 0.5
    face = np.stack([rng.integers(0, 20, 200) + 0.5, rng.integers(0, 20, 200) + 0.5, rng.integers(0, 19, 200)], 1)
    return cloud(np.concatenate([centre, face])), tgt


@pytest.mark.parametrize("n_tgt", [8379, 4500])
def test_equal_distances_resolve_to_the_lowest_index(S, P, n_tgt):
    """8379: the cell grid, ties across cells (and across chunks in the dense mode).  4500: dense only, ties across the chunks."""
    src, tgt = lattice_scene()
    assert tgt.shape[0] == 8379 >= GRID_MIN
    tgt = tgt[:n_tgt]
    d = f32_d2(src, tgt)
    tied = d == d.min(1)[:, None]
    if n_tgt == 8379:
        assert (tied[:300].sum(1) == 8).all() and (d.min(1)[:300] == 0.75).all() and (tied[300:].sum(1) == 4).all()
    chunk = np.arange(n_tgt) // ICP_TC
    spans = np.array([np.unique(chunk[row]).size for row in tied])
    assert (spans >= 2).sum() >= 200                          # equal keys' distances meet in the atomicMin across chunks
    assert np.array_equal(first_sweep(src, tgt)[1], tied.argmax(1))
    rev = np.ascontiguousarray(tgt[::-1])
    for iters in (1, 3):
        want, want_rev = P.align(src, tgt, max_iterations=iters), P.align(src, rev, max_iterations=iters)
        assert not np.array_equal(want["T"], want_rev["T"])   # it is the index that decides
        for search in (1, 0):
            assert same_result(device(S, src, tgt, search=search, max_iterations=iters), want), (search, iters)
            assert same_result(device(S, src, rev, search=search, max_iterations=iters), want_rev), (search, iters)


def odd_targets(n):
    rng = np.random.default_rng(61)
    base = rng.uniform(-12.0, 12.0, (n, 3)) * np.array([1.0, 1.0, 0.25])
    flat = base.copy()
    flat[:, 2] = 1.5
    same = np.tile(np.array([[1.0, 2.0, 3.0]]), (n, 1))
    dup = np.concatenate([base[:n - 500], base[:500]])
    junk = base.copy()
    junk[[5, n // 2, n - 1]] = [[np.nan, 1.0, 2.0], [5000.0, -3000.0, 40.0], [1.0, np.inf, 2.0]]
    pick = rng.permutation(n - 500)[:600]
    src = base[pick] @ rot([0.0, 0.1, 1.0], 0.02).T + np.array([0.1, 0.05, -0.05]) + rng.normal(0.0, 0.03, (600, 3))
    src[77] = [np.nan, 0.0, 0.0]                             # a source point without a neighbour
    return cloud(src), dict(flat=cloud(flat), identical=cloud(same), duplicated=cloud(dup), nan_and_outlier=cloud(junk))


@pytest.mark.parametrize("n_tgt", [3000, 8400])
@pytest.mark.parametrize("kind", ["flat", "identical", "duplicated", "nan_and_outlier"])
def test_odd_records(S, P, kind, n_tgt):
    src, targets = odd_targets(n_tgt)
    tgt = targets[kind]
    if kind == "identical":                                  # every target point is every query's candidate: fewer queries
        src = src[:120]
    want = P.align(src, tgt, max_iterations=3)
    assert want["n_correspondences"] == src.shape[0] - 1 and want["iterations"] >= 1
    for search in ((1, 0) if n_tgt >= GRID_MIN else (1,)):
        assert same_result(device(S, src, tgt, search=search, max_iterations=3), want), search


@pytest.mark.parametrize("side", [12, 92])
def test_cap_keeps_equality(S, P, side):
    """a z = 0 lattice (92 x 92: the cell grid) and sources exactly 0.5 m above target points: d^2 = 0.25 in f32 without rounding"""
    g = np.stack([m.reshape(-1) for m in np.meshgrid(np.arange(side), np.arange(side), indexing="ij")], 1).astype(np.float64)
    tgt = cloud(np.concatenate([g, np.zeros((g.shape[0], 1))], 1))
    src = tgt[(np.arange(100) * 37) % tgt.shape[0]].copy()
    src[:, 2] = 0.5
    assert (first_sweep(src, tgt)[0] == np.float32(0.25)).all() and (side * side >= GRID_MIN) == (side == 92)
    for cap, n in ((0.5, 100), (0.4999, 0)):
        want = P.align(src, tgt, max_corr_dist=cap, max_iterations=1)
        assert want["n_correspondences"] == n and want["state"] == (1 if n else 5) and want["fitness"] < DBL_MAX
        for search in (1, 0):
            assert same_result(device(S, src, tgt, search=search, max_corr_dist=cap, max_iterations=1), want), (cap, search)
    assert same_result(device(S, src, tgt, max_corr_dist=0.5), P.align(src, tgt, max_corr_dist=0.5))


def test_cap_leaving_three_and_two_correspondences(S, P):
    src, tgt = few_scene(3)
    want = P.align(src, tgt, max_corr_dist=1.0, max_iterations=1)
    assert want["n_correspondences"] == 3 and want["state"] == 1
    assert same_result(device(S, src, tgt, max_corr_dist=1.0, max_iterations=1), want)
    assert same_result(device(S, src, tgt, max_corr_dist=1.0), P.align(src, tgt, max_corr_dist=1.0))
    src, tgt = few_scene(2)
    got = device(S, src, tgt, max_corr_dist=1.0)
    assert same_result(got, P.align(src, tgt, max_corr_dist=1.0))
    assert got["state"] == 5 and got["n_correspondences"] == 2 and not got["converged"] and got["iterations"] == 0
    assert np.array_equal(got["T"], np.eye(4)) and 0.0 < got["fitness"] < DBL_MAX


@pytest.mark.parametrize("name", list(STATE_CASES))
def test_whole_alignment_in_every_state(S, P, name):
    scene, kw, state, iterations = STATE_CASES[name]
    src, tgt = scene()
    got = device(S, src, tgt, **kw)
    assert same_result(got, P.align(src, tgt, **kw))
    assert (got["state"], got["iterations"], got["converged"]) == (state, iterations, True)


def test_guess_and_device_pointers(S, P, cube):
    import torch
    G = rigid([0.2, 1.0, -0.4], 0.1, [0.3, -0.1, 0.05]).astype(np.float32)
    tgt, _, noisy = blob_scene()
    for src, t in ((noisy, tgt), cube):                      # dense only, and the cell grid
        want, plain = P.align(src, t, guess=G, max_iterations=8), P.align(src, t, max_iterations=8)
        assert not np.array_equal(want["T"], plain["T"]) and want["iterations"] >= 2
        icp = ctx(S, max_iterations=8)
        assert same_result(icp.align(src, t, G), want) and same_result(icp.align(src, t), plain)
        assert same_result(icp.align(src, t, np.eye(4)), plain)
        d_src, d_tgt = (torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in (src, t))
        assert same_result(icp.align_device(d_src.data_ptr(), src.shape[0], d_tgt.data_ptr(), t.shape[0]), plain)
        assert same_result(icp.align_device(d_src.data_ptr(), src.shape[0], d_tgt.data_ptr(), t.shape[0], G), want)
        assert np.array_equal(d_src.cpu().numpy(), src) and np.array_equal(d_tgt.cpu().numpy(), t)   # the caller's clouds are read only
        bad = np.eye(4, dtype=np.float32)
        bad[3, 3] = 2.0
        with pytest.raises(S.ScalError) as e:
            icp.align(src, t, bad)
        assert e.value.code == S.E_ARG
        icp.close()


def test_one_context_many_calls(S, P, cube):
    src, tgt = cube
    small = tgt[[10, 2000, 7000]]
    calls = [(src, tgt, 1), (src, small, 1), (src[:2], tgt, 1), (src, tgt, 0), (src[:300], tgt[:5000], 1), (src, tgt, 1)]
    want = [P.align(s, t, max_iterations=4) for s, t, _ in calls]
    assert [w["state"] for w in want] == [1, 1, 5, 1, 1, 1] and want[1]["n_correspondences"] == 700
    icp = ctx(S, max_iterations=4)
    for k, (s, t, search) in enumerate(calls):
        icp.set_search(search)
        got = icp.align(s, t)
        assert same_result(got, want[k]), k
        assert same_result(device(S, s, t, search=search, max_iterations=4), want[k]), k     # a fresh context gives the same
    icp.close()
