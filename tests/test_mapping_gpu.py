"""Stage C parity: scan-to-map on the HIP path vs the oracle, fed the same stage-A/B outputs scan by scan.

Bar: poses within 1e-5 (north_star).  Observed differences are ~1e-12 per step because every f32 quantity that
feeds a gate (kNN distances, voxel centroids, associated points) is bit-identical and only the order of the f64
normal-equation reduction differs from Ceres' sequential sum; the test asserts 1e-7 to leave room for that.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _sorted_rows(a):
    a = np.ascontiguousarray(a, np.float32)
    v = a.view(np.uint32).reshape(-1, 4)
    order = np.lexsort((v[:, 3], v[:, 2], v[:, 1], v[:, 0]))
    return v[order]


@pytest.fixture(scope="module")
def stage_ab(O, hdl64_stream):
    """Oracle stage A + B outputs for the first scans (inputs of stage C for both implementations)."""
    od = O.Odometry()
    out = []
    for k in range(10):
        f = O.features(hdl64_stream(k), O.HDL64, 5.0)
        c = f["cloud"]
        qlc, tlc, qw, tw, st = od.step(c[f["sharp"]], c[f["less_sharp"]], c[f["flat"]], f["less_flat"])
        out.append(dict(corner=c[f["less_sharp"]].copy(), surf=f["less_flat"].copy(), full=c.copy(), q=qw.copy(), t=tw.copy()))
    return out


def test_stream_parity(O, S, stage_ab):
    om = O.Mapper(0.4, 0.8, voxel_order=1, knn_mode=0)
    gm = S.LaserMapping(0.4, 0.8, max_scan_points=200000, max_map_points=2000000)
    worst = 0.0
    slack = dict(registered=0, map=0)
    for k, fr in enumerate(stage_ab):
        qo, to, so, rego = om.step(fr["corner"], fr["surf"], fr["full"], fr["q"], fr["t"], want_registered=True)
        qg, tg, sg, regg = gm.process(fr["corner"], fr["surf"], fr["full"], fr["q"], fr["t"], want_registered=True)
        assert sg.n_corner_stack == so.n_corner_stack and sg.n_surf_stack == so.n_surf_stack, k
        assert sg.n_corner_map == so.n_corner_map and sg.n_surf_map == so.n_surf_map, k
        assert sg.solved == so.solved
        assert list(sg.n_edge) == list(so.n_edge) and list(sg.n_plane) == list(so.n_plane), (k, list(sg.n_edge), list(so.n_edge), list(sg.n_plane), list(so.n_plane))
        assert list(sg.lm_iters) == list(so.lm_iters) and list(sg.lm_success) == list(so.lm_success), k
        for o in range(2):
            assert abs(sg.cost_init[o] - so.cost_init[o]) <= 1e-9 * max(1.0, so.cost_init[o])
            assert abs(sg.cost_final[o] - so.cost_final[o]) <= 1e-9 * max(1.0, so.cost_final[o])
        d = max(np.abs(qg - qo).max(), np.abs(tg - to).max())
        worst = max(worst, d)
        assert d <= 1e-7, (k, d)
        # registered full-resolution cloud (:845-849): f32 results of an f64 transform
        nbad = (regg.view(np.uint32) != rego.view(np.uint32)).any(axis=1).sum()
        slack["registered"] = max(slack["registered"], int(nbad))
        assert nbad == 0, (k, nbad)   # measured: 0 on every scan (round 2 allowed max(5, n / 10000) without need)
        # map content of the 5x5x3 window (laserCloudCornerFromMap / SurfFromMap for the next scan): same point set
        for which in (0, 1):
            mo = _sorted_rows(om.export(which))
            mg = _sorted_rows(gm.export(which))
            assert mo.shape == mg.shape, (k, which, mo.shape, mg.shape)
            nb = (mo != mg).any(axis=1).sum()
            slack["map"] = max(slack["map"], int(nb))
            assert nb == 0, (k, which, nb, mo.shape[0])   # bit-identical point sets (round 2 allowed max(3, n / 5000))
        qa, ta = om.wmap_wodom()
        qb, tb = gm.wmap_wodom()
        assert np.abs(qa - qb).max() <= 1e-7 and np.abs(ta - tb).max() <= 1e-7
    print("worst pose difference over the stream:", worst, "rows that differ from the oracle (max over scans):", slack)
    gm.close()


def test_first_scan_and_small_map(O, S, stage_ab):
    """Map too small (:555, :731-734): no solve, the prior pose is returned and the scan is still inserted."""
    om = O.Mapper(0.4, 0.8)
    gm = S.LaserMapping(0.4, 0.8, max_scan_points=200000, max_map_points=1000000)
    fr = stage_ab[0]
    qo, to, so, _ = om.step(fr["corner"], fr["surf"], None, fr["q"], fr["t"])
    qg, tg, sg, _ = gm.process(fr["corner"], fr["surf"], None, fr["q"], fr["t"])
    assert so.solved == 0 and sg.solved == 0
    assert np.array_equal(qo, qg) and np.array_equal(to, tg)
    assert sg.n_map_corner_total > 0 and sg.n_map_surf_total > 0
    # empty inputs are legal
    qg, tg, sg, _ = gm.process(np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32), None, fr["q"], fr["t"])
    assert sg.n_corner_stack == 0 and sg.n_surf_stack == 0
    gm.close()


def test_window_roll(O, S, stage_ab):
    """Drive the pose across cube boundaries so the 21x21x11 window rolls (:324-508) and slabs are dropped."""
    om = O.Mapper(0.4, 0.8)
    gm = S.LaserMapping(0.4, 0.8, max_scan_points=200000, max_map_points=2000000)
    fr = stage_ab[1]
    q = np.array([0.0, 0.0, 0.0, 1.0])
    for step, tx in enumerate([0.0, 180.0, 420.0, 480.0, -300.0, -620.0, 0.0]):
        t = np.array([tx, 0.3 * tx, -0.1 * tx])
        qo, to, so, _ = om.step(fr["corner"], fr["surf"], None, q, t)
        qg, tg, sg, _ = gm.process(fr["corner"], fr["surf"], None, q, t)
        assert sg.n_corner_map == so.n_corner_map and sg.n_surf_map == so.n_surf_map, step
        assert max(np.abs(qg - qo).max(), np.abs(tg - to).max()) <= 1e-7, step
        for which in (0, 1):
            mo, mg = _sorted_rows(om.export(which)), _sorted_rows(gm.export(which))
            assert mo.shape == mg.shape, (step, which)
            # /laser_cloud_map: every cube of the 21x21x11 grid (laserMapping.cpp:824-837), incl. the cubes outside the 5x5x3 window
            ao, ag = _sorted_rows(om.export_all(which)), _sorted_rows(gm.export_all(which))
            assert ao.shape == ag.shape and ao.shape[0] >= mo.shape[0] and np.array_equal(ao, ag), (step, which, ao.shape, ag.shape)
    gm.close()


def test_merge_insert_equals_full_sort(S, stage_ab):
    """The map insertion (:738-802) has two device paths: a full sort of the map pool and, while the cube window stays put, a
    merge of the scan's sorted points into the already sorted map.  Both must give the same map, bit for bit, hence the same poses."""
    a = S.LaserMapping(0.4, 0.8, max_scan_points=200000, max_map_points=2000000)
    b = S.LaserMapping(0.4, 0.8, max_scan_points=200000, max_map_points=2000000)
    b.set_merge_insert(False)
    used = 0
    frames = list(stage_ab) + [stage_ab[-1], stage_ab[-1]]  # a repeated scan: every new voxel run joins an old point
    for k, fr in enumerate(frames):
        qa, ta, sa, _ = a.process(fr["corner"], fr["surf"], None, fr["q"], fr["t"])
        qb, tb, sb, _ = b.process(fr["corner"], fr["surf"], None, fr["q"], fr["t"])
        assert sb.insert_path == 0
        used += sa.insert_path
        assert np.array_equal(qa, qb) and np.array_equal(ta, tb), k
        assert sa.n_map_corner_total == sb.n_map_corner_total and sa.n_map_surf_total == sb.n_map_surf_total, k
        for which in (0, 1):
            ma, mb = _sorted_rows(a.export(which)), _sorted_rows(b.export(which))  # export order is not defined
            assert ma.shape == mb.shape and np.array_equal(ma, mb), (k, which)
    assert used >= len(frames) - 3, used  # first scan and window moves take the full sort
    a.close(), b.close()


def test_full_grid_cell_falls_back_to_the_general_build(S, hdl64_stream):
    """Queued steps bin the map into fixed slices per 1 m cell in one launch (27 corner / 8 surf entries: one per filter voxel that
    can intersect the cell).  A cell that would overflow stops the chain and the step is redone with the general three-launch
    build.  Forced here by lowering the slices to 1 entry: every queued step overflows, is redone, and nothing may change -
    poses, maps, composition - against a mapper that never uses the shortcut."""
    n = 6
    regs = [S.ScanRegistration(S.HDL64, 5.0, max_points=200000) for _ in range(3)]
    od = S.LaserOdometry(max_points=200000)
    mk = lambda: S.LaserMapping(0.4, 0.8, max_scan_points=200000, max_map_points=3000000)
    a, g = mk(), mk()
    a.debug_set_grid_cap(1, 1)
    g.set_merge_insert(False)
    for k in range(n):
        r = regs[k % len(regs)]
        r.laserCloudHandler(hdl64_stream(k))
        _, _, qw, tw, _ = od.step_features(r)
        qa, ta, sa = a.process_features(r, qw, tw)
        qg, tg, sg = g.process_features(r, qw, tw)
        assert np.array_equal(qa, qg) and np.array_equal(ta, tg), k
        assert sa.n_corner_map == sg.n_corner_map and sa.n_surf_map == sg.n_surf_map
    ca = a.path_counters()
    assert ca[2] == n - 1, ca    # every queued step met a full cell and was redone from its start
    a.debug_set_grid_cap(27, 8)  # back to the real slices: the shortcut holds on this data
    for k in range(n, n + 4):
        r = regs[k % len(regs)]
        r.laserCloudHandler(hdl64_stream(k))
        _, _, qw, tw, _ = od.step_features(r)
        qa, ta, sa = a.process_features(r, qw, tw)
        qg, tg, sg = g.process_features(r, qw, tw)
        assert np.array_equal(qa, qg) and np.array_equal(ta, tg), k
    assert a.path_counters()[2] == n - 1, a.path_counters()
    for which in (0, 1):
        ma, mg = _sorted_rows(a.export(which)), _sorted_rows(g.export(which))
        assert ma.shape == mg.shape and np.array_equal(ma, mg), which
    a.close(), g.close()


@pytest.mark.parametrize("plane_res", [0.8, 0.25])
def test_queued_steps_equal_general_path(S, hdl64_stream, plane_res):
    """Steps queued behind each other (pose composition, window decision and map sizes stay on the device; nothing is read back
    between them) against one synchronous step at a time and against the general path with the full-sort insertion.  The odometry
    poses jump across a cube boundary twice, so a queued step meets a moved window: the device stops the speculative chain, the
    host redoes that step on the general path and replays the ones queued behind it.  plane_res 0.25 gives more than 8192 stack
    points per scan: every merge insert gives up and every insertion is redone with the full sort.  All three must agree bit for bit."""
    n, depth = 14, 3
    regs = [S.ScanRegistration(S.HDL64, 5.0, max_points=200000) for _ in range(depth + 2)]
    od = S.LaserOdometry(max_points=200000)
    mk = lambda: S.LaserMapping(0.4, plane_res, max_scan_points=200000, max_map_points=3000000)
    a, b, g = mk(), mk(), mk()
    g.set_merge_insert(False)
    b.set_poll(False)   # a stopped chain is noticed by collect only: the steps queued behind it meanwhile must be replayed
    poses_a, poses_b, poses_g, paths = [], [], [], []
    inflight = []
    for k in range(n):
        r = regs[k % len(regs)]
        r.laserCloudHandler(hdl64_stream(k))
        qlc, tlc, qw, tw, _ = od.step_features(r)
        tw = tw + np.array([30.0 if 6 <= k < 10 else 0.0, 0.0, 0.0])
        qa, ta, sa = a.process_features(r, qw, tw)
        qg, tg, sg = g.process_features(r, qw, tw)
        assert sg.insert_path == 0
        paths.append(sa.insert_path)
        poses_a.append(np.concatenate([qa, ta])), poses_g.append(np.concatenate([qg, tg]))
        b.enqueue_features(r, qw, tw)
        inflight.append(k)
        if len(inflight) == depth:
            qb, tb, sb = b.collect()
            poses_b.append(np.concatenate([qb, tb]))
            inflight.pop(0)
    while inflight:
        qb, tb, sb = b.collect()
        poses_b.append(np.concatenate([qb, tb]))
        inflight.pop(0)
    b.finish()
    for k in range(n):
        assert np.array_equal(poses_a[k], poses_g[k]), (k, np.abs(poses_a[k] - poses_g[k]).max())
        assert np.array_equal(poses_b[k], poses_g[k]), (k, np.abs(poses_b[k] - poses_g[k]).max())
    for which in (0, 1):
        ma, mb, mg = _sorted_rows(a.export(which)), _sorted_rows(b.export(which)), _sorted_rows(g.export(which))
        assert ma.shape == mg.shape and np.array_equal(ma, mg), which
        assert mb.shape == mg.shape and np.array_equal(mb, mg), which
    qa_, ta_ = a.wmap_wodom()
    qb_, tb_ = b.wmap_wodom()
    qg_, tg_ = g.wmap_wodom()
    assert np.array_equal(qa_, qg_) and np.array_equal(ta_, tg_) and np.array_equal(qb_, qg_) and np.array_equal(tb_, tg_)
    ca, cb, cg = a.path_counters(), b.path_counters(), g.path_counters()
    print("path counters (speculative, general, redone after a window move, insertion redone):", ca, cb, cg)
    assert cg[0] == 0 and cg[1] == n
    if plane_res == 0.8:
        assert sum(paths) >= n - 4, paths   # first scan and the two window moves take the full sort
        assert ca[2] == 2 and cb[2] >= 2 and ca[3] == 0 and cb[3] == 0, (ca, cb)
        assert cb[0] > n, cb                # steps queued behind a stopped one were replayed
    else:
        assert sum(paths) == 0, paths       # too many new points for the merge: always redone with the full sort
        assert ca[3] >= n - 4 and cb[3] >= n - 4, (ca, cb)
    for m in (a, b, g):
        m.close()


def test_insertion_redo_after_the_features_context_was_rerun(S, hdl64_stream):
    """A speculative step whose merge gives up (plane_res 0.25: more stack points than one merge takes) stops the chain AFTER its
    pose has been published.  collect does not poll, so the caller gets the pose, reruns the step's features context with the next
    scan - allowed once the pose is collected (include/scaloam_hip.h) - and only then does finish notice the stop and redo the
    insertion with the full sort.  That redo must not need the context: finish succeeds, and the map and the next scan's pose equal,
    bit for bit, those of a context driven one synchronous step at a time."""
    n0 = 4
    regs = [S.ScanRegistration(S.HDL64, 5.0, max_points=200000) for _ in range(2)]
    od = S.LaserOdometry(max_points=200000)
    mk = lambda: S.LaserMapping(0.4, 0.25, max_scan_points=200000, max_map_points=3000000)
    a, b = mk(), mk()
    b.set_poll(False)
    for k in range(n0):   # the first scan takes the general path, the rest are queued speculatively (and redone synchronously)
        r = regs[k % 2]
        r.laserCloudHandler(hdl64_stream(k))
        _, _, qw, tw, _ = od.step_features(r)
        qa, ta, _ = a.process_features(r, qw, tw)
        qb, tb, _ = b.process_features(r, qw, tw)
        assert np.array_equal(qa, qb) and np.array_equal(ta, tb), k
    before = b.path_counters()
    assert before[0] >= 1, before
    x = regs[n0 % 2]
    x.laserCloudHandler(hdl64_stream(n0))
    _, _, qw, tw, _ = od.step_features(x)
    qa, ta, _ = a.process_features(x, qw, tw)
    b.enqueue_features(x, qw, tw)
    qb, tb, _ = b.collect()                      # the pose stands; the stop of the merge has not been noticed yet
    assert np.array_equal(qa, qb) and np.array_equal(ta, tb)
    x.laserCloudHandler(hdl64_stream(n0 + 1))    # the context is rerun before the insertion is redone
    b.finish()
    after = b.path_counters()
    assert after[3] == before[3] + 1 and after[0] == before[0] + 1, (before, after)   # this step's insertion was redone
    for which in (0, 1):
        assert np.array_equal(_sorted_rows(a.export(which)), _sorted_rows(b.export(which))), which
    _, _, qw, tw, _ = od.step_features(x)
    qa, ta, _ = a.process_features(x, qw, tw)
    qb, tb, _ = b.process_features(x, qw, tw)
    assert np.array_equal(qa, qb) and np.array_equal(ta, tb)
    for which in (0, 1):
        assert np.array_equal(_sorted_rows(a.export(which)), _sorted_rows(b.export(which))), which
    for m in regs + [od, a, b]:
        m.close()


def test_long_stream_parity_device_pipeline(O, S, hdl64_stream):
    """50 scans of the BASELINE config #2 sequence (seed 205) through the device-resident pipeline A -> B -> C (features context handed
    from stage to stage, stage C on its speculative chain) against the oracle chain.  Long enough for the trajectory (1 m per scan)
    to change the centre cube of the map window in-stream, so the merge insert, its full-sort fallback and a real window change
    (chain stopped on the device, step redone on the general path) all meet the oracle.  Poses within 1e-6, residual-block
    counts and LM iterations equal at every scan, the final maps hold the same points."""
    n = 50
    reg = S.ScanRegistration(S.HDL64, 5.0, max_points=200000)
    od = S.LaserOdometry(max_points=200000)
    gm = S.LaserMapping(0.4, 0.8, max_scan_points=200000, max_map_points=3000000)
    oo, om = O.Odometry(), O.Mapper(0.4, 0.8, voxel_order=1, knn_mode=0)
    worst, paths = 0.0, []
    for k in range(n):
        xyz = hdl64_stream(k)
        reg.laserCloudHandler(xyz)
        qlc, tlc, qw, tw, _ = od.step_features(reg)
        qg, tg, sg = gm.process_features(reg, qw, tw)
        f = O.features(xyz, O.HDL64, 5.0)
        c = f["cloud"]
        a = oo.step(c[f["sharp"]], c[f["less_sharp"]], c[f["flat"]], f["less_flat"])
        qo, to, so, _ = om.step(c[f["less_sharp"]], f["less_flat"], c, a[2], a[3])
        assert sg.solved == so.solved and list(sg.n_edge) == list(so.n_edge) and list(sg.n_plane) == list(so.n_plane), (k, list(sg.n_plane), list(so.n_plane))
        assert list(sg.lm_iters) == list(so.lm_iters) and list(sg.lm_success) == list(so.lm_success), k
        assert sg.n_corner_map == so.n_corner_map and sg.n_surf_map == so.n_surf_map, k
        d = max(np.abs(qg - qo).max(), np.abs(tg - to).max())
        worst = max(worst, d)
        assert d <= 1e-6, (k, d)
        paths.append(sg.insert_path)
    cnt = gm.path_counters()
    print("worst pose difference over 50 scans:", worst, "insert paths:", paths, "path counters:", cnt)
    assert cnt[2] >= 1, cnt            # the centre cube changed at least once: a speculative step was redone on the general path
    assert sum(paths) >= n - 6, paths   # everything else went through the merge insert
    for which in (0, 1):
        mo, mg = _sorted_rows(om.export(which)), _sorted_rows(gm.export(which))
        assert mo.shape == mg.shape, (which, mo.shape, mg.shape)
        print("map rows that differ from the oracle, class", which, ":", int((mo != mg).any(axis=1).sum()), "of", mo.shape[0])
        assert np.array_equal(mo, mg), which   # 0 of 51,865 / 29,236 rows differ after 50 scans
    for x in (reg, od, gm):
        x.close()


def test_fine_filters_queued_chain_without_fixed_pools(O, S, worlds):
    """Filters of 0.2 / 0.4 m (the mulran launch values) on a VLP-16 stream - __graft_entry__.smoke()'s configuration, longer: 216 + 27
    voxels can meet a 1 m cell, more than the fixed-slice pools of the one-launch grid are built for, so the queued chain keeps the
    three general grid launches and computes the merge insert's old keys in a launch of its own (k_merge_okeys).  Round 3 lost that
    launch for a few commits - every other stream in this file runs at 0.4 / 0.8 m and did not notice; smoke() did.  Poses, block counts
    and map sizes follow the oracle, the maps hold the same points, and the steps do go through the merge insert."""
    n = 8
    w = worlds(O.VLP16, 101)
    reg = S.ScanRegistration(S.VLP16, 0.1, max_points=60000)
    od = S.LaserOdometry(max_points=60000)
    gm = S.LaserMapping(0.2, 0.4, max_scan_points=60000, max_map_points=600000)
    oo, om = O.Odometry(), O.Mapper(0.2, 0.4, voxel_order=1, knn_mode=0)
    paths = []
    for k in range(n):
        xyz = w.scan(k)
        reg.laserCloudHandler(xyz)
        _, _, qw, tw, _ = od.step_features(reg)
        qg, tg, sg = gm.process_features(reg, qw, tw)
        f = O.features(xyz, O.VLP16, 0.1)
        c = f["cloud"]
        a = oo.step(c[f["sharp"]], c[f["less_sharp"]], c[f["flat"]], f["less_flat"])
        qo, to, so, _ = om.step(c[f["less_sharp"]], f["less_flat"], c, a[2], a[3])
        assert sg.solved == so.solved and list(sg.n_edge) == list(so.n_edge) and list(sg.n_plane) == list(so.n_plane), (k, list(sg.n_plane), list(so.n_plane))
        assert sg.n_corner_map == so.n_corner_map and sg.n_surf_map == so.n_surf_map, k
        assert max(np.abs(qg - qo).max(), np.abs(tg - to).max()) <= 1e-6, k
        paths.append(sg.insert_path)
    assert sum(p == 1 for p in paths) >= n - 2, paths   # the first scan takes the general path; the rest merge
    for which in (0, 1):
        assert np.array_equal(_sorted_rows(om.export(which)), _sorted_rows(gm.export(which))), which
    for x in (reg, od, gm):
        x.close()


def test_degenerate_plane_fit_follows_the_reference(O, S):
    """laserMapping.cpp:664-687 with five neighbours whose sum is zero: the least-squares normal of A n = -1 is n = 0, so d = 1/0 and
    n/|n| = NaN; `fabs(NaN) > 0.2` is false, the block counts as valid and goes to the solver with NaN parameters.  Every LM step is
    then invalid and the pose comes back unchanged (Ceres would stop with "Residual and Jacobian evaluation failed").  The HIP path
    must take the same road as the oracle: same block counts, same (prior) pose."""
    rng = np.random.default_rng(3)
    star = np.array([[0.85, 0, 0], [-0.85, 0, 0], [0, 0.85, 0], [0, -0.85, 0], [0, 0, 0]], np.float32)   # sum = 0, 0.85 m apart (> the 0.8 m leaf)
    gx, gy = np.meshgrid(np.arange(8) * 1.7 + 12.0, np.arange(8) * 1.7 - 6.0)
    ground = np.stack([gx.ravel(), gy.ravel(), np.full(64, -1.7)], 1).astype(np.float32)                # 64 well separated surf points, far from the star
    surf = np.concatenate([star, ground])
    surf = np.concatenate([surf, np.zeros((surf.shape[0], 1), np.float32)], 1)
    corner = np.stack([np.full(14, 20.0), np.arange(14) * 0.9 - 6.0, np.arange(14) * 0.45], 1).astype(np.float32)
    corner = np.concatenate([corner, np.zeros((14, 1), np.float32)], 1)
    q, t = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)
    om, gm = O.Mapper(0.4, 0.8), S.LaserMapping(0.4, 0.8, max_scan_points=10000, max_map_points=100000)
    for m in (om, gm):     # first scan: map too small, inserted with the prior pose
        m.step(corner, surf, None, q, t) if m is om else m.process(corner, surf, None, q, t)
    # second scan: one surf point at the centre of the star (its five neighbours are the star), a few on the ground patch
    surf2 = np.concatenate([np.array([[0.02, -0.01, 0.0, 0.0]], np.float32), surf[5:25] + np.array([0.05, 0.02, 0.0, 0.0], np.float32)])
    qo, to, so, _ = om.step(corner, surf2, None, q, t)
    qg, tg, sg, _ = gm.process(corner, surf2, None, q, t)
    assert so.solved == 1 and sg.solved == 1
    assert list(sg.n_plane) == list(so.n_plane) and list(sg.n_edge) == list(so.n_edge), (list(sg.n_plane), list(so.n_plane))
    assert list(sg.lm_iters) == list(so.lm_iters) and list(sg.lm_success) == list(so.lm_success) == [0, 0]
    assert np.array_equal(qg, qo) and np.array_equal(tg, to) and np.array_equal(qg, q) and np.array_equal(tg, t)
    gm.close()


def test_ceres_adapter_mode(O, S, stage_ab):
    """SURVEY.md section 8b's adapter cut: the HOST owns the solver, the device prepares the scan (scal_map_adapter_begin), associates at
    the solver's current pose (scal_map_associate), hands out the residual blocks (scal_map_get_blocks) or evaluates all of them in
    one batch (scal_map_eval_blocks: residuals + ambient Jacobians, the interface of the reference's AutoDiffCostFunctions,
    lidarFactor.hpp:12-138), and inserts the scan at the solved pose (scal_map_adapter_finish).
      (1) every block's residual and 3x7 / 1x7 Jacobian equals the oracle's autodiff (Jets) evaluation of the same functor;
      (2) with the oracle's restatement of ceres::Solve as the host solver the poses equal the all-device path's."""
    a = S.LaserMapping(0.4, 0.8, max_scan_points=200000, max_map_points=2000000)   # all-device
    b = S.LaserMapping(0.4, 0.8, max_scan_points=200000, max_map_points=2000000)   # adapter mode
    checked = 0
    for k, fr in enumerate(stage_ab[:6]):
        qa, ta, sa, _ = a.process(fr["corner"], fr["surf"], fr["full"], fr["q"], fr["t"])
        q, t = b.adapter_begin(fr["corner"], fr["surf"], fr["full"], fr["q"], fr["t"])
        for outer in range(2):  # :563
            nb, nr = b.associate(q, t)
            if nb == 0:   # map too small (:555): no solve
                continue
            kind, cp, pa, pb = b.blocks()
            assert nb == sa.n_edge[outer] + sa.n_plane[outer] and nr == 3 * sa.n_edge[outer] + sa.n_plane[outer], (k, outer)
            assert (kind == 0).sum() == sa.n_edge[outer] and (kind == 2).sum() == sa.n_plane[outer]
            x7 = np.concatenate([q, t])
            r, J = b.eval_blocks(x7)
            row = 0
            for i in list(range(0, nb, max(1, nb // 150)))[:150]:   # a sample of the blocks against the autodiff oracle
                row = int(3 * (kind[:i] == 0).sum() + (kind[:i] != 0).sum())
                ro, Jo = O.factor_eval(int(kind[i]), cp[i], np.concatenate([pa[i], pb[i]]), x7)
                n_r = 3 if kind[i] == 0 else 1
                assert np.abs(r[row:row + n_r] - ro).max() <= 1e-9 * max(1.0, np.abs(ro).max()), (k, outer, i)
                assert np.abs(J[row:row + n_r] - Jo).max() <= 1e-9 * max(1.0, np.abs(Jo).max()), (k, outer, i)
                checked += 1
            x, iters, trace, term = O.ceres_solve(kind, cp, pa, pb, x7)   # the host's solver (oracle restatement of ceres::Solve)
            q, t = x[:4].copy(), x[4:].copy()
        sb, _ = b.adapter_finish(q, t)
        assert max(np.abs(q - qa).max(), np.abs(t - ta).max()) <= 1e-9, (k, np.abs(q - qa).max(), np.abs(t - ta).max())
        assert sb.n_map_corner_total == sa.n_map_corner_total and sb.n_map_surf_total == sa.n_map_surf_total, k
        qwa, twa = a.wmap_wodom()
        qwb, twb = b.wmap_wodom()
        assert np.abs(qwa - qwb).max() <= 1e-9 and np.abs(twa - twb).max() <= 1e-9
    assert checked > 500
    for which in (0, 1):
        ma, mb = _sorted_rows(a.export(which)), _sorted_rows(b.export(which))
        assert ma.shape == mb.shape and (ma != mb).any(axis=1).sum() <= 3
    with pytest.raises(S.ScalError) as e:
        b.associate(q, t)   # no open step
    assert e.value.code == S.E_STATE
    a.close(), b.close()


def test_lm_barrier_gives_up_cleanly(S, stage_ab):
    """The LM solve's exchange is a bounded wait: when a round's partial sums do not show up within the poll budget the workgroup
    gives up, raises the sticky flags (exchange + stage C's abort word), nothing of the step is committed and every kernel queued
    behind it drains as a no-op.  The host clears the exchange, rolls the map <- odometry correction back and runs the step once
    more; the second failure is reported as SCAL_E_HIP and the scan is dropped.  The budget is lowered to zero here to force that
    path (it cannot be provoked otherwise without another process hogging the GPU).  Afterwards the context must behave exactly
    like one that never saw the failure: the abandoned step left no trace in the map."""
    gm = S.LaserMapping(0.4, 0.8, max_scan_points=200000, max_map_points=2000000)
    ref = S.LaserMapping(0.4, 0.8, max_scan_points=200000, max_map_points=2000000)
    for fr in stage_ab[:3]:
        gm.process(fr["corner"], fr["surf"], None, fr["q"], fr["t"])
        ref.process(fr["corner"], fr["surf"], None, fr["q"], fr["t"])
    fr = stage_ab[3]
    try:
        gm.debug_set_lm_polls(0)   # process-global device symbol: always put back
        for _ in range(2):         # twice: the second failure starts from a context that has already been cleaned up once
            with pytest.raises(S.ScalError) as e:
                gm.process(fr["corner"], fr["surf"], None, fr["q"], fr["t"])
            assert e.value.code == S.E_HIP and "abandoned" in str(e.value)
    finally:
        gm.debug_set_lm_polls(1 << 22)
    gm.finish()
    for fr in stage_ab[3:6]:       # the same scan again, and two more: solves normally, bit-identical to the undisturbed context
        q, t, st, _ = gm.process(fr["corner"], fr["surf"], None, fr["q"], fr["t"])
        assert st.solved == 1 and st.lm_iters[0] >= 1
        q2, t2, st2, _ = ref.process(fr["corner"], fr["surf"], None, fr["q"], fr["t"])
        assert np.array_equal(q, q2) and np.array_equal(t, t2)
    for which in (0, 1):
        assert np.array_equal(_sorted_rows(gm.export(which)), _sorted_rows(ref.export(which)))
    gm.close(), ref.close()


def test_lm_give_up_on_the_queued_chain(S, hdl64_stream):
    """The same failure with steps queued speculatively behind the abandoned one (device-resident features, nothing read back
    between the steps): every queued step must come back as SCAL_E_HIP without touching the map, and the scans replayed afterwards
    must give the poses and the map of a context that never failed."""
    n0, nq = 4, 3
    regs = [S.ScanRegistration(S.HDL64, 5.0, max_points=200000) for _ in range(nq)]
    od = S.LaserOdometry(max_points=200000)
    mk = lambda: S.LaserMapping(0.4, 0.8, max_scan_points=200000, max_map_points=3000000)
    a, b = mk(), mk()
    b.set_poll(False)
    odo = []
    for k in range(n0 + nq):
        r = regs[k % nq]
        r.laserCloudHandler(hdl64_stream(k))
        _, _, qw, tw, _ = od.step_features(r)
        odo.append((qw.copy(), tw.copy()))
        if k < n0:
            a.process_features(r, qw, tw), b.process_features(r, qw, tw)
    # scans n0 .. n0+nq-1 are now in the three features contexts
    try:
        b.debug_set_lm_polls(0)
        for k in range(n0, n0 + nq):
            b.enqueue_features(regs[k % nq], *odo[k])
        for k in range(n0, n0 + nq):
            with pytest.raises(S.ScalError) as e:
                b.collect()
            assert e.value.code == S.E_HIP and "abandoned" in str(e.value), k
    finally:
        b.debug_set_lm_polls(1 << 22)
    b.finish()
    for k in range(n0, n0 + nq):
        b.enqueue_features(regs[k % nq], *odo[k])
    for k in range(n0, n0 + nq):
        qa, ta, _ = a.process_features(regs[k % nq], *odo[k])
        qb, tb, _ = b.collect()
        assert np.array_equal(qa, qb) and np.array_equal(ta, tb), k
    b.finish()
    for which in (0, 1):
        assert np.array_equal(_sorted_rows(a.export(which)), _sorted_rows(b.export(which)))
    for x in regs + [od, a, b]:
        x.close()
