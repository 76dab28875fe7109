"""scal_nbr_* and scaloam/nbr.py without a GPU: the struct layout against the header's own, the argument checks that precede the
device, SCAL_E_NO_DEVICE where there is none; and the CPU restatement itself - its two candidate paths against each other on the
inputs tests/test_nbr_gpu.py compares the device with, the outlier rule on a hand-made cloud, the map diff against the constructed
scene's ground truth, and Removert's margin condition on every map diff input of the GPU tests."""
import ctypes as C
import functools
import importlib.util
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@functools.lru_cache(maxsize=None)
def _scene_tool():
    spec = importlib.util.spec_from_file_location("mapdiff_scene", os.path.join(ROOT, "tools", "mapdiff_scene.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@functools.lru_cache(maxsize=None)
def _scene():
    ms = _scene_tool()
    return ms.two_sessions(1.0, ms.SCENE_SEED)


@functools.lru_cache(maxsize=None)
def _scene_diffs():
    from scaloam import nbr
    X, Y = _scene()
    return nbr.map_diff(X["map"], Y["map"], Y["scans"], Y["poses"]), nbr.map_diff(Y["map"], X["map"], X["scans"], X["poses"])


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_nbr_struct_layout_matches_the_header(S, tmp_path):
    fields = [f for f, _ in S.NbrConfig._fields_]
    args = ["sizeof(scal_nbr_config)"] + [f"offsetof(scal_nbr_config, {f})" for f in fields]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scaloam_hip.h"\nint main(void) {\n'
                   + "".join(f'    printf("%zu ", (size_t)({a}));\n' for a in args) + '    printf("\\n");\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(S.NbrConfig)] + [getattr(S.NbrConfig, f).offset for f in fields]


def test_nbr_argument_checks_and_no_device(S):
    L = S.lib()
    h = C.c_void_p()
    assert L.scal_nbr_create(None, C.byref(h)) == S.E_ARG
    for bad in ((0, 0, 10), (0, 10, 0), (0, -1, 10), (0, 10, -3)):
        cfg = S.NbrConfig(*bad)
        assert L.scal_nbr_create(C.byref(cfg), C.byref(h)) == S.E_ARG, bad
        assert b"scal_nbr_create" in L.scal_last_error()
    cfg = S.NbrConfig(0, 100, 100)
    assert L.scal_nbr_create(C.byref(cfg), None) == S.E_ARG
    rc = L.scal_nbr_create(C.byref(cfg), C.byref(h))
    if S.device_count() < 1:
        assert rc == S.E_NO_DEVICE and not h.value
        with pytest.raises(S.ScalError) as e:
            S.RadiusIndex(100, 100)
        assert e.value.code == S.E_NO_DEVICE
    else:
        assert rc == S.OK and h.value
        L.scal_nbr_destroy(h)
    # null contexts are refused before anything touches a device
    pairs, items = C.c_longlong(0), C.c_int(0)
    assert L.scal_nbr_set_index(None, None, 0, 0.5) == S.E_ARG
    assert L.scal_nbr_set_index_device(None, None, 0, 0.5) == S.E_ARG
    assert L.scal_nbr_query(None, None, 0, None, None) == S.E_ARG
    assert L.scal_nbr_query_device(None, None, 0, None, None) == S.E_ARG
    assert L.scal_nbr_query_self(None, None, None) == S.E_ARG
    assert L.scal_nbr_stats(None, C.byref(pairs), C.byref(items)) == S.E_ARG
    L.scal_nbr_destroy(None)


def test_restatement_argument_checks(S):
    from scaloam import nbr
    p = np.zeros((3, 4), np.float32)
    for r in (0.0, -1.0, float("nan"), float("inf"), 1e-60, 1e60):   # the last two are 0 and inf as a float32
        with pytest.raises(ValueError):
            nbr.radius_counts(p, p, r)
    with pytest.raises(ValueError):
        nbr.radius_counts(p, p, 0.5, path="grid")
    with pytest.raises(ValueError):
        nbr.radius_outlier_mask(p, 0.5, -1)
    with pytest.raises(ValueError):
        nbr.update_map(p, np.zeros(2, np.uint8), p, np.zeros(3, np.uint8))
    with pytest.raises(ValueError):
        nbr.map_diff(p, p, [p], np.zeros((2, 12)))


@pytest.mark.parametrize("r", [0.5, 0.3, 0.7, 1.0, 1e-3])
def test_brute_force_equals_the_tree_path(S, r):
    from scaloam import nbr
    assert r in _scene_tool().RADII
    I, Q = _scene_tool().radius_inputs(r)
    assert I.shape[0] > 3000 and Q.shape[0] > 2000
    cb, db = nbr.radius_counts(I, Q, r, path="brute")
    ct, dt = nbr.radius_counts(I, Q, r, path="tree")
    assert cb.dtype == np.uint16 and db.dtype == np.float32
    assert np.array_equal(cb, ct) and np.array_equal(_bits(db), _bits(dt))
    assert np.array_equal(cb == 0, np.isinf(db)) and not np.isnan(db).any()
    bad = ~np.isfinite(Q[:, :3]).all(1)
    assert bad.sum() == 9 and (cb[bad] == 0).all()
    if r != 1e-3:
        assert cb.max() >= 200          # the clump
    # the self query counts the point itself
    cs, ds = nbr.radius_counts(I, I, r, path="tree")
    fin = np.isfinite(I[:, :3]).all(1)
    assert (cs[fin] >= 1).all() and (ds[fin] == 0).all() and (cs[~fin] == 0).all()


def test_pairs_at_exactly_r_count(S):
    from scaloam import nbr
    I = np.array([[0, 0, 0, 1], [0.5, 0, 0, 2], [0.5000001, 0, 0, 3], [np.nan, 0, 0, 4]], np.float32)
    c, d = nbr.radius_counts(I, I[:1], 0.5)
    assert c[0] == 2 and d[0] == 0
    c, d = nbr.radius_counts(I[1:], I[:1], 0.5)
    assert c[0] == 1 and d[0] == np.float32(0.25)
    c, d = nbr.radius_counts(I[2:], I[:1], 0.5)
    assert c[0] == 0 and np.isposinf(d[0])
    # the order of the sum: ((dx dx + dy dy) + dz dz) in f32
    q = np.array([[0.1, 0.2, 0.3, 0]], np.float32)
    dx, dy, dz = q[0, 0], q[0, 1], q[0, 2]
    c, d = nbr.radius_counts(np.zeros((1, 4), np.float32), q, 1.0)
    assert _bits(d)[0] == _bits((dx * dx + dy * dy) + dz * dz)


def test_radius_outlier_mask_on_a_hand_made_cloud(S):
    from scaloam import nbr
    cluster = np.array([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1], [0.1, 0.1, 0]], float)
    pair = np.array([[10, 0, 0], [10.2, 0, 0]], float)
    single = np.array([[-10, 5, 0]], float)
    cloud = np.concatenate([cluster, pair, single, [[np.nan, 0, 0]]], 0)
    cloud = np.concatenate([cloud, np.ones((cloud.shape[0], 1))], 1).astype(np.float32)
    count, _ = nbr.radius_counts(cloud, cloud, 0.5)
    assert list(count) == [5] * 5 + [2, 2, 1, 0]
    assert list(nbr.radius_outlier_mask(cloud, 0.5, 0)) == [True] * 8 + [False]       # the point itself is a neighbour
    assert list(nbr.radius_outlier_mask(cloud, 0.5, 1)) == [True] * 7 + [False] * 2
    assert list(nbr.radius_outlier_mask(cloud, 0.5, 2)) == [True] * 5 + [False] * 4
    assert list(nbr.radius_outlier_mask(cloud, 0.5, 4)) == [True] * 5 + [False] * 4
    assert not nbr.radius_outlier_mask(cloud, 0.5, 5).any()
    assert list(nbr.radius_outlier_mask(cloud, 0.05, 0)) == [True] * 8 + [False]


def test_map_diff_finds_exactly_the_constructed_differences(S):
    from scaloam import nbr
    ms = _scene_tool()
    X, Y = _scene()
    (lx, sx), (ly, sy) = _scene_diffs()
    assert (X["what"] == ms.OBJ_A).sum() > 30 and (X["what"] == ms.OBJ_B).sum() > 10 and (Y["what"] == ms.OBJ_C).sum() > 20
    assert np.array_equal(lx, X["labels"]) and np.array_equal(ly, Y["labels"])           # no false label in either direction
    assert sx["changed"] == (X["what"] == ms.OBJ_A).sum() and sx["unobserved"] == (X["what"] == ms.OBJ_B).sum()
    assert sy["changed"] == (Y["what"] == ms.OBJ_C).sum() and sy["unobserved"] == 0
    assert sx["common"] + sx["candidates"] == X["map"].shape[0]
    # the margin condition of tests/test_removert_cpu.py on the Removert half of every compared input
    assert sx["margin"] > 1e-9 and sy["margin"] > 1e-9
    up = nbr.update_map(X["map"], lx, Y["map"], ly)
    keep_x = X["what"] != ms.OBJ_A
    want = np.concatenate([X["map"][keep_x], Y["map"][Y["what"] == ms.OBJ_C]], 0)
    assert np.array_equal(_bits(up), _bits(want))
    # the wall and the panel once, the hidden ball, Y's ball, and not X's visible one
    assert up.shape[0] == (X["what"] == ms.STATIC).sum() + (X["what"] == ms.OBJ_B).sum() + (Y["what"] == ms.OBJ_C).sum()


def test_map_diff_margin_on_the_golden_pair(S):
    from scaloam import nbr
    gx, gy, scans, poses = _scene_tool().golden_pair(GOLDEN)
    labels, st = nbr.map_diff(gx, gy, scans, poses)
    assert st["margin"] > 1e-9
    assert gx.shape[0] == 73260 and st["common"] + st["unobserved"] + st["changed"] == gx.shape[0]
    assert 0 < st["changed"] < st["unobserved"] and st["common"] > 0
    assert (labels == 2).sum() == st["changed"]
    # a map diffed against itself is all common
    l2, s2 = nbr.map_diff(gy, gy, scans, poses)
    assert not l2.any() and s2["candidates"] == 0 and s2["margin"] == np.inf


def _write_session(formats, path, ses):
    (path / "Scans").mkdir(parents=True)
    for k, s in enumerate(ses["scans"]):
        formats.write_pcd_binary(str(path / "Scans" / f"{k:06d}.pcd"), s)
    formats.write_poses(str(path / "optimized_poses.txt"), ses["poses"])


def test_diff_sessions_and_radius_filter_tools(S, tmp_path):
    """tools/diff_sessions.py and tools/replay_mapmerge.py --radius-filter on the constructed sessions, saved as the reference saves
    a session: with a device they write what the restatement gives; without one they say so (SCAL_E_NO_DEVICE) and write nothing"""
    import sys
    from scaloam import formats, nbr
    ms = _scene_tool()
    X, Y = _scene()
    _write_session(formats, tmp_path / "old", X)
    _write_session(formats, tmp_path / "new", Y)
    out = tmp_path / "diff"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "diff_sessions.py"), str(tmp_path / "old"), str(tmp_path / "new"), "--leaf", "0",
                        "--out-dir", str(out)], capture_output=True, text=True)
    plain, filt = tmp_path / "map.pcd", tmp_path / "map_filtered.pcd"
    tool = [sys.executable, os.path.join(ROOT, "tools", "replay_mapmerge.py"), str(tmp_path / "old")]
    r1 = subprocess.run(tool + ["--out", str(plain)], capture_output=True, text=True)
    r2 = subprocess.run(tool + ["--out", str(filt), "--radius-filter", "0.5,2"], capture_output=True, text=True)
    if S.device_count() < 1:
        for q in (r, r1, r2):
            assert q.returncode != 0 and "error -7" in q.stderr
        assert not out.exists() and not plain.exists() and not filt.exists()
        return
    assert r.returncode == 0 and r1.returncode == 0 and r2.returncode == 0, (r.stderr, r1.stderr, r2.stderr)
    gone, came, up = (formats.read_pcd(str(out / f)) for f in ("diff_disappeared.pcd", "diff_appeared.pcd", "map_updated.pcd"))
    n_a, n_b, n_c = ((X["what"] == ms.OBJ_A).sum(), (X["what"] == ms.OBJ_B).sum(), (Y["what"] == ms.OBJ_C).sum())
    assert gone.shape[0] == n_a and came.shape[0] == n_c
    assert np.abs(np.linalg.norm(gone[:, :3] - ms.BALL_A[0], axis=1) - ms.BALL_A[1]).max() < 1e-3
    assert np.abs(np.linalg.norm(came[:, :3] - ms.BALL_C[0], axis=1) - ms.BALL_C[1]).max() < 1e-3
    assert up.shape[0] == (X["what"] == ms.STATIC).sum() + n_b + n_c
    merged = formats.read_pcd(str(plain))
    keep = nbr.radius_outlier_mask(merged, 0.5, 2)
    assert 0 < keep.sum() < merged.shape[0]
    assert np.array_equal(_bits(formats.read_pcd(str(filt))), _bits(merged[keep]))
