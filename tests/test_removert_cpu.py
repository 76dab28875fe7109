"""scal_removert_* without a GPU: struct layouts against the header's own, the argument checks that precede the device, SCAL_E_NO_DEVICE
where there is none; and the CPU restatement (scaloam/removert.py) itself - against ground truth on the constructed scenes, its
invariants, and the margin condition on every input tests/test_removert_gpu.py compares the device with."""
import ctypes as C
import functools
import importlib.util
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@functools.lru_cache(maxsize=None)
def _inputs():
    return _tool("removert_scene").test_inputs(GOLDEN)


@functools.lru_cache(maxsize=None)
def _reference(name):
    from scaloam import removert as rv
    v = _inputs()[name]
    return rv.remove_dynamic_points(v["map"], v["scans"], v["poses"], v["remove_res"], v["revert_res"], **v["cfg"])


def _cfg(S, **kw):
    v = dict(max_points=1000, max_keyframes=4, max_scan_points=1000, max_resolutions=4, min_hits=1, device=0, fov_up_deg=25.0,
             fov_down_deg=-25.0, min_range=0.5, max_range=80.0, diff_thres=0.1, min_res_deg=0.0, cell_size=0.0)
    v.update(kw)
    return S.RemovertConfig(**v)


def test_removert_struct_layouts_match_the_header(S, tmp_path):
    fields_a = [f for f, _ in S.RemovertConfig._fields_]
    fields_b = [f for f, _ in S.RemovertStats._fields_]
    args = ["sizeof(scal_removert_config)"] + [f"offsetof(scal_removert_config, {f})" for f in fields_a]
    args += ["sizeof(scal_removert_stats)"] + [f"offsetof(scal_removert_stats, {f})" for f in fields_b]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scaloam_hip.h"\nint main(void) {\n'
                   + "".join(f'    printf("%zu ", (size_t)({a}));\n' for a in args) + '    printf("\\n");\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    A, B = S.RemovertConfig, S.RemovertStats
    assert got == [C.sizeof(A)] + [getattr(A, f).offset for f in fields_a] + [C.sizeof(B)] + [getattr(B, f).offset for f in fields_b]


def test_removert_argument_checks_and_no_device(S):
    L = S.lib()
    h = C.c_void_p()
    nan, inf = float("nan"), float("inf")
    assert L.scal_removert_create(None, C.byref(h)) == S.E_ARG
    for bad in (dict(max_points=0), dict(max_points=-5), dict(max_keyframes=0), dict(max_scan_points=0), dict(max_resolutions=0),
                dict(max_resolutions=9), dict(min_hits=0), dict(min_hits=-1), dict(fov_up_deg=-25.0), dict(fov_up_deg=-30.0),
                dict(fov_up_deg=nan), dict(fov_down_deg=nan), dict(fov_up_deg=95.0), dict(min_range=0.0), dict(min_range=-1.0),
                dict(min_range=nan), dict(max_range=0.0), dict(max_range=nan), dict(max_range=inf), dict(max_range=0.25),
                dict(diff_thres=0.0), dict(diff_thres=-0.1), dict(diff_thres=nan), dict(min_res_deg=nan), dict(min_res_deg=-1.0),
                dict(cell_size=nan), dict(cell_size=-2.0), dict(min_res_deg=1e-4)):
        cfg = _cfg(S, **bad)
        assert L.scal_removert_create(C.byref(cfg), C.byref(h)) == S.E_ARG, bad
        assert b"scal_removert_create" in L.scal_last_error()
    cfg = _cfg(S)
    assert L.scal_removert_create(C.byref(cfg), None) == S.E_ARG
    rc = L.scal_removert_create(C.byref(cfg), C.byref(h))
    if S.device_count() < 1:
        assert rc == S.E_NO_DEVICE and not h.value
        with pytest.raises(S.ScalError) as e:
            S.Removert(1000, 4, 1000)
        assert e.value.code == S.E_NO_DEVICE
    else:
        assert rc == S.OK and h.value
        L.scal_removert_destroy(h)
    # null contexts are refused before anything touches a device
    st = S.RemovertStats()
    off = np.zeros(2, np.int32)
    res = np.array([2.5])
    m = np.zeros(4, np.uint8)
    n = C.c_int(0)
    img = np.zeros(4, np.float32)
    assert L.scal_removert_set_map(None, None, 0) == S.E_ARG
    assert L.scal_removert_set_map_device(None, None, 0) == S.E_ARG
    assert L.scal_removert_run(None, None, off.ctypes.data_as(C.POINTER(C.c_int)), 0, None, res.ctypes.data_as(C.POINTER(C.c_double)), 1, None, 0,
                               m.ctypes.data_as(C.POINTER(C.c_ubyte)), None, C.byref(st)) == S.E_ARG
    assert b"scal_removert_run" in L.scal_last_error()
    assert L.scal_removert_compact(None, 0, None, 0, C.byref(n)) == S.E_ARG
    assert L.scal_removert_scan_image(None, 0, 0, img.ctypes.data_as(C.POINTER(C.c_float)), 2, 2) == S.E_ARG
    L.scal_removert_destroy(None)


def test_image_shape_rounds_like_lround(S):
    from scaloam import removert as rv
    assert rv.image_shape(2.5) == (20, 144) and rv.image_shape(2.0) == (25, 180) and rv.image_shape(5.0) == (10, 72)
    assert rv.image_shape(1.5) == (33, 240)                     # 33.33 down
    assert rv.image_shape(20.0) == (3, 18)                      # 2.5 goes away from zero, not to the even neighbour
    assert rv.image_shape(100.0) == (1, 4) and rv.image_shape(200.0) == (1, 2)   # 0.25 -> at least one row; 3.6 -> 4
    assert rv.finest((2.5, 1.5, 2.0, 1.5)) == 1


@pytest.mark.parametrize("name", ["scene_k4", "scene_k4_revert", "scene_k2", "scene_k2_revert"])
def test_restatement_finds_exactly_the_moving_object(S, name):
    """K keyframes inside a static sphere, each with a ball that stands elsewhere in every keyframe: with the default settings the mask
    is the ball returns, no more and no fewer"""
    v, r = _inputs()[name], _reference(name)
    assert v["map"].shape[0] == {"scene_k4": 288000, "scene_k2": 36000}[name[:8]]
    lab = v["labels"]
    assert lab.sum() > 50
    mask = r.mask.astype(bool)
    assert (mask & ~lab).sum() == 0 and (~mask & lab).sum() == 0
    assert r.stats["dynamic"] == lab.sum() and r.stats["pairs_bruteforce"] == lab.shape[0] * len(v["scans"])
    assert np.array_equal(r.hits, r.hits_all[2])   # 1.5 degrees is the finest of 2.5 / 2.0 / 1.5


def test_restatement_counts_on_the_golden_scans(S):
    assert _inputs()["kaist"]["map"].shape[0] == 109818
    assert _reference("kaist").stats["dynamic"] == 14437 and _reference("kaist_revert").stats["dynamic"] == 2889


def test_restatement_invariants(S):
    from scaloam import removert as rv
    v = _inputs()["scene_k2"]
    mp, scans, P = v["map"], v["scans"], v["poses"]
    base = _reference("scene_k2")
    # one keyframe never sees through its own points
    one = rv.remove_dynamic_points(mp[:18000], scans[:1], P[:1], (2.5, 2.0, 1.5), ())
    assert one.mask.sum() == 0 and one.hits_all.max() == 0
    # permuting the map permutes the mask; permuting the keyframes changes nothing
    perm = np.random.default_rng(0).permutation(mp.shape[0])
    assert np.array_equal(rv.remove_dynamic_points(mp[perm], scans, P, (2.5, 2.0, 1.5), ()).mask, base.mask[perm])
    swapped = rv.remove_dynamic_points(mp, scans[::-1], P[::-1], (2.5, 2.0, 1.5), ())
    assert np.array_equal(swapped.mask, base.mask) and np.array_equal(swapped.hits_all, base.hits_all)
    # min_hits = 2 is a subset of min_hits = 1; a revert resolution never grows the mask
    k = _inputs()["kaist"]
    two = rv.remove_dynamic_points(k["map"], k["scans"], k["poses"], (2.5, 2.0, 1.5), (), min_hits=2)
    assert 0 < two.mask.sum() < _reference("kaist").mask.sum() and not (two.mask & ~_reference("kaist").mask).any()
    assert not (_reference("kaist_revert").mask & ~_reference("kaist").mask).any()
    # outside the field of view, below min_range or beyond max_range: never dynamic.  Points on the rays of keyframe 0 that stop
    # short of its wall are hit by it; the same points pushed out of its gates are not
    d = scans[0][:2000, :3].astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    R, t = P[0].reshape(3, 4)[:, :3], P[0].reshape(3, 4)[:, 3]

    def world(local):
        return np.concatenate([local @ R.T + t, np.zeros((local.shape[0], 1))], 1).astype(np.float32)
    inside = rv.remove_dynamic_points(world(d * 5.0), scans[:1], P[:1], (2.5,), ())
    assert inside.mask.all()
    near = rv.remove_dynamic_points(world(d * 0.4), scans[:1], P[:1], (2.5,), ())
    assert near.mask.sum() == 0
    short = rv.remove_dynamic_points(world(d * 5.0), scans[:1], P[:1], (2.5,), (), max_range=4.9)
    assert short.mask.sum() == 0
    up = np.radians(40.0)
    tilt = np.stack([np.cos(up) * d[:, 0], np.cos(up) * d[:, 1], np.full(d.shape[0], np.sin(up))], 1) * 5.0
    assert rv.remove_dynamic_points(world(tilt), scans[:1], P[:1], (2.5,), ()).mask.sum() == 0
    # records that are not finite never take part
    bad = world(d[:4] * 5.0)
    bad[0, 0], bad[1, 1], bad[2, 2] = np.nan, np.inf, -np.inf
    assert list(rv.remove_dynamic_points(bad, scans[:1], P[:1], (2.5,), ()).mask) == [0, 0, 0, 1]


def test_margin_condition_on_every_gpu_input(S):
    """Device and glibc f64 atan2 differ in the last bits; a pixel index can only differ where u or v lies that close to an integer.
    This is a condition on the inputs, not a tolerance on the outputs: on every input the GPU tests use, no participating point comes
    within 1e-9 pixel of a pixel edge (1e-9 pixel of u at W = 240 is 2.6e-11 rad, five orders above the rounding of an atan2 near pi)."""
    for name in _inputs():
        assert _reference(name).margin > 1e-9, name
    assert _reference("range_edge").mask[_inputs()["range_edge"]["inside"]].all()
    assert not _reference("range_edge").mask[~_inputs()["range_edge"]["inside"]].any()


def test_replay_mapmerge_remove_dynamic(S, tmp_path):
    """tools/replay_mapmerge.py --remove-dynamic on a saved session: with a device it writes the static map beside the merged one and
    reports the counts of the restatement; without one it says so (SCAL_E_NO_DEVICE) and writes nothing"""
    import sys
    from scaloam import formats, removert as rv
    v = _inputs()["scene_k2"]
    ses = tmp_path / "session"
    (ses / "Scans").mkdir(parents=True)
    for k, s in enumerate(v["scans"]):
        formats.write_pcd_binary(str(ses / "Scans" / f"{k:06d}.pcd"), s)
    formats.write_poses(str(ses / "optimized_poses.txt"), v["poses"])
    out = tmp_path / "map.pcd"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "replay_mapmerge.py"), str(ses), "--out", str(out), "--remove-dynamic",
                        "--revert-res"], capture_output=True, text=True)
    static = tmp_path / "map_static.pcd"
    if S.device_count() < 1:
        assert r.returncode != 0 and "error -7" in r.stderr and not static.exists()
        return
    assert r.returncode == 0, r.stderr
    # the tool's poses went through optimized_poses.txt: the reference is computed from what it read
    poses = np.asarray(formats.read_poses(str(ses / "optimized_poses.txt")), np.float64).reshape(-1, 12)
    merged = formats.read_pcd(str(out))
    ref = rv.remove_dynamic_points(merged, v["scans"], poses, (2.5, 2.0, 1.5), (), keep_images=False)
    assert ref.margin > 1e-9   # the margin condition on this input: the session's poses are those of the text file
    assert f"remove-dynamic: {ref.stats['dynamic']} of {merged.shape[0]} points dynamic" in r.stdout
    kept = formats.read_pcd(str(static))
    assert kept.shape[0] == merged.shape[0] - ref.stats["dynamic"] and 0 < ref.stats["dynamic"] < 200
    assert np.array_equal(kept.view(np.uint32), merged[ref.mask == 0].view(np.uint32))
