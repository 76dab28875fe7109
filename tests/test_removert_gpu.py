"""scal_removert_* on the device against the CPU restatement (scaloam/removert.py): the mask, the hit counts and every scan range
image bit for bit, on the inputs tools/removert_scene.py names (tests/test_removert_cpu.py holds each of them to the margin
condition); the culling, the chunking, the degenerate inputs, the compaction and the device map input."""
import functools
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

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


def _ctx(S, v, **kw):
    cfg = dict(max_points=max(v["map"].shape[0], 1), max_keyframes=max(len(v["scans"]), 1),
               max_scan_points=max(sum(s.shape[0] for s in v["scans"]), 1), max_resolutions=4)
    cfg.update(v["cfg"])
    cfg.update(kw)
    return S.Removert(**cfg)


def _run(S, name, **kw):
    v = _inputs()[name]
    rm = _ctx(S, v, **kw)
    mask, stats, hits = rm.remove(v["map"], v["scans"], v["poses"], v["remove_res"], v["revert_res"], want_hits=True)
    return rm, mask, stats, hits


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


NAMES = ["scene_k4", "scene_k4_revert", "scene_k2", "scene_k2_revert", "kaist", "kaist_revert", "corridor", "far_keyframe", "range_edge"]


@pytest.mark.parametrize("name", NAMES)
def test_mask_hits_and_images_equal_the_restatement(S, name):
    v, ref = _inputs()[name], _reference(name)
    rm, mask, stats, hits = _run(S, name)
    # the scan half first: a difference here would explain one below
    for k in range(len(v["scans"])):
        for i in range(len(v["remove_res"]) + len(v["revert_res"])):
            assert _same_bits(rm.scan_image(k, i), ref.images[k][i]), (k, i)
    assert np.array_equal(hits, ref.hits)
    assert np.array_equal(mask, ref.mask)
    n, K = v["map"].shape[0], len(v["scans"])
    assert stats["points"] == n and stats["keyframes"] == K and stats["dynamic"] == int(ref.mask.sum())
    assert stats["pairs_bruteforce"] == n * K and 0 < stats["pairs_tested"] <= n * K
    if v["labels"] is not None:
        assert np.array_equal(mask.astype(bool), v["labels"])


def test_hits_at_every_resolution(S):
    """the hits output reports the finest remove resolution: run each resolution as the only one"""
    v, ref = _inputs()["kaist_revert"], _reference("kaist_revert")
    rm = _ctx(S, v)
    rm.set_map(v["map"])
    for i, res in enumerate((2.5, 2.0, 1.5, 5.0)):
        mask, _, hits = rm.run(v["scans"], v["poses"], (res,), (), want_hits=True)
        assert np.array_equal(hits, ref.hits_all[i]), res
        assert np.array_equal(mask, (ref.hits_all[i] >= 1).astype(np.uint8)), res


def test_min_hits_two(S):
    from scaloam import removert as rv
    v = _inputs()["kaist"]
    ref = rv.remove_dynamic_points(v["map"], v["scans"], v["poses"], v["remove_res"], (), min_hits=2, keep_images=False)
    mask, _ = _ctx(S, v, min_hits=2).remove(v["map"], v["scans"], v["poses"], v["remove_res"], ())
    assert np.array_equal(mask, ref.mask) and 0 < mask.sum() < _reference("kaist").mask.sum()


def test_cell_size_changes_the_work_not_the_result(S):
    """corridor: mixed-sign coordinates, 425 m long (more than four sensor ranges), 8 keyframes 20 m apart"""
    v, ref = _inputs()["corridor"], _reference("corridor")
    n, K = v["map"].shape[0], len(v["scans"])
    assert np.ptp(v["map"][:, 0]) >= 4 * 80.0 and v["map"][:, 0].min() < 0 < v["map"][:, 0].max() and v["map"][:, 1].min() < 0 < v["map"][:, 1].max()
    pairs = {}
    for cell in (0.01, 0.7, 0.0, 40.0, 5000.0):   # 0.01: more cells than the grid may have, the cells grow; 0 = max_range / 8
        _, mask, stats, hits = _run(S, "corridor", cell_size=cell)
        assert np.array_equal(mask, ref.mask) and np.array_equal(hits, ref.hits), cell
        pairs[cell] = stats["pairs_tested"]
        assert stats["pairs_tested"] <= stats["pairs_bruteforce"] == n * K
    assert pairs[0.0] < n * K and pairs[0.7] < n * K and pairs[5000.0] == n * K   # one cell lists every keyframe
    # the pairs the range gate accepts are a lower bound no culling may go below
    from scaloam import removert as rv
    accepted = sum(int(rv.View(v["map"], p, 0.5, 80.0).in_range.sum()) for p in v["poses"])
    assert all(accepted <= p for p in pairs.values())


def test_far_keyframe_contributes_nothing(S):
    _, mask, stats, hits = _run(S, "far_keyframe")
    _, mask2, stats2, hits2 = _run(S, "scene_k2")
    assert np.array_equal(mask, mask2) and np.array_equal(hits, hits2)
    assert stats["pairs_tested"] == stats2["pairs_tested"]   # no cell lists the far keyframe


def test_range_edge_points(S):
    v = _inputs()["range_edge"]
    _, mask, _, _ = _run(S, "range_edge", cell_size=0.5)
    assert np.array_equal(mask, _reference("range_edge").mask)
    assert mask[v["inside"]].all() and not mask[~v["inside"]].any()


def test_chunks_give_the_same_result(S):
    v, ref = _inputs()["scene_k4_revert"], _reference("scene_k4_revert")
    whole = _run(S, "scene_k4_revert")
    for kw in (dict(max_keyframes=2), dict(max_keyframes=3), dict(max_scan_points=100000)):   # two and two, three and one, one each
        rm, mask, stats, hits = _run(S, "scene_k4_revert", **kw)
        assert np.array_equal(mask, ref.mask) and np.array_equal(hits, ref.hits), kw
        assert stats == whole[2], kw
        # the images of the last chunk are still there, the others are gone
        assert _same_bits(rm.scan_image(3, 1), ref.images[3][1])
        with pytest.raises(S.ScalError) as e:
            rm.scan_image(0, 1)
        assert e.value.code == S.E_STATE
    with pytest.raises(S.ScalError) as e:
        _run(S, "scene_k4_revert", max_scan_points=1000)
    assert e.value.code == S.E_TOO_MANY


def test_degenerate_inputs(S):
    v = _inputs()["scene_k2"]
    mp, scans, P = v["map"], v["scans"], v["poses"]
    rm = _ctx(S, v, max_keyframes=3)
    with pytest.raises(S.ScalError) as e:
        rm.run(scans, P)
    assert e.value.code == S.E_STATE                       # no map yet
    # an empty map
    mask, stats = rm.remove(np.zeros((0, 4), np.float32), scans, P)
    assert mask.shape == (0,) and stats == dict(points=0, keyframes=2, dynamic=0, pairs_tested=0, pairs_bruteforce=0)
    assert rm.compact(0).shape == (0, 4) and rm.compact(1).shape == (0, 4)
    # no keyframe at all, and one keyframe: a scan never sees through its own points
    mask, stats = rm.remove(mp, [], np.zeros((0, 12)))
    assert mask.sum() == 0 and stats["pairs_tested"] == 0
    mask, stats, hits = rm.remove(mp[:18000], scans[:1], P[:1], want_hits=True)
    assert mask.sum() == 0 and hits.max() == 0 and stats["pairs_tested"] == 18000
    # a keyframe with zero points hits nothing: the result is that of the others
    empty = np.zeros((0, 4), np.float32)
    mask, _, hits = rm.remove(mp, [scans[0], empty, scans[1]], np.stack([P[0], P[0], P[1]]), v["remove_res"], (), want_hits=True)
    assert np.array_equal(mask, _reference("scene_k2").mask) and np.array_equal(hits, _reference("scene_k2").hits)
    assert np.isinf(rm.scan_image(1, 0)).all()
    # records that are not finite never take part and upset nothing
    bad = mp.copy()
    bad[5, 0], bad[6, 1], bad[7, 2], bad[8, :3] = np.nan, np.inf, -np.inf, np.nan
    mask, _ = rm.remove(bad, scans, P, v["remove_res"], ())
    want = _reference("scene_k2").mask.copy()
    want[5:9] = 0
    assert np.array_equal(mask, want)
    # arguments a run refuses
    for kw in (dict(remove_res=()), dict(remove_res=(2.5, 2.0, 1.5), revert_res=(5.0, 6.0)), dict(remove_res=(0.5,)), dict(remove_res=(float("nan"),)),
               dict(remove_res=(2.5,), revert_res=(400.0,))):
        with pytest.raises(S.ScalError) as e:
            rm.run(scans, P, **kw)
        assert e.value.code == S.E_ARG, kw
    with pytest.raises(S.ScalError) as e:
        rm.set_map(np.zeros((mp.shape[0] + 1, 4), np.float32))
    assert e.value.code == S.E_TOO_MANY


def test_compact_partitions_the_map_in_input_order(S):
    v, ref = _inputs()["kaist"], _reference("kaist")
    rm, mask, _, _ = _run(S, "kaist")
    keep, gone = rm.compact(0), rm.compact(1)
    assert _same_bits(keep, v["map"][mask == 0]) and _same_bits(gone, v["map"][mask == 1])
    assert keep.shape[0] + gone.shape[0] == v["map"].shape[0] and gone.shape[0] == int(ref.mask.sum())


def test_device_map_input(S):
    """the points a MapMerge holds on the device, used in place, against the same points downloaded"""
    v = _inputs()["kaist_revert"]
    mm = S.MapMerge(max_points=200000, max_frame_points=50000)
    for s, p in zip(v["scans"], v["poses"]):
        mm.add(s, p, near_thres=2.0)
    pts = mm.download()
    assert 0 < pts.shape[0] < v["map"].shape[0]            # the near points are gone
    rm = _ctx(S, v)
    mask_d, stats_d, hits_d = rm.remove_device(mm, v["scans"], v["poses"], v["remove_res"], v["revert_res"], want_hits=True)
    keep_d = rm.compact(0)
    mask_h, stats_h, hits_h = _ctx(S, v).remove(pts, v["scans"], v["poses"], v["remove_res"], v["revert_res"], want_hits=True)
    assert np.array_equal(mask_d, mask_h) and np.array_equal(hits_d, hits_h) and stats_d == stats_h and mask_d.sum() > 0
    assert _same_bits(keep_d, pts[mask_h == 0])
    from scaloam import removert as rv
    assert np.array_equal(mask_h, rv.remove_dynamic_points(pts, v["scans"], v["poses"], v["remove_res"], v["revert_res"], keep_images=False).mask)
