"""Ceres-adapter mode, the back end stages B and C share (csrc/lm_host.hpp), on three paths the stage tests do not reach: a block
export cut short by `cap`, an evaluation without Jacobians, and a step whose map is too small for a solve.  Three scans."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def frames(O, S, hdl64_stream):
    """Stage A (oracle) and stage B (all-device step) outputs of three scans."""
    od = S.LaserOdometry(max_points=200000)
    out = []
    for k in range(3):
        f = O.features(hdl64_stream(k), O.HDL64, 5.0)
        c = f["cloud"]
        clouds = (c[f["sharp"]], c[f["less_sharp"]], c[f["flat"]], f["less_flat"])
        _, _, qw, tw, _ = od.step(*clouds)
        out.append(dict(clouds=clouds, full=c, q=qw.copy(), t=tw.copy()))
    od.close()
    return out


def _check_open_step(ctx, q, t):
    """The two shared paths on a context whose associate() has blocks to hand out."""
    nb, nr = ctx.associate(q, t)
    assert nb > 258 and nr >= nb   # more than one workgroup of k_blocks_export / k_blocks_eval
    full = ctx.blocks()
    assert all(a.shape[0] == nb for a in full)
    for cap in (1, 257, nb - 1):
        part = ctx.blocks(cap)
        for a, b in zip(part, full):
            assert a.shape[0] == cap and np.array_equal(a.view(np.uint8), b[:cap].view(np.uint8)), cap
    for a, b in zip(ctx.blocks(nb + 7), full):   # a larger array gets every block and no more
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    x7 = np.concatenate([q, t])
    r1, J1 = ctx.eval_blocks(x7, want_jac=True)
    r0, J0 = ctx.eval_blocks(x7, want_jac=False)
    assert J0 is None and J1.shape == (nr, 7) and r1.shape == r0.shape == (nr,)
    assert np.any(r1 != 0.0) and np.array_equal(r1.view(np.uint64), r0.view(np.uint64))


def test_odometry_block_export_cap_and_residuals_only(S, frames):
    od = S.LaserOdometry(max_points=200000)
    for k, fr in enumerate(frames):
        q, t, need = od.adapter_begin(*fr["clouds"])
        assert need == (k > 0)
        if need:
            _check_open_step(od, q, t)
        od.adapter_finish(q, t)
    od.close()


def test_mapping_block_export_cap_residuals_only_and_empty_step(S, frames):
    mp = S.LaserMapping(0.4, 0.8, max_scan_points=200000, max_map_points=2000000)
    for k, fr in enumerate(frames):
        _, less_sharp, _, less_flat = fr["clouds"]
        q, t = mp.adapter_begin(less_sharp, less_flat, fr["full"], fr["q"], fr["t"])
        if k == 0:   # fresh context: the map is too small (laserMapping.cpp:555), no solve
            assert mp.associate(q, t) == (0, 0)
            for cap in (None, 5):
                assert all(a.shape[0] == 0 for a in mp.blocks(cap))
            r, J = mp.eval_blocks(np.concatenate([q, t]))
            assert r.shape == (0,) and J.shape == (0, 7)
            r, J = mp.eval_blocks(np.concatenate([q, t]), want_jac=False)
            assert r.shape == (0,) and J is None
        else:
            _check_open_step(mp, q, t)
        mp.adapter_finish(q, t)
    mp.close()
