"""scaloam/nbr.py normals_within - the specification of scal_nbr_normals* - against numpy.linalg.eigh on the inputs
tools/mapdiff_scene.py names, the Jacobi's convergence on them, a plane, hand-made rows, the viewpoint, argument checks, and the PCD
writer.  tests/test_normals_gpu.py holds the device to normals_within bit for bit."""
import functools
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = 0x7FC00000


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
    """knn_within at k = 20; k = 5 is its first columns"""
    from scaloam import nbr
    I, Q = _inputs(r)
    return nbr.knn_within(I, Q, 20, r)[0]


def _xyzi(rows):
    a = np.zeros((len(rows), 4), np.float32)
    a[:, :3] = np.asarray(rows, np.float32)
    return a


def plane_lattice():
    """49 x 49 points on z = 0.3 x - 0.2 y + 1, spacing 0.25 (z rounded to f32: off the plane by up to 2^-24 |z|)"""
    g = np.arange(-6.0, 6.25, 0.25)
    x, y = np.meshgrid(g, g, indexing="ij")
    return _xyzi(np.stack([x.ravel(), y.ravel(), (0.3 * x - 0.2 * y + 1.0).ravel()], 1))


@pytest.mark.parametrize("r", [0.5, 1.0])
@pytest.mark.parametrize("k", [5, 20])
def test_against_eigh(r, k):
    from scaloam import nbr
    I, Q = _inputs(r)
    assert Q.shape[0] == 2615
    idx = _rows(r)[:, :k]
    c, A, m = nbr.covariances(I, idx)
    fit = m >= 3
    assert 2400 <= fit.sum() <= 2500 and ((m == 0) | fit).all()
    trace = []
    lam, V = nbr.jacobi_eig3(A, trace=trace)
    assert len(trace) == 9 and trace[0] > 0 and trace[7] == 0.0 and trace[8] == 0.0      # exactly diagonal before the 8th sweep
    w, U = np.linalg.eigh(A[fit])
    tr = np.trace(A[fit], axis1=1, axis2=2)
    assert (tr > 0).all()
    err = np.abs(np.sort(lam[fit], 1) - w).max(1) / tr
    print("max |lambda - eigh| / trace", err.max())
    assert err.max() <= 1e-12
    nc, dist = nbr.normals_within(I, Q, k, r)
    assert nc.dtype == np.float32 and nc.shape == (Q.shape[0], 4) and dist.dtype == np.float32 and dist.shape == (Q.shape[0],)
    assert (nc.view(np.uint32)[~fit] == NAN).all() and (dist.view(np.uint32)[~fit] == NAN).all() and np.isfinite(nc[fit]).all()
    # the normal is the restatement's f64 column, rounded; against eigh's where the two smallest eigenvalues are apart
    j = np.argmin(lam[fit], 1)
    n64 = V[fit][np.arange(fit.sum()), :, j]
    assert np.array_equal(nc[fit, :3].view(np.uint32), n64.astype(np.float32).view(np.uint32))
    gap = (w[:, 1] - w[:, 0]) >= 1e-6 * tr
    print("rows outside the gap condition", int((~gap).sum()), "of", int(fit.sum()))
    assert (~gap).sum() <= 0.01 * fit.sum()
    dev = 1.0 - np.abs((n64 * U[:, :, 0]).sum(1))
    print("max 1 - |n . n_eigh|", dev[gap].max())
    assert dev[gap].max() <= 1e-12
    assert np.abs((n64 * n64).sum(1) - 1.0).max() <= 1e-14
    curv = nc[fit, 3].astype(np.float64)
    assert (curv >= 0).all() and (curv <= 1.0 / 3.0 + 1e-7).all() and np.abs(curv - np.maximum(w[:, 0], 0) / tr).max() <= 1e-7


def test_a_plane():
    from scaloam import nbr
    P = plane_lattice()
    nc, dist = nbr.normals_within(P, P, 9, 0.6)
    assert np.isfinite(nc).all() and np.isfinite(dist).all()       # every lattice point has 3 or more neighbours within 0.6
    u = np.array([0.3, -0.2, -1.0]) / np.linalg.norm([0.3, -0.2, -1.0])
    # z is off the plane by at most 2^-24 |z| < 3e-7 over a neighbourhood 0.25 wide or more: an angle below 1e-5
    assert np.linalg.norm(np.cross(nc[:, :3].astype(np.float64), u), axis=1).max() <= 1e-5
    assert np.abs(dist).max() <= 1e-6 and nc[:, 3].max() <= 1e-10 and nc[:, 3].min() >= 0
    for vp, sign in (((0.0, 0.0, 100.0), -1.0), ((0.0, 0.0, -100.0), 1.0)):        # above the plane: against u, whose z is negative
        nv, dv = nbr.normals_within(P, P, 9, 0.6, viewpoint=vp)
        assert (np.sign(nv[:, :3] @ u) == sign).all()
        same = nv[:, :3].view(np.uint32) == nc[:, :3].view(np.uint32)
        flipped = nv[:, :3].view(np.uint32) == nc[:, :3].view(np.uint32) ^ np.uint32(0x80000000)
        assert (same.all(1) | flipped.all(1)).all()
        assert np.array_equal(nv[:, 3].view(np.uint32), nc[:, 3].view(np.uint32))
        # the distance is negated with the normal; a sum that cancels to +0 stays +0, so by value
        assert np.array_equal(dv, np.where(flipped.all(1), -dist, dist))


def test_the_viewpoint_flips_exactly_the_sign_bits():
    from scaloam import nbr
    I, Q = _inputs(1.0)
    n0, d0 = nbr.normals_within(I, Q, 20, 1.0)
    fit = n0.view(np.uint32)[:, 0] != NAN
    sign = np.uint32(0x80000000)
    seen = []
    for vp in ((0.5, -0.25, 40.0), (0.5, -0.25, -40.0)):
        n1, d1 = nbr.normals_within(I, Q, 20, 1.0, viewpoint=vp)
        assert np.array_equal(n1.view(np.uint32)[~fit], n0.view(np.uint32)[~fit]) and (d1.view(np.uint32)[~fit] == NAN).all()
        x = n1.view(np.uint32)[fit] ^ n0.view(np.uint32)[fit]
        flipped = x[:, 0] == sign
        assert (x[:, 3] == 0).all() and (x[:, :3] == np.where(flipped, sign, 0)[:, None]).all()
        assert np.array_equal(d1[fit], np.where(flipped, -d0[fit], d0[fit]))      # by value: a sum that cancels to +0 stays +0
        w = np.asarray(vp)[None, :] - Q[fit, :3].astype(np.float64)
        dot = (n1[fit, :3].astype(np.float64) * w).sum(1)
        assert (dot >= -1e-5).all() and 0 < flipped.sum() < fit.sum()
        seen.append(flipped)
    assert (seen[0] != seen[1]).mean() > 0.5         # most queries lie between the two viewpoints


def test_hand_made_rows():
    from scaloam import nbr
    two = _xyzi([(0, 0, 0), (0.1, 0, 0), (5, 5, 5)])
    nc, dist = nbr.normals_within(two, two[:1], 3, 0.5)                     # m = 2
    assert (nc.view(np.uint32) == NAN).all() and (dist.view(np.uint32) == NAN).all()
    dup = _xyzi([(0.3, -1.7, 2.9)] * 3)
    nc, dist = nbr.normals_within(dup, dup[:1], 5, 0.5)                     # C = 0: no rotation, V stays the identity
    assert nc.view(np.uint32).tolist() == [[0x3F800000, 0, 0, 0]] and dist.view(np.uint32).tolist() == [0]
    line = _xyzi([(0, 0, 0), (1, 0, 0), (2, 0, 0)])
    nc, dist = nbr.normals_within(line, line[1:2], 3, 1.5)                  # diag(2/3, 0, 0): the tie goes to the lower column
    assert nc.view(np.uint32).tolist() == [[0, 0x3F800000, 0, 0]] and dist.view(np.uint32).tolist() == [0]
    skew = _xyzi([(0, 0, 0), (1, 1, 0), (2, 2, 0), (3, 3, 0)])
    nc, dist = nbr.normals_within(skew, _xyzi([(1.5, 1.5, 0.25)]), 4, 4.0)  # a line in the x-y plane: lambda = (0, 4.5 / 2 .., 0)
    n = nc[0, :3].astype(np.float64)
    assert abs(n @ np.array([1.0, 1.0, 0.0])) <= 1e-7 and abs(n @ n - 1.0) <= 1e-6 and nc[0, 3] == 0.0
    q = _xyzi([(np.nan, 0, 0), (0, np.inf, 0), (1, 0, 0)])
    nc, dist = nbr.normals_within(line, q, 3, 1.5)
    assert (nc.view(np.uint32)[:2] == NAN).all() and (dist.view(np.uint32)[:2] == NAN).all() and np.isfinite(nc[2]).all()
    nc, dist = nbr.normals_within(np.zeros((0, 4), np.float32), q, 3, 1.5)  # an empty index
    assert nc.shape == (3, 4) and (nc.view(np.uint32) == NAN).all() and (dist.view(np.uint32) == NAN).all()
    nc, dist = nbr.normals_within(line, np.zeros((0, 4), np.float32), 3, 1.5)
    assert nc.shape == (0, 4) and dist.shape == (0,)
    assert nbr.NAN_BITS == NAN and "0x7fc00000" in open(os.path.join(ROOT, "include", "scaloam_hip.h")).read()


def test_untouched_means_untouched():
    """a pair with a_pq == 0 is skipped, not rotated by the identity: a -0 in A or V survives"""
    from scaloam import nbr
    A = np.array([[[2.0, 0.0, 0.5], [0.0, -0.0, 0.0], [0.5, 0.0, 1.0]]])
    lam, V = nbr.jacobi_eig3(A)
    assert np.signbit(lam[0, 1]) and V[0, 1].tolist() == [0.0, 1.0, 0.0] and V[0, :, 1].tolist() == [0.0, 1.0, 0.0]
    w = np.linalg.eigvalsh(A[0])
    assert np.abs(np.sort(lam[0]) - w).max() <= 1e-15


def test_estimate_and_point_to_plane():
    from scaloam import nbr
    I, Q = _inputs(0.5)
    nc, dist = nbr.estimate_normals(I, 11, 0.5)
    want = nbr.normals_within(I, I, 11, 0.5)
    assert np.array_equal(nc.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(dist.view(np.uint32), want[1].view(np.uint32))
    d, valid = nbr.point_to_plane(I, Q, 11, 0.5)
    want = nbr.normals_within(I, Q, 11, 0.5)[1]
    assert np.array_equal(d.view(np.uint32), want.view(np.uint32)) and np.array_equal(valid, ~np.isnan(want)) and 0 < valid.sum() < Q.shape[0]
    st = nbr.residual_stats(d, valid)
    assert st["valid"] == valid.sum() and st["points"] == Q.shape[0] and 0 < st["median_abs"] <= st["rms"] and st["mean_abs"] <= st["rms"] <= 0.5
    assert nbr.residual_stats(d[:0], valid[:0]) == dict(valid=0, points=0, mean_abs=None, rms=None, median_abs=None)


def test_argument_checks():
    from scaloam import nbr
    I, Q = _inputs(0.5)
    for k in (0, 2, 65, 2.5, -3):
        for call in (lambda: nbr.normals_within(I, Q, k, 0.5), lambda: nbr.estimate_normals(I, k, 0.5), lambda: nbr.point_to_plane(I, Q, k, 0.5)):
            with pytest.raises(ValueError):
                call()
    for r in (0.0, -1.0, np.inf, np.nan, 1e-60):
        with pytest.raises(ValueError):
            nbr.normals_within(I, Q, 5, r)
    for vp in ((0, 0), (0, 0, 0, 1), ()):
        with pytest.raises(ValueError):
            nbr.normals_within(I, Q, 5, 0.5, viewpoint=vp)
    assert nbr.MIN_NORMAL_K == 3 and nbr.JACOBI_SWEEPS == 8


def test_pcd_writer_round_trip(tmp_path):
    from scaloam import formats, nbr
    I, _ = _inputs(0.5)
    I = I.copy()
    I[:, 3] = np.arange(I.shape[0], dtype=np.float32)
    nc, _ = nbr.estimate_normals(I, 11, 0.5)
    path = str(tmp_path / "n.pcd")
    formats.write_pcd_normals_binary(path, I, nc)
    head = open(path, "rb").read(400).decode("ascii", "replace")
    assert "FIELDS x y z intensity normal_x normal_y normal_z curvature\n" in head and f"POINTS {I.shape[0]}\n" in head
    assert os.path.getsize(path) == head.index("DATA binary\n") + len("DATA binary\n") + 32 * I.shape[0]
    assert np.array_equal(formats.read_pcd(path).view(np.uint32), I.view(np.uint32))       # the reader skips what it does not know
    back = formats.read_pcd_normals(path)
    assert np.array_equal(back[0].view(np.uint32), I.view(np.uint32)) and np.array_equal(back[1].view(np.uint32), nc.view(np.uint32))
    with pytest.raises(ValueError):
        formats.write_pcd_normals_binary(path, I, nc[:-1])
    formats.write_pcd_binary(path, I)
    with pytest.raises(ValueError):
        formats.read_pcd_normals(path)
