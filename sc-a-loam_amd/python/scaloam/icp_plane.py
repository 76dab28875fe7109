"""CPU restatement of scal_icp_align_plane* (include/scaloam_hip.h): point-to-plane ICP on a target that carries normals, the
specification csrc/icp.hip and csrc/icp_dev.hpp (icp_plane_sums) are held to bit for bit, in the role nbr.py has for scal_nbr_*.  numpy
and scipy only.  Every f32 and f64 expression is elementwise in the order the header states; the 32 sums of a sweep are reduced in
the device's order (sweep_sums: the lanes' xor butterfly, the four waves, the workgroups); the LDL^T, the quaternion and the
convergence criteria are csrc/icp_host.hpp's operation by operation.  DESIGN.md section 8.14 has the reasoning.

register is the one-call use: the map's normals by nbr.estimate_normals, then the alignment, on the CPU or (device=True, through
scaloam.RadiusIndex and scaloam.LoopICP, imported only then) on the GPU; nothing else here touches the device."""
import numpy as np

NSUM = 32                 # SCAL_ICP_PLANE_NSUM
PIVOT_MIN = 1e-10         # SCAL_ICP_PLANE_PIVOT_MIN
TREE_SLACK = 1e-3         # the candidates of a query: everything within its f64 nearest distance widened by this factor (nbr.TREE_SLACK)
_TINY = 1e-20             # and by this much: differences below 4e-23 square to an f32 zero
_NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
_DBL_MAX = float(np.finfo(np.float64).max)
_F32_CAP = np.float32(3.4e38)
_TRI = [(i, j) for i in range(6) for j in range(i, 6)]


def _xyzi(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 4)


def nearest_keys(cur, tgt):
    """uint64 [n_src]: the key (f32 squared distance bits << 32 | target index) of every source point's nearest target point - the
    smallest key over all finite target points, so the lowest index among equal distances - and _NO_KEY where there is none (the
    source point is not finite, no target point is, or the distance leaves the f32 range)."""
    from scipy.spatial import cKDTree
    P, Q = cur[:, :3], tgt[:, :3]
    keys = np.full(P.shape[0], _NO_KEY, np.uint64)
    fq = np.isfinite(Q).all(1)
    fp = np.flatnonzero(np.isfinite(P).all(1))
    pos = np.flatnonzero(fq).astype(np.uint64)
    if fp.size == 0 or pos.size == 0:
        return keys
    Qf, Pf = Q[fq], P[fp]
    tree = cKDTree(Qf.astype(np.float64))
    step = 1 << 15
    for a in range(0, Pf.shape[0], step):
        p = Pf[a:a + step]
        p64 = p.astype(np.float64)
        d1, _ = tree.query(p64, k=1)
        lists = tree.query_ball_point(p64, d1 * (1.0 + TREE_SLACK) + _TINY, return_sorted=False)
        lens = np.fromiter((len(l) for l in lists), np.int64, len(lists))
        ti = np.concatenate([np.asarray(l, np.int64) for l in lists])
        pi = np.repeat(np.arange(p.shape[0]), lens)
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            dx, dy, dz = p[pi, 0] - Qf[ti, 0], p[pi, 1] - Qf[ti, 1], p[pi, 2] - Qf[ti, 2]
            d = dx * dx          # f32, the dense sweep's arithmetic
            d = d + dy * dy
            d = d + dz * dz
        ok = d < _F32_CAP
        k = (d[ok].view(np.uint32).astype(np.uint64) << np.uint64(32)) | pos[ti[ok]]
        best = np.full(p.shape[0], _NO_KEY, np.uint64)
        np.minimum.at(best, pi[ok], k)
        keys[fp[a:a + step]] = best
    return keys


def point_terms(cur, tgt, tgt_nc, keys, max2):
    """float64 [n_src, 32]: what every source point adds to the 32 sums (the header's table); +0 where it adds nothing"""
    n = cur.shape[0]
    v = np.zeros((n, NSUM), np.float64)
    has = keys != _NO_KEY
    idx = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    idx[~has] = 0
    d = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    v[has, 30] = 1.0
    v[has, 31] = d[has].astype(np.float64)
    if tgt.shape[0] == 0:
        return v
    with np.errstate(invalid="ignore"):
        row = has & ~(d > np.float32(max2)) & np.isfinite(tgt_nc[idx, :3]).all(1)
    i = np.flatnonzero(row)
    p, q, nn = cur[i, :3].astype(np.float64), tgt[idx[i], :3].astype(np.float64), tgt_nc[idx[i], :3].astype(np.float64)
    px, py, pz, nx, ny, nz = p[:, 0], p[:, 1], p[:, 2], nn[:, 0], nn[:, 1], nn[:, 2]
    with np.errstate(all="ignore"):
        a = [py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz]
        ex, ey, ez = q[:, 0] - px, q[:, 1] - py, q[:, 2] - pz
        r = (ex * nx + ey * ny) + ez * nz
        v[i, 0] = 1.0
        for k, (r0, c0) in enumerate(_TRI):
            v[i, 1 + k] = a[r0] * a[c0]
        for r0 in range(6):
            v[i, 22 + r0] = a[r0] * r
        v[i, 28] = r * r
    v[i, 29] = d[i].astype(np.float64)
    return v


def reduce_terms(v):
    """the device's reduction of the per-point terms v [n, ns] -> float64 [ns] (32 sums here, 17 in icp_point): source point i is lane
    i % 64 of wave (i / 64) % 4 of workgroup i / 256; lanes by the xor butterfly 32, 16, .. 1, waves as ((r0 + r1) + r2) + r3,
    workgroups sequentially from +0"""
    n, ns = v.shape
    nb = max((n + 255) // 256, 0)
    pad = np.zeros((nb * 256, ns), np.float64)
    pad[:n] = v
    w = pad.reshape(nb, 4, 64, ns)
    lane = np.arange(64)
    with np.errstate(all="ignore"):
        for o in (32, 16, 8, 4, 2, 1):
            w = w + w[:, :, lane ^ o, :]
        w = w[:, :, 0, :]
        part = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
        s = np.zeros(ns, np.float64)
        for b in range(nb):
            s = s + part[b]
    return s


def sweep_sums(cur, tgt, tgt_nc, max2):
    """The 32 sums of one correspondence sweep of cur [n, 4] against tgt [m, 4] with normals tgt_nc [m, 4], in the device's order.
    max2: the squared cap, as a float32."""
    cur, tgt, tgt_nc = _xyzi(cur), _xyzi(tgt), _xyzi(tgt_nc)
    return reduce_terms(point_terms(cur, tgt, tgt_nc, nearest_keys(cur, tgt), np.float32(max2)))


def solve_normal_equations(tri, b):
    """x float64 [6] of A x = b by the header's LDL^T without pivoting (A's upper triangle row-major in tri [21]), or None when a
    pivot d_j is not > PIVOT_MIN A_jj: the system is degenerate"""
    f = np.float64
    A = np.zeros((6, 6), f)
    for k, (i, j) in enumerate(_TRI):
        A[i, j] = A[j, i] = tri[k]
    L, D, v, y, x = np.zeros((6, 6), f), np.zeros(6, f), np.zeros(6, f), np.zeros(6, f), np.zeros(6, f)
    with np.errstate(all="ignore"):
        for j in range(6):
            for k in range(j):
                v[k] = L[j, k] * D[k]
            d = A[j, j]
            for k in range(j):
                d = d - L[j, k] * v[k]
            if not d > f(PIVOT_MIN) * A[j, j]:
                return None
            D[j] = d
            for i in range(j + 1, 6):
                s = A[i, j]
                for k in range(j):
                    s = s - L[i, k] * v[k]
                L[i, j] = s / d
        for i in range(6):
            y[i] = b[i]
            for k in range(i):
                y[i] = y[i] - L[i, k] * y[k]
        for i in range(6):
            x[i] = y[i] / D[i]
        for i in range(5, -1, -1):
            for k in range(i + 1, 6):
                x[i] = x[i] - L[k, i] * x[k]
    return x


def increment(x6):
    """float32 [4, 4]: the rigid increment of x = (alpha, beta, gamma, tx, ty, tz), the header's quaternion form"""
    f = np.float64
    with np.errstate(all="ignore"):
        hx, hy, hz = f(x6[0]) / f(2.0), f(x6[1]) / f(2.0), f(x6[2]) / f(2.0)
        m = np.sqrt(((f(1.0) + hx * hx) + hy * hy) + hz * hz)
        w, x, y, z = f(1.0) / m, hx / m, hy / m, hz / m
        R = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
             [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
             [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
        T = np.zeros((4, 4), np.float32)
        T[:3, :3] = np.array(R, f).astype(np.float32)
        T[:3, 3] = np.asarray(x6[3:6], f).astype(np.float32)
    T[3, 3] = 1.0
    return T


def transform(T, pts):
    """pts [n, 4] moved by the f32 matrix T as the device's icp_transform does: ((m0 x + m1 y) + m2 z) + m3 in f32, .w kept"""
    T = np.asarray(T, np.float32)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    out = pts.copy()
    with np.errstate(all="ignore"):
        for r in range(3):
            out[:, r] = ((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]
    return out


def _check_guess(guess):
    """the f32 4x4 guess to use, or None for none / the identity; ValueError as scal_icp_align_guess refuses"""
    if guess is None:
        return None
    g = np.asarray(guess)
    if g.size != 16:
        raise ValueError("the guess is a 4x4 matrix")
    with np.errstate(over="ignore"):
        g = g.astype(np.float32).reshape(4, 4)
    if not np.isfinite(g[:3]).all():
        raise ValueError("the guess is not finite")
    if not (g[3, 0] == 0 and g[3, 1] == 0 and g[3, 2] == 0 and g[3, 3] == 1):
        raise ValueError("the last row of the guess must be 0 0 0 1")
    return None if np.array_equal(g, np.eye(4, dtype=np.float32)) else g


def align_plane(src, tgt, tgt_nc, guess=None, max_corr_dist=150.0, max_iterations=100, transformation_epsilon=1e-6, fitness_epsilon=1e-6):
    """scal_icp_align_plane on the CPU: the dict scaloam.LoopICP.align_plane returns (converged, iterations, state,
    n_correspondences, fitness, plane_fitness, T [4, 4], normal_eq [27], first_eq [27])."""
    src, tgt, nc = _xyzi(src), _xyzi(tgt), _xyzi(tgt_nc)
    if nc.shape[0] != tgt.shape[0]:
        raise ValueError("tgt_nc is [n_tgt, 4]: one normal and curvature per target point")
    if not (max_iterations > 0 and max_corr_dist > 0):
        raise ValueError("max_iterations and max_corr_dist must be > 0")
    g = _check_guess(guess)
    f = np.float64
    res = dict(converged=False, iterations=0, state=0, n_correspondences=0, fitness=_DBL_MAX, plane_fitness=_DBL_MAX, T=np.eye(4),
               normal_eq=np.zeros(27), first_eq=np.zeros(27))
    if src.shape[0] == 0 or tgt.shape[0] == 0:
        res["state"] = 5
        return res
    max2 = np.float32(f(max_corr_dist) * f(max_corr_dist))
    te, fe = f(transformation_epsilon), f(fitness_epsilon)
    F = np.eye(4, dtype=np.float32)
    cur = src
    if g is not None:
        F, cur = g.copy(), transform(g, src)
    it, st, converged, prev_mse = 0, 0, False, f(_DBL_MAX)
    with np.errstate(all="ignore"):
        while True:
            sums = sweep_sums(cur, tgt, nc, max2)
            if it == 0:
                res["first_eq"] = sums[1:28].copy()
            res["n_correspondences"] = int(sums[0])
            if sums[0] < 6:
                st = 5
                break
            x = solve_normal_equations(sums[1:22], sums[22:28])
            if x is None:
                st = 6
                break
            T = increment(x)
            cur = transform(T, cur)
            F = np.stack([((T[r, 0] * F[0] + T[r, 1] * F[1]) + T[r, 2] * F[2]) + T[r, 3] * F[3] for r in range(4)])   # f32
            it += 1
            if it >= max_iterations:
                st, converged = 1, True
                break
            cos_angle = f(0.5) * (((f(T[0, 0]) + f(T[1, 1])) + f(T[2, 2])) - f(1.0))
            tr2 = (f(T[0, 3]) * f(T[0, 3]) + f(T[1, 3]) * f(T[1, 3])) + f(T[2, 3]) * f(T[2, 3])
            if cos_angle >= f(1.0) - te and tr2 <= te:
                st, converged = 2, True
                break
            mse = sums[29] / sums[0]
            if np.abs(mse - prev_mse) < f(1e-12):
                st, converged = 3, True
                break
            if np.abs(mse - prev_mse) / prev_mse < fe:
                st, converged = 4, True
                break
            prev_mse = mse
        sums = sweep_sums(transform(F, src), tgt, nc, max2)
        res.update(converged=converged, iterations=it, state=st, T=F.astype(np.float64), normal_eq=sums[1:28].copy(),
                   fitness=float(sums[31] / sums[30]) if sums[30] > 0 else _DBL_MAX,
                   plane_fitness=float(sums[28] / sums[0]) if sums[0] > 0 else _DBL_MAX)
    return res


def register(map_xyzi, cloud_xyzi, k=10, r=0.8, guess=None, device=False, **icp_settings):
    """The one-call use: the map's normals from its own k nearest neighbours within r (nbr.estimate_normals), then the cloud aligned to
    the map by point-to-plane ICP.  device=True runs both steps on the GPU (scaloam.RadiusIndex.normals_self,
    scaloam.LoopICP.align_plane) with results equal bit for bit.  icp_settings: max_corr_dist, max_iterations,
    transformation_epsilon, fitness_epsilon.  Returns align_plane's dict."""
    from . import nbr
    M, P = _xyzi(map_xyzi), _xyzi(cloud_xyzi)
    nc, _ = nbr.estimate_normals(M, k, r, device=device)
    if not device:
        return align_plane(P, M, nc, guess, **icp_settings)
    from . import LoopICP
    icp = LoopICP(max_source=max(P.shape[0], 1), max_target=max(M.shape[0], 1), **icp_settings)
    try:
        return icp.align_plane(P, M, nc, guess)
    finally:
        icp.close()
