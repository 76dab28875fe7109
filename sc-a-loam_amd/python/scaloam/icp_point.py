"""CPU restatement of scal_icp_align* (include/scaloam_hip.h): the point-to-point loop-verification ICP, the specification
csrc/icp.hip, csrc/icp_dev.hpp (icp_corr_sums) and csrc/icp_host.hpp are held to bit for bit, in the role icp_plane.py has for
scal_icp_align_plane*.  numpy and scipy only.  The search (nearest_keys: smallest f32 squared distance, lowest index among equals),
the point transform, the guess check and the device's reduction order (reduce_terms) are icp_plane's; the 17 sums of a sweep, Horn's
closed form with its cyclic Jacobi and the convergence ladder are restated here operation by operation, every scalar an IEEE f64
and every matrix entry rounded to f32 where the host rounds it.  Nothing here touches the device."""
import numpy as np

from .icp_plane import _DBL_MAX, _F32_CAP, _NO_KEY, _check_guess, _xyzi, nearest_keys, reduce_terms, transform

NSUM = 17                 # ICP_NSUM: n, sum p[3], sum q[3], sum q p^T[9] row-major, sum d^2
JACOBI_SWEEPS = 64        # eig4_max's sweep limit


def point_terms(cur, tgt, keys, max2):
    """float64 [n_src, 17]: what icp_corr_sums adds for every source point p with nearest target point q at f32 squared distance d:
    1, p, q, q_r * p_c (row-major, f64 products of the f32 coordinates), d; +0 where there is no key or d > max2 (equality kept)"""
    n = cur.shape[0]
    v = np.zeros((n, NSUM), np.float64)
    has = keys != _NO_KEY
    idx = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    idx[~has] = 0
    d = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    if tgt.shape[0] == 0:
        return v
    with np.errstate(invalid="ignore"):
        i = np.flatnonzero(has & ~(d > np.float32(max2)))
    p, q = cur[i, :3].astype(np.float64), tgt[idx[i], :3].astype(np.float64)
    v[i, 0] = 1.0
    v[i, 1:4] = p
    v[i, 4:7] = q
    with np.errstate(all="ignore"):
        for r in range(3):
            for c in range(3):
                v[i, 7 + 3 * r + c] = q[:, r] * p[:, c]
    v[i, 16] = d[i].astype(np.float64)
    return v


def sweep_sums(cur, tgt, max2):
    """The 17 sums of one correspondence sweep of cur [n, 4] against tgt [m, 4], in the device's order (k_icp_reduce per workgroup,
    k_icp_final over the workgroups from +0).  max2: the squared cap, as a float32."""
    cur, tgt = _xyzi(cur), _xyzi(tgt)
    return reduce_terms(point_terms(cur, tgt, nearest_keys(cur, tgt), np.float32(max2)))


def _eig4_max(a):
    """icp_host.hpp's eig4_max: the unit eigenvector (w, x, y, z) of the largest eigenvalue of the symmetric 4x4 a (a list of lists
    of np.float64, overwritten) by cyclic Jacobi"""
    f = np.float64
    one, zero = f(1.0), f(0.0)
    v = [[one if i == j else zero for j in range(4)] for i in range(4)]
    for _ in range(JACOBI_SWEEPS):
        off, diag = zero, zero
        for i in range(4):
            for j in range(4):
                if i == j:
                    diag = diag + a[i][j] * a[i][j]
                else:
                    off = off + a[i][j] * a[i][j]
        if off <= f(1e-40) * diag or off == zero:
            break
        for p in range(3):
            for r in range(p + 1, 4):
                if a[p][r] == zero:
                    continue
                theta = (a[r][r] - a[p][p]) / (f(2.0) * a[p][r])
                t = (one if theta >= zero else -one) / (np.abs(theta) + np.sqrt(theta * theta + one))
                c = one / np.sqrt(t * t + one)
                s = t * c
                for k in range(4):
                    akp, akr = a[k][p], a[k][r]
                    a[k][p], a[k][r] = c * akp - s * akr, s * akp + c * akr
                for k in range(4):
                    apk, ark = a[p][k], a[r][k]
                    a[p][k], a[r][k] = c * apk - s * ark, s * apk + c * ark
                for k in range(4):
                    vkp, vkr = v[k][p], v[k][r]
                    v[k][p], v[k][r] = c * vkp - s * vkr, s * vkp + c * vkr
    best = 0
    for i in range(1, 4):
        if a[i][i] > a[best][best]:
            best = i
    nrm = zero
    for k in range(4):
        nrm = nrm + v[k][best] * v[k][best]
    nrm = np.sqrt(nrm)
    return [v[k][best] / nrm for k in range(4)]


def transform_from_sums(sums):
    """float32 [4, 4]: icp_host.hpp's transform_from_sums, the rigid increment that moves the p onto the q in the least-squares
    sense (Horn's quaternion form), from sums[0 .. 16) = n, sum p, sum q, sum q_r p_c"""
    f = np.float64
    sums = [f(x) for x in np.asarray(sums, f).reshape(-1)[:16]]
    with np.errstate(all="ignore"):
        n = sums[0]
        mp = [sums[1 + k] / n for k in range(3)]
        mq = [sums[4 + k] / n for k in range(3)]
        S = [[None] * 3 for _ in range(3)]
        for r in range(3):
            for c in range(3):
                S[c][r] = sums[7 + 3 * r + c] / n - mq[r] * mp[c]        # S[a][b] = cov(p_a, q_b)
        N = [[S[0][0] + S[1][1] + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0]],
             [S[1][2] - S[2][1], S[0][0] - S[1][1] - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2]],
             [S[2][0] - S[0][2], S[0][1] + S[1][0], -S[0][0] + S[1][1] - S[2][2], S[1][2] + S[2][1]],
             [S[0][1] - S[1][0], S[2][0] + S[0][2], S[1][2] + S[2][1], -S[0][0] - S[1][1] + S[2][2]]]
        w, x, y, z = _eig4_max(N)
        R = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
             [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
             [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
        T = np.zeros((4, 4), np.float32)
        for r in range(3):
            t = mq[r]
            for c in range(3):
                T[r, c] = np.float32(R[r][c])
                t = t - R[r][c] * mp[c]
            T[r, 3] = np.float32(t)
    T[3, 3] = 1.0
    return T


def align(src, tgt, guess=None, max_corr_dist=150.0, max_iterations=100, transformation_epsilon=1e-6, fitness_epsilon=1e-6):
    """scal_icp_align / scal_icp_align_guess on the CPU: the dict scaloam.LoopICP.align returns (converged, iterations, state,
    n_correspondences, fitness, T [4, 4]).  States: 1 iteration cap, 2 increment below transformation_epsilon, 3 absolute and
    4 relative change of the mean squared distance, 5 fewer than 3 correspondences or an empty cloud (not converged)."""
    src, tgt = _xyzi(src), _xyzi(tgt)
    if not (max_iterations > 0 and max_corr_dist > 0):
        raise ValueError("max_iterations and max_corr_dist must be > 0")
    g = _check_guess(guess)
    f = np.float64
    res = dict(converged=False, iterations=0, state=0, n_correspondences=0, fitness=_DBL_MAX, T=np.eye(4))
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
            sums = sweep_sums(cur, tgt, max2)
            res["n_correspondences"] = int(sums[0])
            if sums[0] < 3:
                st = 5
                break
            T = transform_from_sums(sums)
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
            mse = sums[16] / sums[0]
            if np.abs(mse - prev_mse) < f(1e-12):
                st, converged = 3, True
                break
            if np.abs(mse - prev_mse) / prev_mse < fe:
                st, converged = 4, True
                break
            prev_mse = mse
        # getFitnessScore(): the original source moved by the whole transformation, no cap
        sums = sweep_sums(transform(F, src), tgt, _F32_CAP)
        res.update(converged=converged, iterations=it, state=st, T=F.astype(np.float64),
                   fitness=float(sums[16] / sums[0]) if sums[0] > 0 else _DBL_MAX)
    return res
