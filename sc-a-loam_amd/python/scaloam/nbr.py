"""CPU restatement of scal_nbr_* (include/scaloam_hip.h) and the two uses built on it: the map diff between two sessions that share a
frame, and a radius outlier filter.  radius_counts is the specification csrc/nbr.hip is held to bit for bit, in the role removert.py
has for scal_removert; numpy and scipy only, every f32 expression elementwise in the order the header states.  DESIGN.md section
8.11 has the reasoning.  The functions that take device=True run the same steps on the GPU through scaloam.RadiusIndex and
scaloam.Removert (imported only then); nothing else here touches the device.

knn_within is the specification of scal_nbr_knn* in the same way (the k nearest candidates within r by (d2, input position), DESIGN.md
section 8.12); knn makes exact unbounded k-NN of it by escalating the radius, statistical_outlier_mask is the filter built on that.

normals_within is the specification of scal_nbr_normals* (the plane through a query's knn_within row: normal, curvature, signed
distance; f64, every sum in row order, a cyclic Jacobi); estimate_normals and point_to_plane are its uses.

PCL is not on the machines this was written on, so radius_outlier_mask and statistical_outlier_mask restate PCL 1.8's
RadiusOutlierRemoval and StatisticalOutlierRemoval rules from their source text - parity unpinned, as DESIGN.md section 2 says of the
other PCL restatements."""
import numpy as np

from . import removert as _rv

# Twice the project's 0.4 m map leaf.  Two maps filtered on the same global voxel lattice can put their centroids of one surface up
# to a voxel diagonal apart (0.4 sqrt(3) = 0.69 m): a radius below that would call a surface both sessions saw "changed".  A
# setting, not a measured value.
DEFAULT_RADIUS = 0.8
BRUTE_LIMIT = 4000        # index and query sets up to this size take the dense path
TREE_SLACK = 1e-3         # the tree's f64 radius is wider by this factor; it only widens the candidate list
COMMON, UNOBSERVED, CHANGED = 0, 1, 2
MAX_K = 64                # SCAL_NBR_MAX_K
_NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _xyzi(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 4)


def _radius(r):
    with np.errstate(over="ignore", under="ignore"):
        r32 = np.float32(r)
    if not (np.isfinite(r) and r > 0 and np.isfinite(r32) and r32 > 0):
        raise ValueError("the radius must be finite and > 0 (as a float32 too)")
    with np.errstate(over="ignore", under="ignore"):
        return r32, np.float32(r32 * r32)


def _d2(q, p):
    """the header's f32 d2 of q [.., 3] and p [.., 3], every operation rounded once"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        dx, dy, dz = q[..., 0] - p[..., 0], q[..., 1] - p[..., 1], q[..., 2] - p[..., 2]
        return ((dx * dx + dy * dy) + dz * dz).astype(np.float32)


def _brute(I, Q, r2, count, best):
    """every finite query against every finite index record; Q in slabs that keep the dense block small"""
    if I.shape[0] == 0:
        return
    step = max(1, (1 << 22) // I.shape[0])
    for a in range(0, Q.shape[0], step):
        d2 = _d2(Q[a:a + step, None, :], I[None, :, :])
        within = d2 <= r2
        count[a:a + step] = within.sum(1)
        best[a:a + step] = np.where(within, d2, np.float32(np.inf)).min(1)


def _tree(I, Q, r32, r2, count, best, progress=None):
    from scipy.spatial import cKDTree
    if I.shape[0] == 0:
        return
    tree = cKDTree(I.astype(np.float64))
    step = 1 << 16
    for a in range(0, Q.shape[0], step):
        if progress:
            progress(a, Q.shape[0])
        q = Q[a:a + step]
        lists = tree.query_ball_point(q.astype(np.float64), float(r32) * (1.0 + TREE_SLACK), return_sorted=False)
        lens = np.fromiter((len(l) for l in lists), np.int64, len(lists))
        if lens.sum() == 0:
            continue
        pi = np.concatenate([np.asarray(l, np.int64) for l in lists if len(l)])
        qi = np.repeat(np.arange(q.shape[0]), lens)
        d2 = _d2(q[qi], I[pi])
        within = d2 <= r2
        count[a:a + step] = np.bincount(qi[within], minlength=q.shape[0])
        b = np.full(q.shape[0], np.inf, np.float32)
        np.minimum.at(b, qi[within], d2[within])
        best[a:a + step] = b


def radius_counts(index_xyzi, query_xyzi, r, path=None, progress=None):
    """(count uint16 [nq] saturating at 65535, min_d2 float32 [nq], +inf where count is 0).  path: "brute", "tree" or None = by size.
    progress(done, total) is called by the tree path before every slab of 65536 queries (long runs of the benchmark)."""
    I, Q = _xyzi(index_xyzi), _xyzi(query_xyzi)
    r32, r2 = _radius(r)
    fi, fq = np.isfinite(I[:, :3]).all(1), np.isfinite(Q[:, :3]).all(1)
    Ifin, Qfin = I[fi, :3], Q[fq, :3]
    cnt, best = np.zeros(Qfin.shape[0], np.int64), np.full(Qfin.shape[0], np.inf, np.float32)
    if path is None:
        path = "brute" if max(I.shape[0], Q.shape[0]) <= BRUTE_LIMIT else "tree"
    if path == "brute":
        _brute(Ifin, Qfin, r2, cnt, best)
    elif path == "tree":
        _tree(Ifin, Qfin, r32, r2, cnt, best, progress)
    else:
        raise ValueError("path is 'brute', 'tree' or None")
    count, min_d2 = np.zeros(Q.shape[0], np.uint16), np.full(Q.shape[0], np.inf, np.float32)
    count[fq], min_d2[fq] = np.minimum(cnt, 65535).astype(np.uint16), best
    return count, min_d2


def _device_counts(index_xyzi, query_xyzi, r, self_query=False):
    from . import RadiusIndex
    I = _xyzi(index_xyzi)
    Q = I if self_query else _xyzi(query_xyzi)
    idx = RadiusIndex(max(I.shape[0], 1), max(min(Q.shape[0], 1 << 24), 1))
    try:
        idx.set_index(I, r)
        return idx.query_self() if self_query else idx.query(Q)
    finally:
        idx.close()


def radius_outlier_mask(xyzi, r, min_neighbors, device=False):
    """bool [n]: the records to keep.  PCL 1.8 RadiusOutlierRemoval: radiusSearch returns the point itself among its neighbours and
    a point stays iff that number is > min_neighbors (setMinNeighborsInRadius; filters/impl/radius_outlier_removal.hpp compares
    `k <= min_pts_radius_` to drop).  Records that are not finite are dropped.  Counts saturate at 65535: min_neighbors above
    65534 keeps nothing."""
    P = _xyzi(xyzi)
    _radius(r)
    if int(min_neighbors) < 0:
        raise ValueError("min_neighbors must be >= 0")
    count, _ = _device_counts(P, None, r, self_query=True) if device else radius_counts(P, P, r)
    return (count.astype(np.int64) > int(min_neighbors)) & np.isfinite(P[:, :3]).all(1)


def _k(k):
    if int(k) != k or not 1 <= int(k) <= MAX_K:
        raise ValueError(f"k must be an integer in 1 .. {MAX_K}")
    return int(k)


def _rows(keys):
    """sorted uint64 keys (d2 bits << 32 | position, _NO_KEY as padding) -> (idx int32, d2 float32)"""
    pad = keys == _NO_KEY
    idx = np.where(pad, -1, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    d2 = np.where(pad, np.float32(np.inf), (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)).astype(np.float32)
    return idx, d2


def _knn_brute(I, pos, Q, r2, k, keys):
    """dense: the key (d2 bits, position) of every candidate pair, the k smallest per query.  d2 is >= +0 and never NaN, so its bits
    order as its value does - the device keeps the same keys"""
    if I.shape[0] == 0:
        return
    step = max(1, (1 << 21) // I.shape[0])
    for a in range(0, Q.shape[0], step):
        d2 = _d2(Q[a:a + step, None, :], I[None, :, :])
        key = np.where(d2 <= r2, (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | pos[None, :], _NO_KEY)
        m = min(k, key.shape[1])
        if m < key.shape[1]:
            key = np.partition(key, m - 1, axis=1)[:, :m]
        keys[a:a + step, :m] = np.sort(key, axis=1)


def _knn_tree(I, pos, Q, r32, r2, k, keys):
    """candidates from the tree at a slightly wider f64 radius, the exact f32 decision, a lexsort on (d2, position) per query"""
    from scipy.spatial import cKDTree
    if I.shape[0] == 0:
        return
    tree = cKDTree(I.astype(np.float64))
    step = 1 << 16
    for a in range(0, Q.shape[0], step):
        q = Q[a:a + step]
        lists = tree.query_ball_point(q.astype(np.float64), float(r32) * (1.0 + TREE_SLACK), return_sorted=False)
        lens = np.fromiter((len(l) for l in lists), np.int64, len(lists))
        if lens.sum() == 0:
            continue
        pi = np.concatenate([np.asarray(l, np.int64) for l in lists if len(l)])
        qi = np.repeat(np.arange(q.shape[0]), lens)
        d2 = _d2(q[qi], I[pi])
        within = d2 <= r2
        pi, qi, d2 = pi[within], qi[within], d2[within]
        order = np.lexsort((pos[pi], d2, qi))
        pi, qi, d2 = pi[order], qi[order], d2[order]
        first = np.searchsorted(qi, np.arange(q.shape[0]))       # where each query's candidates begin
        rank = np.arange(qi.shape[0]) - first[qi]
        take = rank < k
        keys[a + qi[take], rank[take]] = (d2[take].view(np.uint32).astype(np.uint64) << np.uint64(32)) | pos[pi[take]]


def knn_within(index_xyzi, query_xyzi, k, r, path=None):
    """(idx int32 [nq, k], d2 float32 [nq, k]): per query its first k candidates - the finite index records with d2 <= r2 - in the
    order (d2, input position), padded with -1 and +inf; a query that is not finite gets a padded row.  path as in radius_counts."""
    I, Q = _xyzi(index_xyzi), _xyzi(query_xyzi)
    k = _k(k)
    r32, r2 = _radius(r)
    fi, fq = np.isfinite(I[:, :3]).all(1), np.isfinite(Q[:, :3]).all(1)
    Ifin, Qfin, pos = I[fi, :3], Q[fq, :3], np.flatnonzero(fi).astype(np.uint64)
    keys = np.full((Qfin.shape[0], k), _NO_KEY, np.uint64)
    if path is None:
        path = "brute" if max(I.shape[0], Q.shape[0]) <= BRUTE_LIMIT else "tree"
    if path == "brute":
        _knn_brute(Ifin, pos, Qfin, r2, k, keys)
    elif path == "tree":
        _knn_tree(Ifin, pos, Qfin, r32, r2, k, keys)
    else:
        raise ValueError("path is 'brute', 'tree' or None")
    out = np.full((Q.shape[0], k), _NO_KEY, np.uint64)
    out[fq] = keys
    return _rows(out)


def knn(index_xyzi, query_xyzi, k, r0, r_max=None, device=False):
    """Exact k nearest neighbours without a radius, by escalation: knn_within at r0, then again at twice the radius for the queries
    whose row is not full, and so on.  A full row is final: what the bound left out is strictly farther than its last entry.  It stops
    when no row is short; when a short row holds every finite index record - the radius covers them all, I has fewer than k; when
    the next radius would pass r_max (short rows then stay as the last level left them: padded behind the neighbours within that
    radius); or when the radius leaves the float32 range.  query_xyzi None is the self query.  device=True swaps the bounded
    primitive for scaloam.RadiusIndex (the index rebuilt per level, only the unresolved queries sent) and nothing else.
    Returns (idx int32 [nq, k], d2 float32 [nq, k], levels)."""
    I = _xyzi(index_xyzi)
    Q = I if query_xyzi is None else _xyzi(query_xyzi)
    k = _k(k)
    _radius(r0)
    if r_max is not None and not r_max >= r0:
        raise ValueError("r_max must be >= r0")
    nq = Q.shape[0]
    idx, d2 = np.full((nq, k), -1, np.int32), np.full((nq, k), np.inf, np.float32)
    need = min(k, int(np.isfinite(I[:, :3]).all(1).sum()))       # the longest a row can get
    pending = np.flatnonzero(np.isfinite(Q[:, :3]).all(1)) if need else np.zeros(0, np.int64)
    ctx = None
    if device and pending.size:
        from . import RadiusIndex
        ctx = RadiusIndex(max(I.shape[0], 1), max(min(nq, 1 << 22), 1))
    levels, r = 0, float(r0)
    try:
        while pending.size:
            if ctx is not None:
                ctx.set_index(I, r)
                whole = query_xyzi is None and pending.size == nq == I.shape[0]
                li, ld = ctx.knn_self(k) if whole else ctx.knn(Q[pending], k)
                if whole:
                    li, ld = li[pending], ld[pending]
            else:
                li, ld = knn_within(I, Q[pending], k, r)
            idx[pending], d2[pending] = li, ld
            levels += 1
            pending = pending[(li >= 0).sum(1) < need]
            r *= 2.0
            with np.errstate(over="ignore"):
                if (r_max is not None and r > r_max) or not np.isfinite(np.float32(r)):
                    break
    finally:
        if ctx is not None:
            ctx.close()
    return idx, d2, levels


def statistical_outlier_mask(xyzi, mean_k, std_mul, r0, r_max=None, device=False):
    """bool [n]: the records to keep.  PCL 1.8 StatisticalOutlierRemoval (filters/impl/statistical_outlier_removal.hpp), restated:
    nearestKSearch with mean_k + 1 returns the point itself first and it is dropped; dist_i is the f64 mean of sqrt(float64(d2))
    over the other mean_k; over the n_v valid points mean = sum / n_v, var = (sq_sum - sum sum / n_v) / (n_v - 1) and a point stays
    iff dist_i <= mean + std_mul sqrt(var).  A record that is not finite, or whose row is short (fewer than mean_k + 1 finite records
    within r_max, or in the cloud), has dist_i = +inf: it is dropped and takes no part in the statistics.  With fewer than two
    valid points the variance is taken as 0 (PCL divides by zero there), and a variance that rounding left below 0 likewise.  The neighbour lists come from knn (r0, r_max, device as
    there); everything after them is the same host numpy for both paths, so equal lists give equal masks."""
    P = _xyzi(xyzi)
    if int(mean_k) != mean_k or not 1 <= int(mean_k) <= MAX_K - 1:
        raise ValueError(f"mean_k must be an integer in 1 .. {MAX_K - 1}")
    if not np.isfinite(std_mul):
        raise ValueError("std_mul must be finite")
    idx, d2, _ = knn(P, None, int(mean_k) + 1, r0, r_max, device)
    valid = idx[:, -1] >= 0
    dist = np.full(P.shape[0], np.inf, np.float64)
    dist[valid] = np.sqrt(d2[valid, 1:].astype(np.float64)).mean(1)
    n_v = int(valid.sum())
    if n_v == 0:
        return np.zeros(P.shape[0], bool)
    total, sq = float(dist[valid].sum()), float((dist[valid] * dist[valid]).sum())
    mean = total / n_v
    var = max((sq - total * total / n_v) / (n_v - 1), 0.0) if n_v > 1 else 0.0
    return dist <= mean + float(std_mul) * np.sqrt(var)


NAN_BITS = 0x7FC00000     # SCAL_NBR_NAN_BITS: every output of a query with fewer than MIN_NORMAL_K neighbours
MIN_NORMAL_K = 3
JACOBI_SWEEPS = 8
_PAIRS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))       # (p, q, r) of a sweep


def _normal_k(k):
    if int(k) != k or not MIN_NORMAL_K <= int(k) <= MAX_K:
        raise ValueError(f"k must be an integer in {MIN_NORMAL_K} .. {MAX_K}")
    return int(k)


def _viewpoint(viewpoint):
    if viewpoint is None:
        return None
    v = np.asarray(viewpoint, np.float64).reshape(-1)
    if v.shape[0] != 3:
        raise ValueError("the viewpoint is three numbers")
    return v


def covariances(index_xyzi, idx):
    """(c float64 [n, 3], A float64 [n, 3, 3] symmetric, m int64 [n]) of the rows idx (knn_within's, padded with -1): the header's two
    passes, every sum sequential in row order from +0.  Rows with m < 3 hold zeros."""
    P = _xyzi(index_xyzi)[:, :3].astype(np.float64)
    idx = np.asarray(idx)
    n, k = idx.shape
    m = (idx >= 0).sum(1)
    m = np.where(m >= MIN_NORMAL_K, m, 0)
    use = m > 0
    dm = np.where(use, m, 1).astype(np.float64)
    c = np.zeros((n, 3), np.float64)
    for s in range(k):
        on = use & (idx[:, s] >= 0)
        c[on] = c[on] + P[idx[on, s]]
    c = c / dm[:, None]
    S = np.zeros((n, 6), np.float64)
    for s in range(k):
        on = use & (idx[:, s] >= 0)
        d = P[idx[on, s]] - c[on]
        S[on] = S[on] + np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], 1)
    S = S / dm[:, None]
    A = np.zeros((n, 3, 3), np.float64)
    for col, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        A[:, i, j] = A[:, j, i] = S[:, col]
    return c, A, m


def jacobi_eig3(A, sweeps=JACOBI_SWEEPS, trace=None):
    """The header's cyclic Jacobi on symmetric A [n, 3, 3] (not changed): (diag float64 [n, 3], V float64 [n, 3, 3], eigenvectors in
    V's columns).  + - * / sqrt, compares and selects; a pair with a_pq == 0 leaves its row of A and V untouched.  trace, a list,
    receives the largest |off-diagonal| over all rows before every sweep and after the last."""
    A = np.array(A, np.float64)
    n = A.shape[0]
    V = np.zeros((n, 3, 3), np.float64)
    V[:, 0, 0] = V[:, 1, 1] = V[:, 2, 2] = 1.0

    def off():
        return float(np.abs(np.stack([A[:, 0, 1], A[:, 0, 2], A[:, 1, 2]], 1)).max()) if n else 0.0

    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            if trace is not None:
                trace.append(off())
            for p, q, r in _PAIRS:
                apq = A[:, p, q]
                on = apq != 0
                if not on.any():
                    continue
                apq, app, aqq, arp, arq = apq[on], A[on, p, p], A[on, q, q], A[on, r, p], A[on, r, q]
                theta = (aqq - app) / (2.0 * apq)
                t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                t = np.where(theta < 0, -t, t)
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                h = t * apq
                A[on, p, p], A[on, q, q] = app - h, aqq + h
                A[on, p, q] = A[on, q, p] = 0.0
                A[on, r, p] = A[on, p, r] = c * arp - s * arq
                A[on, r, q] = A[on, q, r] = s * arp + c * arq
                vp, vq = V[on, :, p], V[on, :, q]
                V[on, :, p], V[on, :, q] = c[:, None] * vp - s[:, None] * vq, s[:, None] * vp + c[:, None] * vq
    if trace is not None:
        trace.append(off())
    return np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], 1), V


def normals_within(index_xyzi, query_xyzi, k, r, viewpoint=None, path=None):
    """The specification of scal_nbr_normals* (include/scaloam_hip.h): (nc float32 [nq, 4], dist float32 [nq]).
    Per query the plane through its knn_within(k, r) row: nc is the unit normal (the eigenvector of the row's covariance for the
    smallest eigenvalue, turned towards viewpoint when one is given) and the curvature lambda_min / trace; dist the query's signed
    distance to the plane through the row's centroid.  All five are NaN (NAN_BITS) where the row has fewer than 3 entries.  Vectorised
    over the queries, a loop over slots and sweeps; f64, one rounding per operation, sums in row order."""
    I, Q = _xyzi(index_xyzi), _xyzi(query_xyzi)
    k = _normal_k(k)
    vp = _viewpoint(viewpoint)
    idx, _ = knn_within(I, Q, k, r, path)
    return fit_rows(I, Q, idx, vp)


def fit_rows(index_xyzi, query_xyzi, idx, viewpoint=None):
    """normals_within's tail: the fit of the rows idx [nq, k] (knn_within's, or the device's - they are equal), one per query"""
    I, Q, vp = _xyzi(index_xyzi), _xyzi(query_xyzi), _viewpoint(viewpoint)
    c, A, m = covariances(I, idx)
    lam, V = jacobi_eig3(A)
    n = Q.shape[0]
    rows = np.arange(n)
    j = np.zeros(n, np.int64)
    lmin = lam[:, 0].copy()
    for col in (1, 2):
        less = lam[:, col] < lmin
        lmin, j = np.where(less, lam[:, col], lmin), np.where(less, col, j)
    nrm = V[rows, :, j]
    with np.errstate(all="ignore"):
        tr = (lam[:, 0] + lam[:, 1]) + lam[:, 2]
        curv = np.where(tr > 0, np.where(lmin > 0, lmin, 0.0) / np.where(tr > 0, tr, 1.0), 0.0)
        q = Q[:, :3].astype(np.float64)
        if vp is not None:
            w = vp[None, :] - q
            flip = (nrm[:, 0] * w[:, 0] + nrm[:, 1] * w[:, 1]) + nrm[:, 2] * w[:, 2] < 0
            nrm = np.where(flip[:, None], -nrm, nrm)
        e = q - c
        dist = ((nrm[:, 0] * e[:, 0] + nrm[:, 1] * e[:, 1]) + nrm[:, 2] * e[:, 2]).astype(np.float32)
        nc = np.concatenate([nrm, curv[:, None]], 1).astype(np.float32)
    none = m == 0
    nc.view(np.uint32)[none] = NAN_BITS
    dist.view(np.uint32)[none] = NAN_BITS
    return nc, dist


def _device_normals(I, Q, k, r, viewpoint):
    from . import RadiusIndex
    ctx = RadiusIndex(max(I.shape[0], 1), max(min(I.shape[0] if Q is None else Q.shape[0], 1 << 22), 1))
    try:
        ctx.set_index(I, r)
        return ctx.normals_self(k, viewpoint) if Q is None else ctx.normals(Q, k, viewpoint)
    finally:
        ctx.close()


def estimate_normals(xyzi, k, r, viewpoint=None, device=False):
    """(nc float32 [n, 4], dist float32 [n]) of a cloud against itself: every point's neighbourhood holds the point.  device=True runs
    scaloam.RadiusIndex.normals_self; the results are equal bit for bit."""
    P = _xyzi(xyzi)
    k = _normal_k(k)
    _radius(r)
    vp = _viewpoint(viewpoint)
    return _device_normals(P, None, k, r, vp) if device else normals_within(P, P, k, r, vp)


def point_to_plane(map_xyzi, cloud_xyzi, k, r, device=False):
    """(dist float32 [n], valid bool [n]): the signed distance of every cloud point to the local plane of the map - the plane through
    the point's k nearest map records within r - and where one exists (at least 3 such records; dist is NaN elsewhere).  The sign
    follows the unoriented normal: |dist| is the residual.  residual_stats summarises the pair."""
    M, P = _xyzi(map_xyzi), _xyzi(cloud_xyzi)
    k = _normal_k(k)
    _radius(r)
    _, dist = _device_normals(M, P, k, r, None) if device else normals_within(M, P, k, r)
    return dist, dist.view(np.uint32) != NAN_BITS


def residual_stats(dist, valid):
    """of point_to_plane's result, in f64 on the host whichever path made it: dict(valid, points, mean_abs, rms, median_abs), the
    last three None without a valid point"""
    dist, valid = np.asarray(dist, np.float32).reshape(-1), np.asarray(valid, bool).reshape(-1)
    a = np.abs(dist[valid].astype(np.float64))
    return dict(valid=int(valid.sum()), points=int(dist.shape[0]), mean_abs=float(a.mean()) if a.size else None,
                rms=float(np.sqrt((a * a).mean())) if a.size else None, median_abs=float(np.median(a)) if a.size else None)


def map_diff(map_x, map_y, scans_y, poses12_y, r=DEFAULT_RADIUS, device=False, **removert_settings):
    """What is in map X and not in map Y, for two maps in one frame, and whether session Y saw through that place.
    scans_y, poses12_y: Y's keyframes (sensor frame, sensor to world), as scaloam.removert.remove_dynamic_points takes them, and
    removert_settings its keyword arguments (remove_res, revert_res, fov_up_deg, fov_down_deg, min_range, max_range, diff_thres,
    min_hits).  Returns (labels uint8 [N_x], stats): COMMON 0 - a Y point lies within r; UNOBSERVED 1 - none does and no ray of Y
    went through the point; CHANGED 2 - none does and remove_dynamic_points, run on these points alone against Y's keyframes, flags
    it.  From the old map towards the new session 2 reads "disappeared"; from the new map towards the old session it reads
    "appeared" and 1 "newly explored".  stats: common, unobserved, changed, candidates, removert (its stats) and margin - the
    restatement's Removert margin (removert.View.pixels) on the candidates, None on the device path, inf without candidates.
    On the device the candidates go through the host between scaloam.RadiusIndex and scaloam.Removert: they are a small share of the map."""
    X, Y = _xyzi(map_x), _xyzi(map_y)
    P = np.asarray(poses12_y, np.float64).reshape(-1, 12)
    if P.shape[0] != len(scans_y):
        raise ValueError("one pose12 row per scan is needed")
    count, _ = _device_counts(Y, X, r) if device else radius_counts(Y, X, r)
    labels = np.zeros(X.shape[0], np.uint8)
    cand = np.flatnonzero(count == 0)
    margin, rstats = (None if device else np.inf), None
    if cand.size:
        if device:
            from . import Removert
            kw = dict(removert_settings)
            rm_res, rv_res = kw.pop("remove_res", _rv.DEFAULT_REMOVE_RES), kw.pop("revert_res", _rv.DEFAULT_REVERT_RES)
            rm = Removert(max_points=cand.size, max_keyframes=max(len(scans_y), 1), max_scan_points=max(sum(len(s) for s in scans_y), 1),
                          max_resolutions=max(len(rm_res) + len(rv_res), 1), **kw)
            try:
                mask, rstats = rm.remove(X[cand], scans_y, P, rm_res, rv_res)
            finally:
                rm.close()
        else:
            res = _rv.remove_dynamic_points(X[cand], scans_y, P, keep_images=False, **removert_settings)
            mask, rstats, margin = res.mask, res.stats, res.margin
        labels[cand] = UNOBSERVED + mask.astype(np.uint8)
    n2 = int((labels == CHANGED).sum())
    stats = dict(common=int(X.shape[0] - cand.size), unobserved=int(cand.size - n2), changed=n2, candidates=int(cand.size), removert=rstats,
                 margin=margin)
    return labels, stats


def update_map(map_old, labels_old, map_new, labels_new):
    """the old points that did not disappear, in order, followed by the new points the old map does not already hold, in order"""
    A, B = _xyzi(map_old), _xyzi(map_new)
    la, lb = np.asarray(labels_old).reshape(-1), np.asarray(labels_new).reshape(-1)
    if la.shape[0] != A.shape[0] or lb.shape[0] != B.shape[0]:
        raise ValueError("one label per point is needed")
    return np.concatenate([A[la != CHANGED], B[lb != COMMON]], 0)
