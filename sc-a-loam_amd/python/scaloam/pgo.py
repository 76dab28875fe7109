"""Host-side glue of the pose-graph node around the hot path (laserPosegraphOptimization.cpp): the keyframe gate in front of the
ScanContext insert (:598-617, with getOdom :312-323 and diffTransformation :325-336) and the g2o text of the saved pose graph
(:147-175, :198-216), and - further down - the CPU restatement of the pose graph and its batch optimisation that csrc/posegraph.hip is
held to.  No GPU work here; GTSAM / iSAM2 itself is third-party code and is restated, not reproduced."""
import numpy as np


def rpy_from_quat(q_xyzw):
    """tf::Matrix3x3(tf::Quaternion).getRPY (:318-320), in double"""
    x, y, z, w = [float(v) for v in q_xyzw]
    n = x * x + y * y + z * z + w * w
    s = 2.0 / n
    m = np.array([[1 - s * (y * y + z * z), s * (x * y - w * z), s * (x * z + w * y)],
                  [s * (x * y + w * z), 1 - s * (x * x + z * z), s * (y * z - w * x)],
                  [s * (x * z - w * y), s * (y * z + w * x), 1 - s * (x * x + y * y)]])
    if abs(m[2, 0]) >= 1.0:  # gimbal lock branch of tf's getEulerYPR
        yaw = 0.0
        if m[2, 0] < 0:
            pitch, roll = np.pi / 2, np.arctan2(m[0, 1], m[0, 2])
        else:
            pitch, roll = -np.pi / 2, np.arctan2(-m[0, 1], -m[0, 2])
        return roll, pitch, yaw
    pitch = -np.arcsin(m[2, 0])
    roll = np.arctan2(m[2, 1] / np.cos(pitch), m[2, 2] / np.cos(pitch))
    yaw = np.arctan2(m[1, 0] / np.cos(pitch), m[0, 0] / np.cos(pitch))
    return roll, pitch, yaw


def _affine_f32(x, y, z, roll, pitch, yaw):
    """pcl::getTransformation (f32 Affine3f: R = Rz(yaw) Ry(pitch) Rx(roll))"""
    A, B, C_, D, E, F = (np.float32(np.cos(yaw)), np.float32(np.sin(yaw)), np.float32(np.cos(pitch)), np.float32(np.sin(pitch)),
                         np.float32(np.cos(roll)), np.float32(np.sin(roll)))
    DE, DF = D * E, D * F
    T = np.eye(4, dtype=np.float32)
    T[0, :3] = [A * C_, A * DF - B * E, B * F + A * DE]
    T[1, :3] = [B * C_, A * E + B * DF, B * DE - A * F]
    T[2, :3] = [-D, C_ * F, C_ * E]
    T[:3, 3] = [x, y, z]
    return T


def diff_transformation(p1, p2):
    """diffTransformation (:325-336): |dx|,|dy|,|dz|,|droll|,|dpitch|,|dyaw| of p1^-1 * p2, f32 as in the reference"""
    d = (np.linalg.inv(_affine_f32(*p1)) @ _affine_f32(*p2)).astype(np.float32)
    droll = np.arctan2(d[2, 1], d[2, 2])
    dpitch = np.arcsin(-d[2, 0])
    dyaw = np.arctan2(d[1, 0], d[0, 0])
    return np.abs(np.array([d[0, 3], d[1, 3], d[2, 3], droll, dpitch, dyaw], np.float64))


class KeyframeGate:
    """Early reject by counting local delta movement (:598-617).  The accumulators start at 1000000 (:67-68), so the first pose is
    always a keyframe."""

    def __init__(self, meter_gap=2.0, deg_gap=10.0):
        self.meter_gap = float(meter_gap)
        self.rad_gap = np.deg2rad(float(deg_gap))  # :875-876
        self.tr = 1000000.0
        self.rot = 1000000.0
        self.curr = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)  # odom_pose_curr {0.0, ...} (:75)

    def __call__(self, q_xyzw, t_xyz):
        pose = (float(t_xyz[0]), float(t_xyz[1]), float(t_xyz[2])) + tuple(rpy_from_quat(q_xyzw))
        prev, self.curr = self.curr, pose
        d = diff_transformation(prev, self.curr)
        self.tr += float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
        self.rot += float(d[3] + d[4] + d[5])
        if self.tr > self.meter_gap or self.rot > self.rad_gap:
            self.tr, self.rot = 0.0, 0.0
            return True
        return False


def _f6(v):
    return "%f" % v  # std::to_string(double)


def quat_from_rpy(roll, pitch, yaw):
    """gtsam::Rot3::RzRyRx(roll, pitch, yaw).toQuaternion() (:193-196), (x, y, z, w)"""
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return (sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy)


def g2o_vertex(idx, t, q_xyzw):
    """getVertexStr (:147-161)"""
    return "VERTEX_SE3:QUAT %d %s %s %s %s %s %s %s" % ((idx,) + tuple(_f6(v) for v in (t[0], t[1], t[2], q_xyzw[0], q_xyzw[1], q_xyzw[2], q_xyzw[3])))


def g2o_edge(i, j, t, q_xyzw):
    """writeEdge (:163-176)"""
    return "EDGE_SE3:QUAT %d %d %s %s %s %s %s %s %s" % ((i, j) + tuple(_f6(v) for v in (t[0], t[1], t[2], q_xyzw[0], q_xyzw[1], q_xyzw[2], q_xyzw[3])))


def write_g2o(path, keyframe_poses6d, edges):
    """saveGTSAMgraphG2oFormat (:198-216): one vertex per keyframe pose (x, y, z, roll, pitch, yaw), then the edge lines as collected
    (odometry edges :668-683, loop edges :759-771); edges = [(i, j, t_xyz, q_xyzw), ...]"""
    with open(path, "w") as f:
        for k, p in enumerate(keyframe_poses6d):
            f.write(g2o_vertex(k, p[:3], quat_from_rpy(p[3], p[4], p[5])) + "\n")
        for i, j, t, q in edges:
            f.write(g2o_edge(i, j, t, q) + "\n")


def read_g2o(path):
    """vertices {idx: (t, q_xyzw)} and edges [(i, j, t, q_xyzw)] of a singlesession_posegraph.g2o"""
    V, E = {}, []
    for ln in open(path):
        w = ln.split()
        if not w:
            continue
        if w[0] == "VERTEX_SE3:QUAT":
            v = [float(x) for x in w[2:9]]
            V[int(w[1])] = (np.array(v[:3]), np.array(v[3:]))
        elif w[0] == "EDGE_SE3:QUAT":
            v = [float(x) for x in w[3:10]]
            E.append((int(w[1]), int(w[2]), np.array(v[:3]), np.array(v[3:])))
    return V, E


def local2global_f32(xyzi, pose6):
    """local2global (:338-359): the cloud moved by pcl::getTransformation(pose6) in f32, each coordinate ((T0 x + T1 y) + T2 z) + T3 rounded
    operation by operation; intensity kept"""
    T = _affine_f32(*pose6)
    p = np.asarray(xyzi, np.float32)
    out = p.copy()
    for r in range(3):
        out[:, r] = ((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3]
    return out


def pgo_map_cloud(clouds, poses6, n_own, skip):
    """pubMap's cloud before its VoxelGrid (:815-822): own keyframes 0, skip, 2 skip, ... below n_own (the keyframes with database index
    < kf_end, counted from the pipeline's first own keyframe: n_own = kf_end - pre-filled entries), each moved by its pose with local2global's
    f32 arithmetic, concatenated in keyframe order"""
    parts = [local2global_f32(clouds[j], poses6[j]) for j in range(0, max(0, int(n_own)), int(skip))]
    return np.concatenate(parts).astype(np.float32) if parts else np.zeros((0, 4), np.float32)


def _quat_from_matrix(m):
    """Eigen::Quaterniond(Matrix3d) (gtsam Rot3::toQuaternion), (x, y, z, w)"""
    q = np.zeros(4)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        s = np.sqrt(t + 1.0)
        q[3] = 0.5 * s
        s = 0.5 / s
        q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * s, (m[0, 2] - m[2, 0]) * s, (m[1, 0] - m[0, 1]) * s
        return q
    i = 0
    if m[1, 1] > m[0, 0]:
        i = 1
    if m[2, 2] > m[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    s = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
    q[i] = 0.5 * s
    s = 0.5 / s
    q[3] = (m[k, j] - m[j, k]) * s
    q[j] = (m[j, i] + m[i, j]) * s
    q[k] = (m[k, i] + m[i, k]) * s
    return q


def relative_pose_from_icp(T):
    """doICPVirtualRelative's return value (:536-547): pcl::getTranslationAndEulerAngles of the f32 ICP transform, poseFrom =
    Pose3(Rot3::RzRyRx(roll, pitch, yaw), (x, y, z)), poseFrom.between(identity) -> (q_xyzw, t) in double"""
    T = np.asarray(T, np.float64).reshape(4, 4).astype(np.float32)
    x, y, z = T[0, 3], T[1, 3], T[2, 3]
    roll, pitch, yaw = np.arctan2(T[2, 1], T[2, 2]), np.arcsin(-T[2, 0]), np.arctan2(T[1, 0], T[0, 0])
    cr, sr, cp, sp, cy, sy = (np.cos(float(roll)), np.sin(float(roll)), np.cos(float(pitch)), np.sin(float(pitch)),
                              np.cos(float(yaw)), np.sin(float(yaw)))
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    R = Rz @ Ry @ Rx
    Rt = R.T
    t = -(Rt @ np.array([float(x), float(y), float(z)]))
    return _quat_from_matrix(Rt), t


# ------------------------------------------------------------------------------------------------ pose-graph optimisation
# CPU restatement of the pose graph the node builds (initNoises :284-310, process_pg :644-690, process_icp :761-768) and of a batch
# Gauss-Newton optimiser over it: the yardstick of csrc/posegraph.hip.  Poses are pose7 rows (qx qy qz qw tx ty tz, the layout
# scal_factors_eval uses); tangent vectors are [omega, v] (rotation first, as GTSAM's Pose3); Exp / Log are the full SE(3) maps.
# Parity with GTSAM is unpinned: which Pose3 chart the reference's build used cannot be found out.
SERIES_THETA = 0.1     # below: the coefficient functions of Exp / Log / Jr^-1 by their series (4 terms, error < 1e-15 relative)
SERIES_SINE = 1e-4     # below (|vector part| of the quaternion): atan by its series in the rotation logarithm
PG_DEFAULTS = dict(max_iterations=50, step_tol=1e-8, lambda_first=1e-4, lambda_factor=10.0, lambda_max=1e8,
                   linear="splu", linear_rtol=1e-12, max_linear_iterations=2000)
PRIOR_VARIANCES = (1e-12,) * 6                              # :286-288
ODOM_VARIANCES = (1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4)       # :292
LOOP_VARIANCES = (0.5,) * 6                                 # :295
LOOP_CAUCHY_K = 1.0                                         # :297


def _hat(w):
    w = np.asarray(w, np.float64)
    H = np.zeros(w.shape[:-1] + (3, 3))
    H[..., 0, 1], H[..., 0, 2], H[..., 1, 0] = -w[..., 2], w[..., 1], w[..., 2]
    H[..., 1, 2], H[..., 2, 0], H[..., 2, 1] = -w[..., 0], -w[..., 1], w[..., 0]
    return H


def _qmul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], -1)


def _qconj(q):
    return q * np.array([-1.0, -1.0, -1.0, 1.0])


def _qmat(q):
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)
    return R


def _coeffs(th2):
    """the coefficient functions of theta (given theta^2): a = (1 - cos)/t^2, b = (t - sin)/t^3, c = (1 - (t/2) cot(t/2))/t^2,
    c2 = (t^2 + 2 cos - 2)/(2 t^4), c3 = (2 t - 3 sin + t cos)/(2 t^5); series below SERIES_THETA"""
    th2 = np.asarray(th2, np.float64)
    small = th2 < SERIES_THETA * SERIES_THETA
    t2 = np.where(small, 1.0, th2)
    t = np.sqrt(t2)
    s, co = np.sin(t), np.cos(t)
    a = (1 - co) / t2
    b = (t - s) / (t2 * t)
    c = (1 - 0.5 * t * np.cos(0.5 * t) / np.sin(0.5 * t)) / t2
    c2 = (t2 + 2 * co - 2) / (2 * t2 * t2)
    c3 = (2 * t - 3 * s + t * co) / (2 * t2 * t2 * t)
    x = np.where(small, th2, 0.0)
    a = np.where(small, 1 / 2 + x * (-1 / 24 + x * (1 / 720 - x / 40320)), a)
    b = np.where(small, 1 / 6 + x * (-1 / 120 + x * (1 / 5040 - x / 362880)), b)
    c = np.where(small, 1 / 12 + x * (1 / 720 + x * (1 / 30240 + x / 1209600)), c)
    c2 = np.where(small, 1 / 24 + x * (-1 / 720 + x * (1 / 40320 - x / 3628800)), c2)
    c3 = np.where(small, 1 / 120 + x * (-1 / 2520 + x * (1 / 120960 - x / 9979200)), c3)
    return a, b, c, c2, c3


def se3_exp(xi):
    """Exp of [omega, v] (shape (..., 6)) -> pose7: q = (sin(t/2)/t omega, cos(t/2)), t = V(omega) v, V = I + a W + b W^2"""
    xi = np.asarray(xi, np.float64)
    w, v = xi[..., :3], xi[..., 3:]
    th2 = np.sum(w * w, -1)
    a, b, _, _, _ = _coeffs(th2)
    small = th2 < SERIES_THETA * SERIES_THETA
    t = np.sqrt(np.where(small, 1.0, th2))
    x = np.where(small, th2, 0.0)
    sh = np.where(small, 1 / 2 + x * (-1 / 48 + x * (1 / 3840 - x / 645120)), np.sin(0.5 * t) / t)
    ch = np.where(small, 1 + x * (-1 / 8 + x * (1 / 384 - x / 46080)), np.cos(0.5 * t))
    wv = np.cross(w, v)
    wwv = np.cross(w, wv)
    tr = v + a[..., None] * wv + b[..., None] * wwv
    return np.concatenate([sh[..., None] * w, ch[..., None], tr], -1)


def _rot_log(q):
    """rotation vector of a unit quaternion (x y z w), angle in [0, pi]"""
    q = np.where(q[..., 3:4] < 0, -q, q)
    v, w = q[..., :3], q[..., 3]
    s2 = np.sum(v * v, -1)
    small = s2 < SERIES_SINE * SERIES_SINE
    s = np.sqrt(np.where(small, 1.0, s2))
    k = 2 * np.arctan2(s, w) / s
    x = np.where(small, s2 / (w * w), 0.0)
    k = np.where(small, 2 / w * (1 + x * (-1 / 3 + x / 5)), k)
    return k[..., None] * v


def se3_log(p):
    """Log of pose7 -> [omega, v]: v = V^-1 t, V^-1 = I - W/2 + c W^2"""
    p = np.asarray(p, np.float64)
    w = _rot_log(p[..., :4])
    t = p[..., 4:]
    _, _, c, _, _ = _coeffs(np.sum(w * w, -1))
    wt = np.cross(w, t)
    return np.concatenate([w, t - 0.5 * wt + c[..., None] * np.cross(w, wt)], -1)


def se3_compose(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    q = _qmul(a[..., :4], b[..., :4])
    t = a[..., 4:] + np.einsum("...rc,...c->...r", _qmat(a[..., :4]), b[..., 4:])
    return np.concatenate([q, t], -1)


def se3_inverse(a):
    a = np.asarray(a, np.float64)
    qi = _qconj(a[..., :4])
    return np.concatenate([qi, -np.einsum("...cr,...c->...r", _qmat(a[..., :4]), a[..., 4:])], -1)


def se3_between(a, b):
    """a^-1 b (gtsam Pose3::between)"""
    return se3_compose(se3_inverse(a), b)


def se3_adjoint(p):
    """Ad(T) for [omega, v]: [[R, 0], [t^ R, R]]"""
    p = np.asarray(p, np.float64)
    R = _qmat(p[..., :4])
    A = np.zeros(p.shape[:-1] + (6, 6))
    A[..., :3, :3] = R
    A[..., 3:, 3:] = R
    A[..., 3:, :3] = _hat(p[..., 4:]) @ R
    return A


def se3_right_jacobian_inverse(xi):
    """Jr^-1(xi) = Jl^-1(-xi), Jl^-1 = [[J, 0], [-J Q J, J]] with J = I - W/2 + c W^2 and Q as in Barfoot, State Estimation for
    Robotics, eq. 7.86 (phi = omega, rho = v)"""
    xi = -np.asarray(xi, np.float64)
    w, v = xi[..., :3], xi[..., 3:]
    _, b, c, c2, c3 = _coeffs(np.sum(w * w, -1))
    W, V = _hat(w), _hat(v)
    I = np.eye(3)
    J = I - 0.5 * W + c[..., None, None] * (W @ W)
    WV, VW = W @ V, V @ W
    WVW = WV @ W
    Q = (0.5 * V + b[..., None, None] * (WV + VW + WVW) + c2[..., None, None] * (W @ WV + VW @ W - 3 * WVW)
         + c3[..., None, None] * (WVW @ W + W @ WVW))
    out = np.zeros(xi.shape[:-1] + (6, 6))
    out[..., :3, :3] = J
    out[..., 3:, 3:] = J
    out[..., 3:, :3] = -(J @ Q @ J)
    return out


def between_residual(Ti, Tj, Z, jacobians=False):
    """r = Log(Z^-1 Ti^-1 Tj); with jacobians the derivatives for right perturbations T <- T Exp(d): dr/ddj = Jr^-1(r),
    dr/ddi = -Jr^-1(r) Ad((Ti^-1 Tj)^-1)"""
    rel = se3_between(Ti, Tj)
    r = se3_log(se3_between(Z, rel))
    if not jacobians:
        return r
    Jj = se3_right_jacobian_inverse(r)
    Ji = -(Jj @ se3_adjoint(se3_inverse(rel)))
    return r, Ji, Jj


def prior_residual(T, P, jacobians=False):
    """r = Log(P^-1 T), dr/dd = Jr^-1(r)"""
    r = se3_log(se3_between(P, T))
    return (r, se3_right_jacobian_inverse(r)) if jacobians else r


def se3_retract(T, d):
    p = se3_compose(T, se3_exp(d))
    p[..., :4] /= np.linalg.norm(p[..., :4], axis=-1, keepdims=True)
    return p


def pose7_from_pose6(p6):
    """x y z roll pitch yaw (Pose6D) -> pose7, Pose6DtoGTSAMPose3 (:193-196)"""
    p6 = np.asarray(p6, np.float64).reshape(-1, 6)
    return np.array([list(quat_from_rpy(p[3], p[4], p[5])) + [p[0], p[1], p[2]] for p in p6]).reshape(-1, 7)


def pose6_from_pose7(p7):
    """pose7 -> x y z roll pitch yaw with RzRyRx(roll, pitch, yaw) = the rotation (updatePoses, :408-431)"""
    p7 = np.asarray(p7, np.float64).reshape(-1, 7)
    return np.array([[p[4], p[5], p[6]] + list(rpy_from_quat(p[:4])) for p in p7]).reshape(-1, 6)


def make_edges(i, j, z, variances, cauchy_k):
    """between edges as the arrays scal_posegraph_add_between takes; cauchy_k 0 = not robust"""
    i = np.asarray(i, np.int32).reshape(-1)
    m = len(i)
    return dict(i=i, j=np.asarray(j, np.int32).reshape(-1), z=np.asarray(z, np.float64).reshape(m, 7),
                var=np.broadcast_to(np.asarray(variances, np.float64), (m, 6)).copy(),
                k=np.broadcast_to(np.asarray(cauchy_k, np.float64), (m,)).copy())


def concat_edges(a, b):
    return {key: np.concatenate([a[key], b[key]]) for key in ("i", "j", "z", "var", "k")}


def whitened_residuals(poses, prior, edges, jacobians=False):
    """e = r / sigma for the prior (first) and every edge, the robust weights w = k^2 / (k^2 + |e|^2) (1 where k = 0) and the cost
    sum(|e|^2 / 2) over the plain rows + sum(k^2 / 2 log(1 + |e|^2 / k^2)) over the robust ones"""
    poses = np.asarray(poses, np.float64)
    sp = 1.0 / np.sqrt(np.asarray(prior["var"], np.float64))
    se = 1.0 / np.sqrt(edges["var"])
    Ti, Tj = poses[edges["i"]], poses[edges["j"]]
    if jacobians:
        rp, Jp = prior_residual(poses[prior["node"]], np.asarray(prior["pose7"], np.float64), True)
        r, Ji, Jj = between_residual(Ti, Tj, edges["z"], True)
    else:
        rp = prior_residual(poses[prior["node"]], np.asarray(prior["pose7"], np.float64))
        r = between_residual(Ti, Tj, edges["z"])
    ep, e = rp * sp, r * se
    e2 = np.sum(e * e, -1)
    k2 = edges["k"] * edges["k"]
    robust = k2 > 0
    k2s = np.where(robust, k2, 1.0)
    w = np.where(robust, k2s / (k2s + e2), 1.0)
    cost = 0.5 * float(ep @ ep) + float(np.sum(np.where(robust, 0.5 * k2s * np.log1p(e2 / k2s), 0.5 * e2)))
    if not jacobians:
        return ep, e, w, cost
    return ep, e, w, cost, Jp * sp[:, None], Ji * se[:, :, None], Jj * se[:, :, None]


# ---- the device's linear solver restated (csrc/posegraph.hip: k_pg_assemble, k_pg_offdiag, k_pg_pcr_*, solve()): numpy only.
# H is kept the way the device keeps it: the diagonal blocks D[n] and one block O[e] = A_i^T A_j per between edge, H[i, j] += O[e],
# H[j, i] += O[e]^T.  The same algorithm in the same order of steps, not the same bits: sums run in numpy's order.
def _blocks(n, prior, edges, w, ep, e, Jp, Ji, Jj):
    sw = np.sqrt(w)
    Ai, Aj, b = Ji * sw[:, None, None], Jj * sw[:, None, None], e * sw[:, None]
    ei, ej = edges["i"].astype(np.int64), edges["j"].astype(np.int64)
    D, g = np.zeros((n, 6, 6)), np.zeros((n, 6))
    pn = int(prior["node"])
    D[pn] += Jp.T @ Jp
    g[pn] += Jp.T @ ep
    np.add.at(D, ei, np.einsum("eki,ekj->eij", Ai, Ai))
    np.add.at(D, ej, np.einsum("eki,ekj->eij", Aj, Aj))
    np.add.at(g, ei, np.einsum("eki,ek->ei", Ai, b))
    np.add.at(g, ej, np.einsum("eki,ek->ei", Aj, b))
    return dict(D=D, i=ei, j=ej, O=np.einsum("eki,ekj->eij", Ai, Aj)), g


def normal_blocks(poses, prior, edges, lam=0.0):
    """H = J^T J in 6x6 blocks (dict: D[n, 6, 6] the diagonal blocks, i, j, O[m, 6, 6] with H[i, j] += O, H[j, i] += O^T per edge) and
    g = J^T b as [n, 6], robust rows scaled by sqrt(w) as optimize_pose_graph does; damping lam * diag(H) on the diagonal"""
    poses = np.asarray(poses, np.float64).reshape(-1, 7)
    ep, e, w, _, Jp, Ji, Jj = whitened_residuals(poses, prior, edges, True)
    H, g = _blocks(len(poses), prior, edges, w, ep, e, Jp, Ji, Jj)
    return damped_blocks(H, lam), g


def damped_blocks(H, lam):
    """H + lam diag(H) (k_pg_assemble: d += lambda * d on the diagonal)"""
    if lam == 0:
        return H
    D = H["D"].copy()
    k = np.arange(6)
    D[:, k, k] += lam * D[:, k, k]
    return dict(H, D=D)


def blocks_matvec(H, p):
    """H p for p [n, 6] (k_pg_hp)"""
    q = np.einsum("nij,nj->ni", H["D"], p)
    np.add.at(q, H["i"], np.einsum("eij,ej->ei", H["O"], p[H["j"]]))
    np.add.at(q, H["j"], np.einsum("eji,ej->ei", H["O"], p[H["i"]]))
    return q


def blocks_dense(H, tridiagonal=False):
    """H as a dense [6 n, 6 n] matrix; tridiagonal: only M, the diagonal blocks and the blocks between neighbouring nodes"""
    n = len(H["D"])
    A = np.zeros((n, 6, n, 6))
    k = np.arange(n)
    A[k, :, k, :] = H["D"]
    for a, b, O in zip(H["i"], H["j"], H["O"]):
        if tridiagonal and abs(int(a) - int(b)) != 1:
            continue
        A[a, :, b, :] += O
        A[b, :, a, :] += O.T
    return A.reshape(6 * n, 6 * n)


def _upper_blocks(H):
    """U[k] = H[k, k + 1] (k_pg_assemble's block towards node + 1; zero for the last node, k_pg_pcr_init)"""
    n = len(H["D"])
    U = np.zeros((n, 6, 6))
    fwd, bwd = H["j"] == H["i"] + 1, H["i"] == H["j"] + 1
    np.add.at(U, H["i"][fwd], H["O"][fwd])
    np.add.at(U, H["j"][bwd], np.swapaxes(H["O"][bwd], 1, 2))
    return U


def pcr_factor(H):
    """Parallel cyclic reduction of M, the block-tridiagonal part of H (rows L_i, D_i, U_i, L_i = U_{i-1}^T), as k_pg_pcr_init and
    k_pg_pcr_level do it: levels s = 1, 2, 4, ... while s < n, every row in each: alpha = L_i Dinv_{i-s}, gamma = U_i Dinv_{i+s},
    D' = D - alpha U_{i-s} - gamma L_{i+s}, L' = -alpha L_{i-s}, U' = -gamma U_{i+s} (terms whose row does not exist are left out).
    Returns the multipliers of every level and the last level's Dinv."""
    D = H["D"].copy()
    n = len(D)
    U = _upper_blocks(H)
    L = np.zeros_like(U)
    L[1:] = np.swapaxes(U[:-1], 1, 2)
    Di = np.linalg.inv(D)
    levels, s = [], 1
    while s < n:
        al, ga = np.zeros_like(D), np.zeros_like(D)
        al[s:] = L[s:] @ Di[:-s]
        ga[:-s] = U[:-s] @ Di[s:]
        Dn, Ln, Un = D.copy(), np.zeros_like(D), np.zeros_like(D)
        Dn[s:] -= al[s:] @ U[:-s]
        Ln[s:] = -(al[s:] @ L[:-s])
        Dn[:-s] -= ga[:-s] @ L[s:]
        Un[:-s] = -(ga[:-s] @ U[s:])
        D, L, U = Dn, Ln, Un
        Di = np.linalg.inv(D)
        levels.append((s, al, ga))
        s *= 2
    return dict(levels=levels, Dinv=Di)


def pcr_solve(factor, r):
    """M^-1 r for r [n, 6]: per level out_i = in_i - alpha_i in_{i-s} - gamma_i in_{i+s} (k_pg_pcr_apply), then Dinv_i in_i
    (k_pg_pcr_final)"""
    v = np.array(r, np.float64).reshape(-1, 6)
    for s, al, ga in factor["levels"]:
        out = v.copy()
        out[s:] -= np.einsum("nij,nj->ni", al[s:], v[:-s])
        out[:-s] -= np.einsum("nij,nj->ni", ga[:-s], v[s:])
        v = out
    return np.einsum("nij,nj->ni", factor["Dinv"], v)


def pcg_solve(H, g, rtol=1e-12, max_iterations=2000):
    """H d = -g by conjugate gradients preconditioned with pcr_solve, the loop of solve() in csrc/posegraph.hip: stop when
    r . M^-1 r <= rtol^2 times its first value.  Returns d [n, 6], the iterations and the status (0 met the tolerance, 1 the bound
    hit, 2 breakdown: a curvature or r . M^-1 r that is not positive and finite)."""
    g = np.asarray(g, np.float64).reshape(-1, 6)
    F = pcr_factor(H)
    d, r = np.zeros_like(g), -g
    z = pcr_solve(F, r)
    rz = rz0 = float(np.sum(r * z))
    if not rz > 0:
        return d, 0, (0 if rz == 0 else 2)
    p, it = z, 0
    while True:
        q = blocks_matvec(H, p)
        pq = float(np.sum(p * q))
        if not (pq > 0 and np.isfinite(pq)):
            return d, it, 2
        a = rz / pq
        d = d + a * p
        r = r - a * q
        z = pcr_solve(F, r)
        rzn = float(np.sum(r * z))
        it += 1
        if not np.isfinite(rzn) or rzn < 0:
            return d, it, 2
        beta, rz = rzn / rz, rzn
        if rz <= rtol * rtol * rz0:
            return d, it, 0
        if it >= max_iterations:
            return d, it, 1
        p = z + beta * p


def optimize_pose_graph(poses, prior, edges, params=None):
    """Batch Gauss-Newton over the graph, robust rows reweighted as gtsam's noiseModel::Robust does (row block and right-hand side
    times sqrt(w), no second-order term); exact sparse solve of the normal equations.  A step that raises the cost is rejected and
    solved again with Levenberg damping lambda diag(H) (lambda_first, then times lambda_factor); damping is dropped after an accepted
    step.  Stops (converged) when a step's max-norm is below step_tol.  Returns poses, stats(costs per iteration starting with the
    initial one, step_norms, weights at the returned estimate, iterations, converged, trials: (cost, trial cost, step, accepted) of
    every solve, rejected: (cost, trial cost) of the rejected ones).  params linear="pcg" solves with pcg_solve (linear_rtol,
    max_linear_iterations) in place of splu, as the device does: a solve that does not meet its tolerance ends the run with the
    last accepted poses; linear_iterations is summed over the solves."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    P = dict(PG_DEFAULTS)
    P.update(params or {})
    if P["linear"] not in ("splu", "pcg"):
        raise ValueError("linear is 'splu' or 'pcg'")
    x = np.array(poses, np.float64).reshape(-1, 7)
    n, m = len(x), len(edges["i"])
    _, _, _, cost = whitened_residuals(x, prior, edges)
    costs, steps = [cost], []
    converged, lam, it = 0, 0.0, 0
    pcg, lin_its, lin_status, trials = P["linear"] == "pcg", 0, 0, []
    ar6 = np.arange(6)
    rows_e = (6 * np.arange(m)[:, None, None] + ar6[None, :, None] + 6) + np.zeros((1, 1, 6), np.int64)
    cols_i = 6 * edges["i"].astype(np.int64)[:, None, None] + ar6[None, None, :] + np.zeros((1, 6, 1), np.int64)
    cols_j = 6 * edges["j"].astype(np.int64)[:, None, None] + ar6[None, None, :] + np.zeros((1, 6, 1), np.int64)
    rows_p = ar6[:, None] + np.zeros((1, 6), np.int64)
    cols_p = 6 * int(prior["node"]) + ar6[None, :] + np.zeros((6, 1), np.int64)
    while it < P["max_iterations"]:
        ep, e, w, cost, Jp, Ji, Jj = whitened_residuals(x, prior, edges, True)
        sw = np.sqrt(w)
        b = np.concatenate([ep, (e * sw[:, None]).reshape(-1)])
        J = sp.csr_matrix((np.concatenate([Jp.reshape(-1), (Ji * sw[:, None, None]).reshape(-1), (Jj * sw[:, None, None]).reshape(-1)]),
                           (np.concatenate([rows_p.reshape(-1), rows_e.reshape(-1), rows_e.reshape(-1)]),
                            np.concatenate([cols_p.reshape(-1), cols_i.reshape(-1), cols_j.reshape(-1)]))), shape=(6 * m + 6, 6 * n))
        H = (J.T @ J).tocsc()
        g = J.T @ b
        if pcg:
            Hb, gb = _blocks(n, prior, edges, w, ep, e, Jp, Ji, Jj)
        while True:
            it += 1
            if pcg:
                d, k, lin_status = pcg_solve(damped_blocks(Hb, lam), gb, P["linear_rtol"], P["max_linear_iterations"])
                lin_its += k
                if lin_status != 0:
                    break
            else:
                A = H if lam == 0 else (H + lam * sp.diags(H.diagonal())).tocsc()
                d = spl.splu(A).solve(-g).reshape(n, 6)
            step = float(np.abs(d).max()) if n else 0.0
            xn = se3_retract(x, d)
            _, _, _, cn = whitened_residuals(xn, prior, edges)
            ok = bool(np.isfinite(cn) and cn <= cost)
            trials.append((cost, cn, step, ok))
            if ok:
                x, lam = xn, 0.0
                costs.append(cn)
                steps.append(step)
            else:
                lam = P["lambda_first"] if lam == 0 else lam * P["lambda_factor"]
            if step < P["step_tol"]:
                converged = 1
            if ok or converged or it >= P["max_iterations"] or lam > P["lambda_max"]:
                break
        if converged or lam > P["lambda_max"] or lin_status != 0:
            break
    _, _, w, cost = whitened_residuals(x, prior, edges)
    return x, dict(costs=costs, step_norms=steps, weights=w, iterations=it, converged=converged, final_cost=cost, trials=trials,
                   rejected=[(c, cn) for c, cn, _, ok in trials if not ok],
                   linear_iterations=lin_its, linear_status=lin_status)


def build_pipeline_graph(gated_poses6, loop_records, kf_ids=None):
    """The node's graph over scal_pipeline's own keyframes (node k = the k-th own keyframe): prior on node 0 at its gated pose
    (:286-288, :654), odometry edges (k-1, k) = between of the gated poses (:664-671, :292), one Cauchy(k = 1) loop edge (loop_kf,
    curr_kf) = (q_rel, t_rel) for every record with verified == 1 (:540-547, :765, :295-300).  loop_records: dicts (or objects) with
    verified, curr_kf, loop_kf, q_rel, t_rel; kf_ids: database index of every own keyframe (default 0, 1, ...: no pre-filled
    entries).  Records whose keyframes are not both among kf_ids are left out.  No GPS factors (:673-681): the pipeline has no GPS."""
    p7 = pose7_from_pose6(gated_poses6)
    n = len(p7)
    ids = list(range(n)) if kf_ids is None else [int(v) for v in kf_ids]
    node = {db: k for k, db in enumerate(ids)}
    prior = dict(node=0, pose7=p7[0].copy(), var=np.array(PRIOR_VARIANCES))
    a = np.arange(max(n - 1, 0))
    edges = make_edges(a, a + 1, se3_between(p7[:-1], p7[1:]) if n > 1 else np.zeros((0, 7)), ODOM_VARIANCES, 0.0)
    get = (lambda r, k: r[k]) if (len(loop_records) and isinstance(loop_records[0], dict)) else getattr
    L = [r for r in loop_records if int(get(r, "verified")) == 1 and int(get(r, "curr_kf")) in node and int(get(r, "loop_kf")) in node]
    if L:
        z = np.array([list(get(r, "q_rel")) + list(get(r, "t_rel")) for r in L], np.float64)
        edges = concat_edges(edges, make_edges([node[int(get(r, "loop_kf"))] for r in L], [node[int(get(r, "curr_kf"))] for r in L], z,
                                               LOOP_VARIANCES, LOOP_CAUCHY_K))
    return prior, edges


def synthetic_graph(true6, li, lj, seed=0, noise=1.0, bad_offset=(8.0, -5.0, 1.0), perturb=0.0):
    """Test graph over the true poses true6 (x y z roll pitch yaw): odometry edges with drift (noise scales it; 0 = exact), loop edges
    (li[k], lj[k]) measured from the true poses with small noise, the middle loop's translation displaced by bad_offset (None: all loops
    consistent).  Initial poses: the dead-reckoned odometry, each moved by a random tangent step of size perturb.  Returns initial
    poses, prior, edges, index of the displaced loop among the loop edges (-1: none)."""
    rng = np.random.default_rng(seed)
    T = pose7_from_pose6(true6)
    n, n_loops = len(T), len(li)
    no = np.concatenate([rng.normal(0, 2e-4, (n - 1, 3)) + 1e-4, rng.normal(0, 2e-3, (n - 1, 3))], 1) * noise
    zo = se3_compose(se3_between(T[:-1], T[1:]), se3_exp(no))
    init = np.empty_like(T)
    init[0] = T[0]
    for k in range(1, n):
        init[k] = se3_compose(init[k - 1], zo[k - 1])
    init[:, :4] /= np.linalg.norm(init[:, :4], axis=1, keepdims=True)
    if perturb:
        init[1:] = se3_retract(init[1:], rng.normal(0, perturb, (n - 1, 6)))
    a = np.arange(n - 1)
    edges = make_edges(a, a + 1, zo, ODOM_VARIANCES, 0.0)
    li, lj = np.asarray(li, np.int64), np.asarray(lj, np.int64)
    nl = np.concatenate([rng.normal(0, 1e-3, (n_loops, 3)), rng.normal(0, 1e-2, (n_loops, 3))], 1) * noise
    zl = se3_compose(se3_between(T[li], T[lj]), se3_exp(nl)).reshape(n_loops, 7)
    bad = -1
    if bad_offset is not None and n_loops:
        bad = n_loops // 2
        zl[bad, 4:] += np.asarray(bad_offset)
    if n_loops:
        edges = concat_edges(edges, make_edges(li, lj, zl, LOOP_VARIANCES, LOOP_CAUCHY_K))
    prior = dict(node=0, pose7=T[0].copy(), var=np.array(PRIOR_VARIANCES))
    return init, prior, edges, bad


def two_lap_graph(n_nodes, n_loops, **kw):
    """two laps of a circle (radius 50 m, gentle climb), loops from the second lap onto the first; see synthetic_graph"""
    half = n_nodes // 2
    ang = 2 * np.pi * np.arange(n_nodes) / half
    true6 = np.stack([50 * np.cos(ang), 50 * np.sin(ang), 0.002 * np.arange(n_nodes), 0.01 * np.sin(3 * ang), 0.01 * np.cos(2 * ang), ang + np.pi / 2], 1)
    lj = half + (np.arange(n_loops) * (n_nodes - half - 1)) // max(n_loops, 1) + 1
    return synthetic_graph(true6, lj - half, lj, **kw)


def out_and_back_graph(n_nodes, n_loops, **kw):
    """a straight drive out, a turn and the same way back, loops from the way back onto the outbound leg; see synthetic_graph"""
    half = n_nodes // 2
    k = np.arange(n_nodes)
    x = np.where(k < half, k, 2 * half - k) * 0.5
    yaw = np.where(k < half, 0.0, np.pi)
    true6 = np.stack([x, 0.3 * (k >= half) + 0.0 * k, 0.001 * k, 0.0 * k, 0.005 * np.sin(0.1 * k), yaw], 1)
    lj = half + 2 + (np.arange(n_loops) * (n_nodes - half - 3)) // max(n_loops, 1)
    return synthetic_graph(true6, 2 * half - lj, lj, **kw)


def reverse_edges(edges, which):
    """the same graph with the chosen edges (index array or boolean mask) entered from their other end: (i, j, Z) -> (j, i, Z^-1).
    The reversed residual is -Ad(Z) r: the same zero, but not the same whitened norm, so the optimum is the same only where the
    reversed edges' residuals vanish at it (a consistent graph)."""
    out = {key: edges[key].copy() for key in ("i", "j", "z", "var", "k")}
    sel = np.zeros(len(edges["i"]), bool)
    sel[np.asarray(which)] = True
    out["i"][sel], out["j"][sel] = edges["j"][sel], edges["i"][sel]
    out["z"][sel] = se3_inverse(edges["z"][sel])
    return out


def reorder_edges(edges, order):
    """the same edges added in another order"""
    order = np.asarray(order, np.int64)
    return {key: edges[key][order].copy() for key in ("i", "j", "z", "var", "k")}


def interleave_order(n_odo, n_loops):
    """an add order that spreads the loop edges (n_odo ...) evenly between the odometry edges (0 ... n_odo - 1), the first loop first"""
    at = (np.arange(n_loops) * n_odo) // max(n_loops, 1)
    key = np.concatenate([np.arange(n_odo) + 0.5, at.astype(np.float64)])
    return np.argsort(key, kind="stable")


def prior_at(init, node):
    """a prior (the node's variances) that holds `node` at its initial pose"""
    return dict(node=int(node), pose7=np.array(init[int(node)], np.float64), var=np.array(PRIOR_VARIANCES))


GRAPH_VARIANTS = ("plain", "prior_last", "prior_middle", "prior_displaced", "loops_reversed", "odometry_alternate_reversed", "interleaved",
                  "parallel_loop", "parallel_loop_reversed", "double_loop", "tight_loops", "tight_loops_reversed")


def graph_variant(init, prior, edges, variant):
    """Another form of a synthetic_graph (odometry edges (k, k + 1) first, then the loops) for the tests of the device's index
    handling: the prior on the last or a middle node, or on node 0 but 0.2 rad and 0.4 m away from its initial pose; all loop edges
    or every second odometry edge entered from the other end; the loops spread between the odometry edges in the add order; one more
    Cauchy loop edge on the nodes of odometry edge n // 3 (its measurement, entered as (k, k + 1) or as (k + 1, k)); the first loop
    edge twice; the loops with the odometry's variances and no robust kernel (they carry as much of a step as the chain does: their
    Jacobians show in its leading digits, and H is far from its block-tridiagonal part), also entered from their other end.  Returns
    init, prior, edges."""
    n, m = len(init), len(edges["i"])
    n_odo = n - 1
    if variant == "plain":
        return init, prior, edges
    if variant == "prior_last":
        return init, prior_at(init, n - 1), edges
    if variant == "prior_middle":
        return init, prior_at(init, n // 2), edges
    if variant == "prior_displaced":
        P = dict(prior, pose7=se3_retract(np.asarray(prior["pose7"], np.float64), np.array([0.15, -0.1, 0.09, 0.3, -0.2, 0.15])))
        return init, P, edges
    if variant == "loops_reversed":
        return init, prior, reverse_edges(edges, np.arange(n_odo, m))
    if variant == "odometry_alternate_reversed":
        return init, prior, reverse_edges(edges, np.arange(1, n_odo, 2))
    if variant == "interleaved":
        return init, prior, reorder_edges(edges, interleave_order(n_odo, m - n_odo))
    if variant in ("parallel_loop", "parallel_loop_reversed"):
        k = n // 3
        extra = make_edges([k], [k + 1], edges["z"][k], LOOP_VARIANCES, LOOP_CAUCHY_K)
        if variant == "parallel_loop_reversed":
            extra = reverse_edges(extra, [0])
        return init, prior, concat_edges(edges, extra)
    if variant in ("tight_loops", "tight_loops_reversed"):
        out = {key: edges[key].copy() for key in ("i", "j", "z", "var", "k")}
        out["var"][n_odo:], out["k"][n_odo:] = ODOM_VARIANCES, 0.0
        return init, prior, reverse_edges(out, np.arange(n_odo, m)) if variant == "tight_loops_reversed" else out
    if variant == "double_loop":
        return init, prior, concat_edges(edges, reorder_edges(edges, [n_odo]))
    raise ValueError("unknown variant %r" % (variant,))
