"""Constructed sessions with a known moving object, for the scal_removert tests and tools/bench_removert.py.

constructed_scene: K keyframes near the centre of a static sphere; each also sees a ball that stands somewhere else in every
keyframe.  Scans are ray casts, the map is the union of the scans moved by their poses, the labels are the ball returns.
corridor_session: the same idea inside a long tunnel, so that a map several sensor ranges long exists (culling, benchmark)."""
import numpy as np


def _rz(yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _rays(step_deg, rng):
    """unit directions in the sensor frame over a grid of elevation -25 + step/2 ... 25 - step/2 and azimuth -180 + step/2 ...
    180 - step/2, each angle jittered by +-0.1 step"""
    el = np.arange(-25.0 + step_deg / 2, 25.0, step_deg)
    az = np.arange(-180.0 + step_deg / 2, 180.0, step_deg)
    E, A = np.meshgrid(el, az, indexing="ij")
    E = np.radians(E + rng.uniform(-0.1, 0.1, E.shape) * step_deg).ravel()
    A = np.radians(A + rng.uniform(-0.1, 0.1, A.shape) * step_deg).ravel()
    return np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], 1)


def _hit_sphere(o, d, c, rad, inside):
    """distance along unit rays o + s d to the sphere (c, rad): the far root from inside, the near root from outside; inf = miss"""
    oc = o - c
    b = (d * oc).sum(1)
    disc = b * b - ((oc * oc).sum() - rad * rad)
    root = np.sqrt(np.where(disc >= 0, disc, np.nan))
    s = -b + root if inside else -b - root
    return np.where((disc >= 0) & (s > 0), s, np.inf)


def _pose12(R, t):
    return np.concatenate([R, t.reshape(3, 1)], 1).reshape(12)


def _cast(R, t, dirs, ball_c, ball_rad, statics):
    """one scan: sensor-frame xyzi f32 and which returns are the ball's.  statics: (centre, radius, inside) spheres"""
    dw = dirs @ R.T
    s_static = np.full(dirs.shape[0], np.inf)
    for c, rad, inside in statics:
        s_static = np.minimum(s_static, _hit_sphere(t, dw, np.asarray(c, float), rad, inside))
    s_ball = _hit_sphere(t, dw, ball_c, ball_rad, False)
    s = np.minimum(s_static, s_ball)
    keep = np.isfinite(s)
    pts = (dirs * s[:, None])[keep]
    scan = np.concatenate([pts, np.zeros((pts.shape[0], 1))], 1).astype(np.float32)
    return scan, (s_ball < s_static)[keep]


def _to_world(scan, R, t):
    w = scan[:, :3].astype(np.float64) @ R.T + t
    return np.concatenate([w, scan[:, 3:4].astype(np.float64)], 1).astype(np.float32)


def constructed_scene(K, step_deg=0.5, seed=0):
    """(map [n, 4] f32, scans, poses12 [K, 12], labels bool [n]): keyframe k at a seeded place within +-1 m in x and y and +-0.3 m
    in z, yaw 0.3 k, inside a static sphere of radius 30 m about the origin; its ball of radius 0.5 m stands 10 m from it at
    azimuth 20 deg + k 360 deg / K."""
    rng = np.random.default_rng(seed)
    scans, poses, maps, labels = [], [], [], []
    for k in range(K):
        t = np.concatenate([rng.uniform(-1.0, 1.0, 2), rng.uniform(-0.3, 0.3, 1)])
        R = _rz(0.3 * k)
        a = np.radians(20.0 + k * 360.0 / K)
        scan, lab = _cast(R, t, _rays(step_deg, rng), t + 10.0 * np.array([np.cos(a), np.sin(a), 0.0]), 0.5, [((0, 0, 0), 30.0, True)])
        scans.append(scan), poses.append(_pose12(R, t)), maps.append(_to_world(scan, R, t)), labels.append(lab)
    return np.concatenate(maps, 0), scans, np.array(poses), np.concatenate(labels)


def _hit_tunnel(o, d, rad):
    """distance along unit rays o + s d, from inside, to the wall of the cylinder of radius rad about the x axis; inf = parallel"""
    a = d[:, 1] ** 2 + d[:, 2] ** 2
    b = d[:, 1] * o[1] + d[:, 2] * o[2]
    disc = b * b - a * (o[1] ** 2 + o[2] ** 2 - rad * rad)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(a > 1e-12, (-b + np.sqrt(disc)) / a, np.inf)


def corridor_session(K, spacing=2.0, step_deg=2.0, seed=0, tunnel_radius=15.0):
    """K keyframes `spacing` metres apart along x inside a tunnel (a cylinder about the x axis), heading along it with a slowly
    swinging yaw; each keyframe sees a ball 8 m ahead and to the side, a place the other keyframes look straight through.  Returns
    beyond 150 m are dropped.  Returns (map, scans, poses12, labels)."""
    rng = np.random.default_rng(seed)
    scans, poses, maps, labels = [], [], [], []
    for k in range(K):
        t = np.array([spacing * k + rng.uniform(-0.2, 0.2), rng.uniform(-0.5, 0.5), rng.uniform(-0.1, 0.1)])
        R = _rz(0.2 * np.sin(0.1 * k))
        a = np.radians(25.0 if k % 2 else -25.0)
        dirs = _rays(step_deg, rng)
        dw = dirs @ R.T
        s_static = _hit_tunnel(t, dw, tunnel_radius)
        s_ball = _hit_sphere(t, dw, t + 8.0 * np.array([np.cos(a), np.sin(a), 0.0]), 0.5, False)
        s = np.minimum(s_static, s_ball)
        keep = s <= 150.0
        pts = (dirs * s[:, None])[keep]
        scan = np.concatenate([pts, np.zeros((pts.shape[0], 1))], 1).astype(np.float32)
        scans.append(scan), poses.append(_pose12(R, t)), maps.append(_to_world(scan, R, t)), labels.append((s_ball < s_static)[keep])
    return np.concatenate(maps, 0), scans, np.array(poses), np.concatenate(labels)


def range_edge_scene(max_range=80.0, seed=3):
    """map points just inside and just outside max_range of the one keyframe, on rays whose scan returns lie a little farther out
    (still inside): with a diff_thres of 1e-4 the inside ones are hit, so a culling that lost a pair at the gate would show"""
    rng = np.random.default_rng(seed)
    t, R = np.array([3.0, -2.0, 0.5]), _rz(0.4)
    el, az = np.radians(rng.uniform(-20, 20, 1500)), np.radians(rng.uniform(-180, 180, 1500))
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], 1)
    scan = np.concatenate([d * (max_range * (1.0 - 1e-6)), np.zeros((d.shape[0], 1))], 1).astype(np.float32)
    ranges = max_range + rng.choice([-1e-2, -1e-3, -3e-4, 1e-5, 1e-3, 1e-2], d.shape[0])
    world = (d * ranges[:, None]) @ R.T + t
    mp = np.concatenate([world, np.zeros((d.shape[0], 1))], 1).astype(np.float32)
    return mp, [scan], _pose12(R, t).reshape(1, 12), ranges < max_range - 2e-4


def test_inputs(golden_dir):
    """every input of tests/test_removert_gpu.py, by name: dict(map, scans, poses, labels or None, cfg: Removert settings other than
    the defaults, remove_res, revert_res).  tests/test_removert_cpu.py holds each of them to the margin condition."""
    import os
    out = {}
    for name, K, step in (("scene_k4", 4, 0.5), ("scene_k2", 2, 1.0)):
        mp, scans, P, lab = constructed_scene(K, step, 0)
        for tag, rev in (("", ()), ("_revert", (5.0,))):
            out[name + tag] = dict(map=mp, scans=scans, poses=P, labels=lab, cfg={}, remove_res=(2.5, 2.0, 1.5), revert_res=rev)
    scans = [np.load(os.path.join(golden_dir, f"KAIST03_{k:06d}.npy")).astype(np.float32) for k in (0, 7, 20)]
    P = np.load(os.path.join(golden_dir, "KAIST03_poses21.npy")).reshape(-1, 12).astype(np.float64)[[0, 7, 20]]
    mp = np.concatenate([_to_world(s, p.reshape(3, 4)[:, :3], p.reshape(3, 4)[:, 3]) for s, p in zip(scans, P)], 0)
    for tag, rev in (("", ()), ("_revert", (5.0,))):
        out["kaist" + tag] = dict(map=mp, scans=scans, poses=P, labels=None, cfg={}, remove_res=(2.5, 2.0, 1.5), revert_res=rev)
    # mixed signs, many cells, more than four sensor ranges long
    mp, scans, P, _ = corridor_session(8, spacing=20.0, step_deg=4.0, seed=1)
    shift = np.array([-70.0, -3.0, 0.0])
    mp = mp.copy()
    mp[:, :3] = (mp[:, :3].astype(np.float64) + shift).astype(np.float32)
    P = P.copy()
    P[:, [3, 7, 11]] += shift
    out["corridor"] = dict(map=mp, scans=scans, poses=P, labels=None, cfg={}, remove_res=(2.5, 2.0, 1.5), revert_res=(5.0,))
    # a keyframe farther than max_range from every point
    mp, scans, P, lab = constructed_scene(2, 1.0, 0)
    far = _pose12(_rz(1.0), np.array([500.0, -300.0, 2.0])).reshape(1, 12)
    out["far_keyframe"] = dict(map=mp, scans=scans + [scans[0]], poses=np.concatenate([P, far], 0), labels=lab, cfg={},
                               remove_res=(2.5, 2.0, 1.5), revert_res=())
    mp, scans, P, lab = range_edge_scene()
    out["range_edge"] = dict(map=mp, scans=scans, poses=P, labels=None, cfg=dict(diff_thres=1e-4), remove_res=(2.5,), revert_res=(),
                             inside=lab)
    return out
