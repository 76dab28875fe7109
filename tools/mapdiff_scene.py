"""A constructed pair of sessions with known differences, for the map diff tests (scaloam.nbr.map_diff) and tools/bench_mapdiff.py;
ray casts on a jittered grid as in tools/removert_scene.py.

Static, in both sessions: a belt of a sphere of radius 30 m about the origin (|z| <= 10 m, so every keyframe's +-25 degree field of
view holds all of it), open towards +x (no wall where the azimuth of the wall point is within +-35 degrees), and in that opening a
panel: a disc of radius 1.5 m at (10, 0, 0) facing the origin.  Rays that leave through the opening return nothing.
Session Y drives near the origin: keyframes at (0, -+0.5, 0).  Session X's keyframes stand 4 m to either side, (0, +-4, 0).
  A  a ball only X has, at (-10, 0, 0): Y looks straight through its place to the wall behind          -> X to Y: CHANGED
  B  a ball only X has, at (25, 0, 0), behind the panel as seen from Y (the panel covers +-8.5 degrees there, the ball +-1.6);
     X's keyframes see it past the panel's edge, and nothing static lies behind it                         -> X to Y: UNOBSERVED
  C  a ball only Y has, at 8 m and 135 degrees: X looks through its place                                -> Y to X: CHANGED
Everything else is COMMON in both directions, by construction: the keyframes of a session stand farther apart than any ball is wide,
so a ball's shadow from one keyframe ends (8 to 12 m behind it) before the wall and the other keyframe samples that wall; the
panel's shadows from all four keyframes fall into the opening; 1 degree rays leave the wall's samples under 0.65 m apart, below the
0.8 m radius of the diff.  update_map of the two diffs therefore holds the wall and the panel once, B and C, and not A."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from removert_scene import _hit_sphere, _pose12, _rays, _rz, _to_world  # noqa: E402

WALL_RADIUS, WALL_HALF_HEIGHT, OPENING_DEG = 30.0, 10.0, 35.0
PANEL_X, PANEL_RADIUS = 10.0, 1.5
BALL_A = (np.array([-10.0, 0.0, 0.0]), 0.5)
BALL_B = (np.array([25.0, 0.0, 0.0]), 0.7)
BALL_C = (8.0 * np.array([np.cos(np.radians(135.0)), np.sin(np.radians(135.0)), 0.0]), 0.3)
STATIC, OBJ_A, OBJ_B, OBJ_C = 0, 1, 2, 3


def _cast(R, t, dirs, balls):
    """one scan: (sensor-frame xyzi f32, what each return is: STATIC or the ball's tag).  balls: (tag, centre, radius)"""
    dw = dirs @ R.T
    s = _hit_sphere(t, dw, np.zeros(3), WALL_RADIUS, True)
    p = t + dw * np.where(np.isfinite(s), s, 0.0)[:, None]
    s = np.where((np.abs(p[:, 2]) <= WALL_HALF_HEIGHT) & (np.abs(np.degrees(np.arctan2(p[:, 1], p[:, 0]))) > OPENING_DEG), s, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        sp = (PANEL_X - t[0]) / dw[:, 0]
    pp = t + dw * np.where(np.isfinite(sp), sp, 0.0)[:, None]
    s = np.minimum(s, np.where(np.isfinite(sp) & (sp > 0) & (pp[:, 1] ** 2 + pp[:, 2] ** 2 <= PANEL_RADIUS ** 2), sp, np.inf))
    what = np.full(dirs.shape[0], STATIC)
    for tag, c, rad in balls:
        sb = _hit_sphere(t, dw, c, rad, False)
        what = np.where(sb < s, tag, what)
        s = np.minimum(s, sb)
    keep = np.isfinite(s)
    pts = (dirs * s[:, None])[keep]
    return np.concatenate([pts, np.zeros((pts.shape[0], 1))], 1).astype(np.float32), what[keep]


def _session(places, balls, step_deg, rng, yaw0):
    scans, poses, maps, what = [], [], [], []
    for k, place in enumerate(places):
        t = np.asarray(place, float) + np.concatenate([rng.uniform(-0.05, 0.05, 2), rng.uniform(-0.02, 0.02, 1)])
        R = _rz(yaw0 + 0.3 * k)
        scan, w = _cast(R, t, _rays(step_deg, rng), balls)
        scans.append(scan), poses.append(_pose12(R, t)), maps.append(_to_world(scan, R, t)), what.append(w)
    return dict(map=np.concatenate(maps, 0), scans=scans, poses=np.array(poses), what=np.concatenate(what))


def two_sessions(step_deg=1.0, seed=0):
    """(X, Y): dicts of map [n, 4] f32, scans, poses [2, 12], what [n] (STATIC / OBJ_*), and `labels`: the diff towards the other
    session that the construction implies"""
    rng = np.random.default_rng(seed)
    X = _session([(0.0, 4.0, 0.0), (0.0, -4.0, 0.0)], [(OBJ_A,) + BALL_A, (OBJ_B,) + BALL_B], step_deg, rng, 0.1)
    Y = _session([(0.0, -0.5, 0.0), (0.0, 0.5, 0.0)], [(OBJ_C,) + BALL_C], step_deg, rng, 0.7)
    X["labels"] = np.select([X["what"] == OBJ_A, X["what"] == OBJ_B], [2, 1], 0).astype(np.uint8)
    Y["labels"] = np.where(Y["what"] == OBJ_C, 2, 0).astype(np.uint8)
    return X, Y


SCENE_SEED = 0   # tests/test_nbr_cpu.py holds this seed to Removert's margin condition


def golden_pair(golden_dir):
    """(map X, map Y, Y's scans, Y's poses): the committed KAIST03 keyframes 0 and 7 merged against keyframe 20, golden poses"""
    scans = {k: np.load(os.path.join(golden_dir, f"KAIST03_{k:06d}.npy")).astype(np.float32) for k in (0, 7, 20)}
    P = np.load(os.path.join(golden_dir, "KAIST03_poses21.npy")).reshape(-1, 12).astype(np.float64)
    world = {k: _to_world(scans[k], P[k].reshape(3, 4)[:, :3], P[k].reshape(3, 4)[:, 3]) for k in scans}
    return np.concatenate([world[0], world[7]], 0), world[20], [scans[20]], P[[20]]


def radius_inputs(r, n_index=3000, n_query=2000, seed=0):
    """(index [*, 4], queries [*, 4]) f32 for the radius query at radius r: uniform in a 6 m cube about the origin, and seeded into it
    records on cell boundaries (multiples of the cell width - the smallest power of two above r - and of r), pairs at exactly r,
    exact duplicates, records that are not finite on both sides, a clump of 200 records in one cell (all within r of its centre, which is a query) with queries around it, and
    records near +-60 km in x and y and +-7 km in z (beyond the clamp of the cell key at every r up to 1 m) with neighbours."""
    rng = np.random.default_rng(seed)
    r32 = np.float32(r)
    w = np.float32(2.0) ** np.float32(np.floor(np.log2(float(r32))) + 1)
    I = [rng.uniform(-3, 3, (n_index, 3))]
    Q = [rng.uniform(-3, 3, (n_query, 3))]
    g = np.array([-2.0, -1.0, 0.0, 1.0, 2.0])
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    for width in (float(w), float(r32)):
        I.append(lattice * width), Q.append(lattice[::2] * width), Q.append(lattice * width + rng.uniform(-0.3, 0.3, lattice.shape) * width)
    # pairs at exactly r along every axis, both ways round, at the origin and off a cell corner
    for base in (np.zeros(3), np.array([float(w), -float(w), 2 * float(w)])):
        I.append(base[None]), Q.append(base[None])
        for axis in range(3):
            for sign in (-1.0, 1.0):
                e = np.zeros(3)
                e[axis] = sign * float(r32)
                Q.append((base + e)[None]), I.append((base - e)[None])
    I.append(I[0][:40]), Q.append(I[0][40:80]), Q.append(Q[0][:20])          # duplicates within and across the sets
    centre = np.array([0.5, 1.5, -0.5]) * float(w)
    I.append(centre + rng.uniform(-0.1, 0.1, (200, 3)) * float(w)), Q.append(centre + rng.uniform(-1.2, 1.2, (80, 3)) * float(w)), Q.append(centre[None])
    for far in ((60000.0, 10.0, 1.0), (-60000.0, -59000.0, 2.0), (5.0, 61000.0, -7000.0), (-3.0, 2.0, 7000.0), (60000.0, 60000.0, 7000.0)):
        f = np.array(far)
        I.append(f + rng.uniform(-1.0, 1.0, (30, 3)) * float(r32)), Q.append(f + rng.uniform(-1.0, 1.0, (12, 3)) * float(r32))
        Q.append(I[-1][:3])
    I, Q = np.concatenate(I, 0), np.concatenate(Q, 0)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan], [np.inf, -np.inf, 1.0]])
    I, Q = np.concatenate([I[:500], bad, I[500:], bad[:2]], 0), np.concatenate([bad[1:], Q[:900], bad, Q[900:]], 0)
    pi, pq = rng.permutation(I.shape[0]), rng.permutation(Q.shape[0])
    with np.errstate(invalid="ignore"):
        I4 = np.concatenate([I, rng.uniform(0, 255, (I.shape[0], 1))], 1).astype(np.float32)[pi]
        Q4 = np.concatenate([Q, rng.uniform(0, 255, (Q.shape[0], 1))], 1).astype(np.float32)[pq]
    return I4, Q4


RADII = (0.5, 0.3, 0.7, 1.0, 1e-3)
