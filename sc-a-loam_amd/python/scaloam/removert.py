"""CPU restatement of scal_removert_* (include/scaloam_hip.h): dynamic-point removal from a merged keyframe map by range-image
visibility.  This file is the specification csrc/removert.hip is held to bit for bit, in the role pgo.py has for the pose graph;
Removert itself (Kim and Kim, IROS 2020) is not part of the reference tree and is restated here, not reproduced - DESIGN.md
section 8.10 lists where the two differ.  numpy only, every expression elementwise in the order the header states (no `@`, no BLAS),
so that each f64 operation rounds exactly once, as the kernels' do without fp contraction.  No GPU work here."""
import math
from collections import namedtuple

import numpy as np

DEFAULT_REMOVE_RES = (2.5, 2.0, 1.5)
DEFAULT_REVERT_RES = (5.0,)

RemovertResult = namedtuple("RemovertResult", "mask hits stats margin images hits_all")


def _lround(x):
    """C's lround for x >= 0: halves away from zero (Python's round() sends them to the even neighbour)"""
    f = math.floor(x)
    return int(f) + (1 if x - f >= 0.5 else 0)


def image_shape(res, fov_up_deg=25.0, fov_down_deg=-25.0):
    """(H, W) of the range image at `res` degrees per pixel"""
    return max(1, _lround((float(fov_up_deg) - float(fov_down_deg)) / float(res))), _lround(360.0 / float(res))


def finest(remove_res):
    """index of the finest remove resolution (the first of the smallest): the one the hits output reports"""
    return int(np.argmin(np.asarray(remove_res, np.float64))) if len(remove_res) else -1


class View:
    """Points as seen from one pose: f32 range, the range test, azimuth and elevation - everything that does not depend on the
    resolution.  pose12 None = the identity (a scan in its own frame); it goes through the same arithmetic."""

    def __init__(self, xyz, pose12, min_range, max_range):
        P = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64) if pose12 is None else np.asarray(pose12, np.float64).reshape(12)
        p = np.asarray(xyz)[:, :3].astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            d0, d1, d2 = p[:, 0] - P[3], p[:, 1] - P[7], p[:, 2] - P[11]
            x = (P[0] * d0 + P[4] * d1) + P[8] * d2
            y = (P[1] * d0 + P[5] * d1) + P[9] * d2
            z = (P[2] * d0 + P[6] * d1) + P[10] * d2
            xy = x * x + y * y
            self.r = np.sqrt(xy + z * z).astype(np.float32)
            self.in_range = (self.r >= np.float32(min_range)) & (self.r <= np.float32(max_range))
            self.az = np.arctan2(y, x)
            self.el = np.arctan2(z, np.sqrt(xy))

    def pixels(self, res, fov_up_deg, fov_down_deg):
        """(takes part, row, col, margin) at `res`.  margin: the smallest distance, in pixels, of u or v of a participating point
        to an integer - and of v of a point inside the range gate but outside the field of view to the field's edge, where a
        last-bit difference in atan2 would let it in."""
        H, W = image_shape(res, fov_up_deg, fov_down_deg)
        fu, fd = float(fov_up_deg) * (np.pi / 180.0), float(fov_down_deg) * (np.pi / 180.0)
        with np.errstate(invalid="ignore"):
            u = (self.az + np.pi) / (2.0 * np.pi) * W
            v = (fu - self.el) / (fu - fd) * H
            ok = self.in_range & (v >= 0.0) & (v < H)
        row = np.where(ok, v, 0.0).astype(np.int64)
        col = np.minimum(np.where(ok, u, 0.0).astype(np.int64), W - 1)
        margin = np.inf
        if ok.any():
            uo, vo = u[ok], v[ok]
            margin = min(margin, float(np.abs(uo - np.rint(uo)).min()), float(np.abs(vo - np.rint(vo)).min()))
        out = self.in_range & ~ok
        if out.any():
            vo = v[out]
            margin = min(margin, float(np.minimum(np.abs(vo), np.abs(vo - H)).min()))
        return ok, row, col, margin


def scan_images(scan_xyzi, resolutions, fov_up_deg=25.0, fov_down_deg=-25.0, min_range=0.5, max_range=80.0):
    """one [H, W] f32 range image per resolution: the smallest range in each pixel, +inf where no point falls; and the margin"""
    view = View(np.asarray(scan_xyzi, np.float32).reshape(-1, 4), None, min_range, max_range)
    images, margin = [], np.inf
    for res in resolutions:
        H, W = image_shape(res, fov_up_deg, fov_down_deg)
        ok, row, col, m = view.pixels(res, fov_up_deg, fov_down_deg)
        img = np.full(H * W, np.inf, np.float32)
        np.minimum.at(img, (row * W + col)[ok], view.r[ok])
        images.append(img.reshape(H, W))
        margin = min(margin, m)
    return images, margin


def remove_dynamic_points(map_xyzi, scans, poses12, remove_res=DEFAULT_REMOVE_RES, revert_res=DEFAULT_REVERT_RES, fov_up_deg=25.0,
                          fov_down_deg=-25.0, min_range=0.5, max_range=80.0, diff_thres=0.1, min_hits=1, keep_images=True):
    """map_xyzi [n, 4] f32 in the world frame; scans: K arrays [*, 4] f32 in their sensor frames; poses12 [K, 12] f64, sensor to
    world.  Returns RemovertResult: mask uint8 [n]; hits uint16 [n] at the finest remove resolution (saturating); stats (every pair
    is tested here: pairs_tested = n K); margin (see View.pixels); images[k][i] for resolution i of remove_res + revert_res;
    hits_all uint16 [R, n]."""
    mp = np.ascontiguousarray(map_xyzi, np.float32).reshape(-1, 4)
    P = np.asarray(poses12, np.float64).reshape(-1, 12)
    if P.shape[0] != len(scans):
        raise ValueError("one pose12 row per scan is needed")
    resolutions = [float(r) for r in remove_res] + [float(r) for r in revert_res]
    n_remove, n, K, R = len(remove_res), mp.shape[0], len(scans), len(remove_res) + len(revert_res)
    hits = np.zeros((R, n), np.int64)
    margin, images = np.inf, []
    thres = np.float32(diff_thres)
    for k in range(K):
        imgs, m = scan_images(scans[k], resolutions, fov_up_deg, fov_down_deg, min_range, max_range)
        margin = min(margin, m)
        view = View(mp, P[k], min_range, max_range)
        for i, res in enumerate(resolutions):
            ok, row, col, m = view.pixels(res, fov_up_deg, fov_down_deg)
            margin = min(margin, m)
            scan_r = imgs[i][row, col]
            with np.errstate(invalid="ignore"):
                hit = ok & np.isfinite(scan_r) & ((np.where(np.isfinite(scan_r), scan_r, np.float32(0)) - view.r) > thres)
            hits[i] += hit
        if keep_images:
            images.append(imgs)
    removed = np.zeros(n, bool)
    for i in range(n_remove):
        removed |= hits[i] >= int(min_hits)
    for i in range(n_remove, R):
        removed &= hits[i] >= 1
    mask = removed.astype(np.uint8)
    hits_all = np.minimum(hits, 65535).astype(np.uint16)
    f = finest(remove_res)
    stats = dict(points=n, keyframes=K, dynamic=int(mask.sum()), pairs_tested=n * K, pairs_bruteforce=n * K)
    return RemovertResult(mask, hits_all[f].copy() if f >= 0 else np.zeros(n, np.uint16), stats, margin, images, hits_all)
