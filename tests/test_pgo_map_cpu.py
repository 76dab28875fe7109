"""scaloam.pgo.pgo_map_cloud: the pose-graph map's cloud before its VoxelGrid (pubMap, laserPosegraphOptimization.cpp:810-834) - which
keyframes it takes (every skip-th below kf_end, counted from the pipeline's first own keyframe) and local2global's f32 arithmetic."""
import numpy as np

from scaloam.pgo import _affine_f32, local2global_f32, pgo_map_cloud


def _clouds(n_kf, seed=7):
    rng = np.random.default_rng(seed)
    out = []
    for j in range(n_kf):
        c = rng.uniform(-40.0, 40.0, size=(3 + j % 4, 4)).astype(np.float32)
        c[:, 3] = 100 * j + np.arange(c.shape[0])  # intensity tags the keyframe and the point
        out.append(c)
    return out


def _poses(n_kf, seed=8):
    rng = np.random.default_rng(seed)
    return [np.concatenate([rng.uniform(-50, 50, 3), rng.uniform(-0.3, 0.3, 2), rng.uniform(-np.pi, np.pi, 1)]) for _ in range(n_kf)]


def test_selection_skip_and_kf_end():
    clouds, poses = _clouds(9), _poses(9)
    for n_own in (0, 1, 4, 9):
        for skip in (1, 2, 3):
            got = pgo_map_cloud(clouds, poses, n_own, skip)
            picked = list(range(0, n_own, skip))
            assert got.dtype == np.float32 and got.shape == (sum(clouds[j].shape[0] for j in picked), 4)
            # concatenated in keyframe order: the intensities name the keyframes and their points in order
            want_w = np.concatenate([clouds[j][:, 3] for j in picked]) if picked else np.zeros(0, np.float32)
            assert np.array_equal(got[:, 3], want_w), (n_own, skip)


def test_prefilled_entries_shift_kf_end():
    """with n_pre pre-filled database entries the own keyframes are database indices n_pre, n_pre + 1, ...: kf_end = n_pre + k covers
    the first k own keyframes, kf_end <= n_pre none"""
    clouds, poses = _clouds(6), _poses(6)
    n_pre = 40
    for kf_end in (n_pre - 3, n_pre, n_pre + 1, n_pre + 5):
        got = pgo_map_cloud(clouds, poses, kf_end - n_pre, 2)
        want = list(range(0, max(0, kf_end - n_pre), 2))
        assert got.shape[0] == sum(clouds[j].shape[0] for j in want), kf_end


def test_f32_operation_order():
    """each coordinate is ((T0 x + T1 y) + T2 z) + T3 with every product and sum rounded to f32 (xf_point's order, no contraction)"""
    clouds, poses = _clouds(5), _poses(5)
    got = pgo_map_cloud(clouds, poses, 5, 1)
    rows, other = [], []
    for j in range(5):
        T = _affine_f32(*poses[j])
        for p in clouds[j]:
            x, y, z = np.float32(p[0]), np.float32(p[1]), np.float32(p[2])
            q = [np.float32(np.float32(np.float32(T[r, 0] * x) + np.float32(T[r, 1] * y)) + np.float32(T[r, 2] * z)) + T[r, 3] for r in range(3)]
            rows.append([q[0], q[1], q[2], p[3]])
            # the same sum in double, rounded once: what a contracted or reassociated evaluation comes closer to
            other.append([np.float32(float(T[r, 0]) * float(x) + float(T[r, 1]) * float(y) + float(T[r, 2]) * float(z) + float(T[r, 3]))
                          for r in range(3)])
    want = np.array(rows, np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(got[:, :3], np.array(other, np.float32)), "the inputs do not tell the operation order apart"
    assert np.array_equal(got, np.concatenate([local2global_f32(clouds[j], poses[j]) for j in range(5)]))


def test_empty_map():
    got = pgo_map_cloud([], [], 0, 2)
    assert got.shape == (0, 4) and got.dtype == np.float32
