"""Inputs shared by tests/test_refine_host.py and tests/test_gpu_refine.py (not a test module)."""
import numpy as np

from spef_amd.quaternion import angle_deg


def noisy(g, seed, sigma_px, count=256):
    """The first ``count`` fixture poses with Gaussian keypoint noise of ``sigma_px`` pixels."""
    rng = np.random.default_rng(seed)
    scale = np.tile([1 / float(g['nu']), 1 / float(g['nv'])], g['kp2d'].shape[1] // 2)
    return (g['kp2d'][:count] + rng.normal(0, sigma_px, (count, g['kp2d'].shape[1])) * scale).astype(np.float32)


def one_outlier(g, count=256):
    """default_rng(7): 1 px Gaussian noise on every keypoint, and one keypoint per frame (never the origin) moved
    60 px in a random direction -> (keypoints float32 [count x 2(n+1)], index of the moved keypoint [count])."""
    rng = np.random.default_rng(7)
    nu, nv = float(g['nu']), float(g['nv'])
    n = g['kp2d'].shape[1] // 2 - 1
    px = g['kp2d'][:count].astype(np.float64).reshape(count, n + 1, 2) * [nu, nv]
    px += rng.normal(0, 1.0, px.shape)
    which = rng.integers(0, n, count)
    phi = rng.uniform(0, 2 * np.pi, count)
    px[np.arange(count), which + 1] += 60.0 * np.stack([np.cos(phi), np.sin(phi)], -1)
    return (px / [nu, nv]).reshape(count, -1).astype(np.float32), which


def pose_errors(q, t, g, count=None):
    """-> (orientation error in degrees, position error relative to the range) against the fixture's poses."""
    count = q.shape[0] if count is None else count
    gt = g['t'][:count].astype(np.float64)
    return (angle_deg(q, g['q'][:count]),
            np.linalg.norm(np.asarray(t, np.float64) - gt, axis=1) / np.linalg.norm(gt, axis=1))


def axis_case(count=3):
    """Problems in which no trial can be accepted: the three points with a positive weight lie on the camera's optical
    axis (identity rotation, points on the model's z axis), so the rotation about that axis moves nothing, its diagonal
    entry of the normal matrix is exactly zero, and the Cholesky pivot fails under any damping. The three points off
    the axis keep the model non-degenerate and carry weight zero.
    -> (kp3d [6 x 3], K, keypoints [count x 14], weights [count x 6], quaternions, positions)."""
    kp3d = np.float32([[0, 0, -0.25], [0, 0, 0.125], [0, 0, 0.5], [0.5, 0, 0], [0, 0.5, 0], [0.25, 0.25, 0.25]])
    K = np.array([[3000.0, 0, 960], [0, 3000.0, 600], [0, 0, 1]])
    rng = np.random.default_rng(5)
    kp = rng.uniform(0.3, 0.7, (count, 14)).astype(np.float32)
    w = np.tile(np.float32([1, 1, 1, 0, 0, 0]), (count, 1))
    q0 = np.tile(np.float32([1, 0, 0, 0]), (count, 1))
    t0 = np.tile(np.float32([0.25, -0.125, 8]), (count, 1))
    return kp3d, K, kp, w, q0, t0
