"""Inputs shared by tests/test_consensus_host.py and tests/test_gpu_consensus.py (not a test module)."""
import numpy as np

FIXTURES = {'keypoints.npz': 96, 'keypoints_speedplus.npz': 64}     # fixture -> rows of the planted inputs
TAU, MIN_INLIERS = 8.0, 6


def cam(g):
    return dict(kp3d=g['kp3d'], K=g['K'], nu=float(g['nu']), nv=float(g['nv']),
                dist=g['dist'] if 'dist' in g.files else None)


def planted(g, k, count, seed=None):
    """default_rng(11 + k): the first ``count`` fixture poses with 1 px Gaussian noise on every keypoint and ``k``
    keypoints per frame (never the origin) moved 40 to 200 px in a random direction
    -> (keypoints float32 [count x 2(n+1)], moved [count x n] bool)."""
    rng = np.random.default_rng(11 + k if seed is None else seed)
    nu, nv = float(g['nu']), float(g['nv'])
    n = g['kp2d'].shape[1] // 2 - 1
    px = g['kp2d'][:count].astype(np.float64).reshape(count, n + 1, 2) * [nu, nv]
    px += rng.normal(0, 1.0, px.shape)
    bad = np.zeros((count, n), bool)
    for i in range(count):
        w = rng.choice(n, k, replace=False)
        bad[i, w] = True
        phi = rng.uniform(0, 2 * np.pi, k)
        r = rng.uniform(40, 200, k)
        px[i, w + 1] += np.stack([r * np.cos(phi), r * np.sin(phi)], -1)
    return (px / [nu, nv]).reshape(count, -1).astype(np.float32), bad
