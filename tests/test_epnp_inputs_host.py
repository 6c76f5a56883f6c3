"""The conditions that the inputs of tests/test_gpu_epnp_shapes.py must meet, checked by the oracle alone (no GPU):
the comparison there is only as good as its inputs."""
import os
import sys

import numpy as np
import pytest

from oracle import decode_ref as D
from oracle import epnp_ref as E

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epnp_inputs as I  # noqa: E402


def test_every_approximation_wins_on_the_noisy_sweep(golden):
    """Each of EPnP's three beta approximations has the lowest reprojection error in at least 5 % of the 512 noisy
    sweep rows, and the winner keyword leaves the pose as it was."""
    g = golden('keypoints.npz')
    win = I.noisy_sweep_winners(g)
    counts = np.bincount(win, minlength=4)[1:]
    print(f'winning approximation 1 / 2 / 3: {counts.tolist()}')
    assert win.size == 512 and counts.sum() == 512 and (counts >= 0.05 * win.size).all()
    c = I.case(g, 7, 'second', 1.0)
    q, t = E.decode_batch(c['kp'][:4], c['pts'], c['cam'].K, c['cam'].nu, c['cam'].nv)
    assert np.array_equal(q, c['rq'][:4]) and np.array_equal(t, c['rt'][:4])


def test_models_stay_in_frame_and_the_oracle_recovers_the_truth(golden):
    """Every case keeps at least 90 % of its rows inside the image; noise-free, the oracle is within a fifth of the
    known-answer bounds' angle (5e-4 deg) and 40 % of their position (2e-4 m) of the true pose, through float32
    pixels, for n = 5, 6, 16 and the cube on both cameras."""
    g = golden('keypoints.npz')
    for n in I.KAT_MODELS + I.SWEEP_N:
        for camera in I.CAMERAS:
            c = I.case(g, n, camera, 0.0)
            assert c['inside'] >= 0.9, (n, camera, c['inside'])
            ang = D.angle_deg_stable(c['rq'], c['q'])
            dp = np.linalg.norm(c['rt'] - c['t'], axis=1)
            print(f'model {n}, {camera}: inside {c["inside"]:.2f}, oracle to truth {ang.max():.2e} deg {dp.max():.2e} m')
            assert ang.max() < 1.1e-4 and dp.max() < 8e-5
    cam = I.second_camera()
    assert cam.K[0, 0] != cam.K[1, 1] and (cam.nu, cam.nv) != (1920.0, 1200.0)
    assert abs(cam.K[0, 2] - cam.nu / 2) > 50 and abs(cam.K[1, 2] - cam.nv / 2) > 50


@pytest.mark.parametrize('kind', I.DIST_KINDS)
def test_distortion_cases_take_the_fallback_where_meant(golden, kind):
    """The strong-k1 cases send some points, not most, through undistortPoints' icdist < 0 fallback; the mild one
    none. The 4-coefficient form is the 5-coefficient one with k3 = 0."""
    gp = golden('keypoints_speedplus.npz')
    c = I.distortion_case(gp, kind)
    fell = c['fell']
    print(f'{kind}: fallback points {int(fell.sum())} of {fell.size}, in {int(fell.any(1).sum())} rows')
    assert np.isfinite(c['rq']).all() and np.isfinite(c['rt']).all()
    if kind == '4coef_mild':
        assert not fell.any()
    else:
        assert fell.sum() >= 1 and fell.mean() < 0.5
    if c['dist'].size == 4:
        us32 = E.pixels_f32(c['kp'][0], c['cam'].nu, c['cam'].nv)
        assert np.array_equal(E.undistort_points(us32, c['cam'].K, c['dist']),
                              E.undistort_points(us32, c['cam'].K, np.append(c['dist'], 0.0)))
