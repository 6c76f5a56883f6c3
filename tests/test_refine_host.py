"""CPU: the NumPy twin of the pose refinement behind EPnP (spef_amd/spe/refine.py), alone."""
import os
import sys

import numpy as np
import pytest

from oracle import epnp_ref as E
from spef_amd.quaternion import angle_deg
from spef_amd.spe import refine as RF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from refine_inputs import axis_case, noisy, one_outlier, pose_errors  # noqa: E402

FIXTURES = ('keypoints.npz', 'keypoints_speedplus.npz')
KAT_DEG, KAT_M = 5e-4, 2e-4      # the noise-free bounds of tests/test_gpu_keypoints.py


def _cam(g):
    return dict(kp3d=g['kp3d'], K=g['K'], nu=float(g['nu']), nv=float(g['nv']),
                dist=g['dist'] if 'dist' in g.files else None)


@pytest.fixture(scope='module')
def outlier_case(golden):
    """Per fixture: the one-outlier keypoints, the moved keypoint's index and the oracle EPnP start (float32)."""
    cache = {}

    def get(name):
        if name not in cache:
            g = golden(name)
            c = _cam(g)
            kp, which = one_outlier(g)
            q0, t0 = E.decode_batch(kp, c['kp3d'], c['K'], c['nu'], c['nv'], c['dist'])
            cache[name] = (g, c, kp, which, q0.astype(np.float32), t0.astype(np.float32))
        return cache[name]
    return get


def test_jacobian_matches_central_differences(golden):
    g = golden('keypoints.npz')
    X = g['kp3d'].astype(np.float64)
    idx = np.arange(8) * 200
    R = RF.quat2dcm(g['q'][idx].astype(np.float64))
    t = g['t'][idx].astype(np.float64)
    uv = RF.observations(g['kp2d'][idx], g['K'], float(g['nu']), float(g['nv'])) + 3.0   # a nonzero residual
    _, J, _ = RF.residual_jacobian(R, t, X, uv, g['K'])
    h = 1e-6
    for k in range(6):
        d = np.zeros((8, 6))
        d[:, k] = h
        rp, _, _ = RF.residual_jacobian(RF.so3_exp(d[:, :3]) @ R, t + d[:, 3:], X, uv, g['K'])
        rm, _, _ = RF.residual_jacobian(RF.so3_exp(-d[:, :3]) @ R, t - d[:, 3:], X, uv, g['K'])
        fd = (rp - rm) / (2 * h)
        scale = np.abs(J).max(axis=(1, 2, 3))[:, None, None]
        assert np.all(np.abs(J[..., k] - fd) <= 1e-6 * scale), k


@pytest.mark.parametrize('name', FIXTURES)
def test_noise_free_kat(golden, name):
    """From the fixture's own poses (all 1,800) and from the oracle EPnP (the first 64), with and without Huber: the
    refined pose stays within the EPnP known-answer bounds, and every problem converges."""
    g = golden(name)
    c = _cam(g)
    eq, et = E.decode_batch(g['kp2d'][:64], c['kp3d'], c['K'], c['nu'], c['nv'], c['dist'])
    for kp, q0, t0, huber in ((g['kp2d'], g['q'], g['t'], 4.0), (g['kp2d'], g['q'], g['t'], 0.0),
                              (g['kp2d'][:64], eq, et, 4.0)):
        o = RF.refine_pose_host(kp, q0, t0, max_iters=50, huber_px=huber, **c)
        assert not o['status'].any()
        assert np.all(o['fit'][:, 3] <= o['fit'][:, 2])
        assert angle_deg(o['ori'], g['q'][:len(kp)]).max() < KAT_DEG
        assert np.linalg.norm(o['pos'] - g['t'][:len(kp)], axis=1).max() < KAT_M


@pytest.mark.parametrize('name', FIXTURES)
def test_outlier_recovery_cost_and_convergence(outlier_case, name):
    g, c, kp, which, q0, t0 = outlier_case(name)
    a0, r0 = pose_errors(q0, t0, g)
    o = RF.refine_pose_host(kp, q0, t0, max_iters=50, huber_px=4.0, **c)
    a1, r1 = pose_errors(o['ori'], o['pos'], g)
    print(f'{name}: orientation median {np.median(a0):.3f} -> {np.median(a1):.3f} deg, relative position '
          f'{np.median(r0):.2e} -> {np.median(r1):.2e}, trials median {np.median(o["iters"]):.0f} max {o["iters"].max()}')
    assert np.median(a1) <= np.median(a0) / 3
    assert np.median(r1) <= np.median(r0) / 3
    assert np.all(o['fit'][:, 3] <= o['fit'][:, 2])            # monotone cost, no tolerance
    assert not o['status'].any()                               # every problem converged: no bit 32
    assert o['ori'].dtype == np.float32 and o['pos'].dtype == np.float32 and o['cov'].shape == (256, 6, 6)
    assert np.all(np.sum(o['ori'] * q0, axis=1) >= 0)          # the start's hemisphere
    cov = o['cov'].astype(np.float64)
    assert np.all(np.diagonal(cov, axis1=1, axis2=2) > 0) and np.allclose(cov, cov.transpose(0, 2, 1), rtol=1e-6)


@pytest.mark.parametrize('name', FIXTURES)
def test_zero_weight_on_the_outlier_recovers_like_huber(outlier_case, name):
    g, c, kp, which, q0, t0 = outlier_case(name)
    w = np.ones((256, 11), np.float32)
    w[np.arange(256), which] = 0
    a0, r0 = pose_errors(q0, t0, g)
    o = RF.refine_pose_host(kp, q0, t0, weights=w, max_iters=50, huber_px=0.0, **c)
    a1, r1 = pose_errors(o['ori'], o['pos'], g)
    assert not o['status'].any()
    assert np.median(a1) <= np.median(a0) / 3 and np.median(r1) <= np.median(r0) / 3


def test_plain_noise_cost_is_monotone(golden):
    g = golden('keypoints.npz')
    c = _cam(g)
    kp = noisy(g, 3, 3.0, 64)
    q0, t0 = E.decode_batch(kp, c['kp3d'], c['K'])
    for huber in (0.0, 4.0):
        o = RF.refine_pose_host(kp, q0, t0, max_iters=50, huber_px=huber, **c)
        assert np.all(o['fit'][:, 3] <= o['fit'][:, 2]) and not (o['status'] & RF.NOT_REFINED).any()
        if huber == 0:   # plain least squares: the squared RMS is the cost, and Gauss-Newton converges quickly
            assert np.all(o['fit'][:, 1] <= o['fit'][:, 0]) and not o['status'].any()
        # (Huber at 4 px on 3 px noise puts many points at the kink: IRLS converges linearly there and a row may
        # need more than 50 trials to reach the 1e-10 step -- bit 32, with the best pose so far)


def test_zero_accept_returns_the_input_bit_for_bit():
    """A problem in which every trial is rejected (axis_case: the normal matrix has a zero pivot whatever the damping)
    ends when the damping passes 1e12, with quaternion and position carrying the input's bits."""
    kp3d, K, kp, w, q0, t0 = axis_case()
    o = RF.refine_pose_host(kp, q0, t0, kp3d, K, 1920.0, 1200.0, weights=w, max_iters=50, huber_px=0.0)
    assert np.array_equal(o['ori'].view(np.uint32), q0.view(np.uint32))
    assert np.array_equal(o['pos'].view(np.uint32), t0.view(np.uint32))
    assert np.all(o['status'] == 0) and np.all((o['iters'] == 15) | (o['iters'] == 16))   # 1e-3 x 10^k > 1e12
    assert np.all(o['fit'][:, 3] == o['fit'][:, 2]) and np.all(o['fit'][:, 2] > 0)
    assert np.all(np.isnan(o['cov']))                          # singular normal matrix
    cut = RF.refine_pose_host(kp, q0, t0, kp3d, K, 1920.0, 1200.0, weights=w, max_iters=5, huber_px=0.0)
    assert np.all(cut['status'] == RF.MAX_ITERS) and np.all(cut['iters'] == 5)
    assert np.array_equal(cut['ori'].view(np.uint32), q0.view(np.uint32))


def test_status_bits(golden):
    g = golden('keypoints.npz')
    c = _cam(g)
    kp = noisy(g, 5, 3.0, 8)
    q0, t0 = g['q'][:8].astype(np.float32), g['t'][:8].astype(np.float32)
    kp[1, 6] = np.nan                       # a non-finite keypoint
    t0[2, 2] = -t0[2, 2]                    # the model behind the camera
    st = np.zeros(8, np.int32)
    st[3] = 8                               # EPnP failed on this row
    w = np.ones((8, 11), np.float32)
    w[4, 2:] = 0                            # two points left
    w[5, 0] = np.inf
    q0[6] = 0                               # no orientation
    o = RF.refine_pose_host(kp, q0, t0, weights=w, max_iters=50, huber_px=4.0, status=st, **c)
    assert list(o['status']) == [0, 16, 16, 24, 16, 16, 16, 0]
    for r in range(1, 7):
        assert np.array_equal(o['ori'][r].view(np.uint32), q0[r].view(np.uint32))
        assert np.array_equal(o['pos'][r].view(np.uint32), t0[r].view(np.uint32))
        assert np.all(np.isnan(o['fit'][r])) and np.all(np.isnan(o['cov'][r])) and o['iters'][r] == 0
    for r in (0, 7):                        # the neighbours are refined as usual
        assert o['fit'][r, 3] < o['fit'][r, 2] and o['iters'][r] > 1 and np.all(np.isfinite(o['cov'][r]))
    assert list(st) == [0, 0, 0, 8, 0, 0, 0, 0]      # the caller's array is not written
    one = RF.refine_pose_host(kp[:1], q0[:1], t0[:1], max_iters=1, huber_px=4.0, **c)
    assert one['status'][0] == 32 and one['iters'][0] == 1
    with pytest.raises(AssertionError):
        RF.refine_pose_host(kp, q0, t0, max_iters=0, **c)
    with pytest.raises(AssertionError):
        RF.refine_pose_host(kp, q0, t0, max_iters=101, **c)
    with pytest.raises(AssertionError):
        RF.refine_pose_host(kp, q0, t0, huber_px=-1.0, **c)


def test_twin_is_vectorised():
    """256 problems x 50 trials in well under a second (the issue's budget), on 16 keypoints."""
    import time
    rng = np.random.default_rng(2)
    X = rng.uniform(-0.5, 0.5, (16, 3)).astype(np.float32)
    K = np.array([[3000.0, 0, 960], [0, 3000.0, 600], [0, 0, 1]])
    kp = rng.uniform(0.2, 0.8, (256, 34)).astype(np.float32)   # no pose fits these: every problem runs all its trials
    q0 = np.tile(np.float32([1, 0, 0, 0]), (256, 1))
    t0 = np.tile(np.float32([0, 0, 8]), (256, 1))
    t = time.perf_counter()
    o = RF.refine_pose_host(kp, q0, t0, X, K, 1920.0, 1200.0, max_iters=50, huber_px=4.0)
    dt = time.perf_counter() - t
    assert o['iters'].max() >= 20 and np.all(o['fit'][:, 3] <= o['fit'][:, 2])
    assert dt < 1.0, dt


def test_config_keys(tmp_path):
    from spef_amd.config import keypoint_refine, load_config
    cfg = load_config(None)
    assert cfg.MODEL.HEAD.KEYPOINTS_REFINE_ITERS == 0 and cfg.MODEL.HEAD.KEYPOINTS_REFINE_HUBER_PX == 0.0
    assert keypoint_refine(cfg) is None
    p = tmp_path / 'c.yaml'
    p.write_text('MODEL:\n  HEAD:\n    ORI: keypoints\n    POS: keypoints\n    KEYPOINTS_REFINE_ITERS: 50\n'
                 '    KEYPOINTS_REFINE_HUBER_PX: 4\n')
    assert keypoint_refine(load_config(str(p))) == (50, 4.0)
    p.write_text('MODEL:\n  HEAD:\n    KEYPOINTS_REFINE_LAMBDA: 1.0\n')
    with pytest.raises(KeyError):
        load_config(str(p))


def test_does_not_import_the_oracle():
    src = open(RF.__file__).read()
    assert 'oracle' not in src
