"""CPU: the NumPy twin of the 3-point consensus between EPnP and the refinement (spef_amd/spe/consensus.py), alone."""
import os
import sys
import time

import numpy as np
import pytest

from oracle import epnp_ref as E
from spef_amd.quaternion import angle_deg
from spef_amd.spe import consensus as CS
from spef_amd.spe import refine as RF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from consensus_inputs import FIXTURES, MIN_INLIERS, TAU, cam, planted  # noqa: E402

KAT_DEG, KAT_M = 5e-4, 2e-4      # the noise-free bounds of tests/test_refine_host.py
ANG_MED, ANG_MAX, POS_MED, POS_MAX = 1e-4, 0.1, 1e-5, 1e-3      # the bounds of tests/test_gpu_refine.py
KS = (1, 2, 3, 4, 5)


@pytest.fixture(scope='module')
def planted_case(golden):
    """(fixture, k) -> the planted inputs, the moved points, the oracle EPnP start and the twin's result; computed
    once."""
    cache = {}

    def get(name, k):
        if (name, k) not in cache:
            g = golden(name)
            c = cam(g)
            kp, bad = planted(g, k, FIXTURES[name])
            q0, t0 = E.decode_batch(kp, c['kp3d'], c['K'], c['nu'], c['nv'], c['dist'])
            q0, t0 = q0.astype(np.float32), t0.astype(np.float32)
            cache[(name, k)] = (g, c, kp, bad, q0, t0,
                                CS.consensus_host(kp, inlier_px=TAU, min_inliers=MIN_INLIERS, quat=q0, pos=t0, **c))
        return cache[(name, k)]
    return get


def test_triples_are_lexicographic():
    for n in (4, 11, 16):
        tr = CS.triples(n)
        assert tr.shape == (n * (n - 1) * (n - 2) // 6, 3)
        assert np.all(tr[:, 0] < tr[:, 1]) and np.all(tr[:, 1] < tr[:, 2]) and tr.max() == n - 1
        key = (tr[:, 0] * n + tr[:, 1]) * n + tr[:, 2]
        assert np.all(np.diff(key) > 0)
    assert CS.default_min_inliers(11) == 6 and CS.default_min_inliers(4) == 4 and CS.default_min_inliers(16) == 8


def test_quartic_roots_known_answers():
    """Products of known linear factors: four, two and no real roots, ascending, +inf for the missing ones."""
    def coef(roots):
        return np.poly(roots)[:, None]
    r4 = CS.quartic_roots(*coef([0.5, -2.0, 3.0, 1.25]))[0]
    np.testing.assert_allclose(r4, [-2.0, 0.5, 1.25, 3.0], rtol=1e-12)
    r2 = CS.quartic_roots(*(np.polymul([1, -1.5], np.polymul([1, 4.0], [1, 0.4, 1.0]))[:, None] * 3.0))[0]
    np.testing.assert_allclose(r2[:2], [-4.0, 1.5], rtol=1e-12)
    assert np.all(np.isinf(r2[2:]))
    assert np.all(np.isinf(CS.quartic_roots(*np.polymul([1, 0.2, 2.0], [1, -1.0, 5.0])[:, None])[0]))
    assert np.all(np.isinf(CS.quartic_roots(*np.array([0.0, 1.0, -3.0, 3.0, -1.0])[:, None])[0]))    # A4 = 0: skipped


@pytest.mark.parametrize('name', list(FIXTURES))
def test_noise_free_recovery(golden, name):
    """Every noise-free row: all n inliers, and the winning hypothesis itself within the EPnP known-answer bounds."""
    g = golden(name)
    o = CS.consensus_host(g['kp2d'], inlier_px=TAU, min_inliers=MIN_INLIERS, quat=g['q'], pos=g['t'], **cam(g))
    n = g['kp3d'].shape[0]
    ang = angle_deg(o['ori'], g['q'])
    dp = np.linalg.norm(o['pos'] - g['t'], axis=1)
    print(f'{name}: {len(ang)} rows, angle max {ang.max():.2e} deg, position max {dp.max():.2e} m, cost max '
          f'{o["cost"].max():.2e}')
    assert not o['status'].any() and np.all(o['n_inliers'] == n) and np.all(o['inliers'])
    assert ang.max() < KAT_DEG and dp.max() < KAT_M
    assert np.all(np.sum(o['ori'] * g['q'], axis=1) >= 0)      # the start's hemisphere


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('name', list(FIXTURES))
def test_planted_masks(planted_case, name, k):
    """The inlier mask is the planted one on every row: no allowance."""
    g, c, kp, bad, q0, t0, o = planted_case(name, k)
    exact = np.all(o['inliers'] == ~bad, axis=1)
    ang = angle_deg(o['ori'], g['q'][:len(kp)])
    print(f'{name} k = {k}: masks exact {exact.sum()} / {len(exact)}; winning hypothesis orientation error median '
          f'{np.median(ang):.3f} p90 {np.percentile(ang, 90):.3f} max {ang.max():.3f} deg')
    assert exact.all()
    assert not o['status'].any() and np.array_equal(o['n_inliers'], (~bad).sum(1))
    assert np.array_equal(o['weights'], (~bad).astype(np.float32))
    assert o['ori'].dtype == np.float32 and o['pos'].dtype == np.float32 and o['inliers'].dtype == bool
    np.testing.assert_allclose(np.linalg.norm(o['ori'].astype(np.float64), axis=1), 1.0, atol=2e-7)
    assert np.all(np.sum(o['ori'] * q0, axis=1) >= 0)
    tr = CS.triples(bad.shape[1])[o['triple']]
    assert not bad[np.arange(len(kp))[:, None], tr].any()      # a winning sample holds no moved point
    # the helper agrees with the search: the winner's triple has the winning cost, and no triple has a lower one
    assert np.array_equal(CS.triple_cost(kp, triple=o['triple'], inlier_px=TAU, **c), o['cost'])
    assert np.all(CS.triple_cost(kp, triple=0, inlier_px=TAU, **c) >= o['cost'])


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('name', list(FIXTURES))
def test_least_squares_on_the_inliers_is_the_oracle_pose(planted_case, name, k):
    """Plain least squares (50 trials, Huber 0) with the twin's weights from the winning hypothesis lands where the
    same refinement with the planted weights lands from the fixture's true pose."""
    g, c, kp, bad, q0, t0, o = planted_case(name, k)
    B = len(kp)
    got = RF.refine_pose_host(kp, o['ori'], o['pos'], weights=o['weights'], max_iters=50, huber_px=0.0, **c)
    want = RF.refine_pose_host(kp, g['q'][:B], g['t'][:B], weights=(~bad).astype(np.float32), max_iters=50,
                               huber_px=0.0, **c)
    ang = angle_deg(got['ori'], want['ori'])
    dp = np.linalg.norm(got['pos'].astype(np.float64) - want['pos'], axis=1)
    err = angle_deg(got['ori'], g['q'][:B])
    print(f'{name} k = {k}: against the oracle pose, angle median {np.median(ang):.2e} max {ang.max():.2e} deg, '
          f'position median {np.median(dp):.2e} max {dp.max():.2e} m; orientation error median {np.median(err):.3f} '
          f'p90 {np.percentile(err, 90):.3f} max {err.max():.3f} deg')
    assert not got['status'].any() and not want['status'].any()       # in particular no bit 32
    assert np.median(ang) < ANG_MED and ang.max() < ANG_MAX
    assert np.median(dp) < POS_MED and dp.max() < POS_MAX


def test_no_consensus(golden):
    """Eight of eleven points moved: no hypothesis reaches 6 inliers; bit 64 and the start pose, bit for bit."""
    g = golden('keypoints.npz')
    c = cam(g)
    kp, bad = planted(g, 8, 32, seed=19)
    q0, t0 = E.decode_batch(kp, c['kp3d'], c['K'], c['nu'], c['nv'], c['dist'])
    q0, t0 = q0.astype(np.float32), t0.astype(np.float32)
    st = np.zeros(32, np.int32)
    st[5] = 8
    o = CS.consensus_host(kp, inlier_px=TAU, min_inliers=MIN_INLIERS, quat=q0, pos=t0, status=st, **c)
    free = CS.consensus_host(kp, inlier_px=TAU, min_inliers=4, quat=q0, pos=t0, **c)
    print('most inliers of a winning hypothesis per row:', free['n_inliers'])
    assert np.all(free['n_inliers'] < MIN_INLIERS)
    assert np.array_equal(o['status'], st | CS.NO_CONSENSUS) and st[5] == 8 and st.sum() == 8
    assert np.array_equal(o['ori'].view(np.uint32), q0.view(np.uint32))
    assert np.array_equal(o['pos'].view(np.uint32), t0.view(np.uint32))
    assert np.all(o['weights'] == 1) and not o['inliers'].any() and not o['n_inliers'].any()
    assert np.all(np.isnan(o['cost'])) and np.all(o['triple'] == -1) and np.all(o['root'] == -1)
    assert np.all(o['scored'] > 0)


def test_unscored_points(planted_case):
    """Points with weight zero are never inliers and never sampled, whether they fit the pose or not."""
    g, c, kp, bad, q0, t0, ref = planted_case('keypoints.npz', 3)
    B, n = bad.shape
    rng = np.random.default_rng(3)
    w = rng.uniform(0.25, 1.0, (B, n)).astype(np.float32)
    off = np.zeros((B, n), bool)
    for i in range(B):                                   # two good points per row are switched off
        off[i, rng.choice(np.nonzero(~bad[i])[0], 2, replace=False)] = True
    w[off] = 0
    o = CS.consensus_host(kp, weights=w, inlier_px=TAU, min_inliers=MIN_INLIERS, quat=q0, pos=t0, **c)
    assert not o['status'].any()
    assert np.array_equal(o['inliers'], ~bad & ~off) and np.array_equal(o['weights'], np.where(~bad & ~off, w, 0))
    tr = CS.triples(n)[o['triple']]
    assert not off[np.arange(B)[:, None], tr].any()
    # the moved points switched off instead: every remaining point is an inlier
    w2 = np.where(bad, 0, w + off).astype(np.float32)
    o2 = CS.consensus_host(kp, weights=w2, inlier_px=TAU, min_inliers=MIN_INLIERS, quat=q0, pos=t0, **c)
    assert np.array_equal(o2['inliers'], ~bad) and np.array_equal(o2['n_inliers'], (~bad).sum(1))
    assert np.all(o2['scored'] < ref['scored'])


def test_status_rows(planted_case):
    g, c, kp, bad, q0, t0, ref = planted_case('keypoints.npz', 2)
    kp, q0, t0 = kp[:8].copy(), q0[:8].copy(), t0[:8].copy()
    w = np.ones((8, 11), np.float32)
    kp[1, 6] = np.nan                       # a non-finite keypoint
    w[2, 3] = -1.0                          # a negative weight
    w[3, 0] = np.inf
    w[4, 2:] = 0                            # two candidates
    w[5, 6:] = 0                            # five candidates: fewer than min_inliers can ever be inliers
    q0[6] = 0                               # no start orientation: no hemisphere to keep, the row is still solved
    o = CS.consensus_host(kp, weights=w, inlier_px=TAU, min_inliers=MIN_INLIERS, quat=q0, pos=t0, **c)
    assert list(o['status']) == [0, 64, 64, 64, 64, 64, 0, 0]
    for r in range(1, 6):
        assert np.array_equal(o['ori'][r].view(np.uint32), q0[r].view(np.uint32))
        assert np.array_equal(o['pos'][r].view(np.uint32), t0[r].view(np.uint32))
        assert np.array_equal(o['weights'][r], w[r], equal_nan=True) and np.isnan(o['cost'][r])
        assert o['triple'][r] == -1 and o['n_inliers'][r] == 0 and not o['inliers'][r].any()
    for r in (0, 6, 7):
        assert np.array_equal(o['inliers'][r], ~bad[r]) and o['cost'][r] == ref['cost'][r]
    assert abs(np.abs(np.sum(o['ori'][6].astype(np.float64) * ref['ori'][6])) - 1) < 1e-6
    with pytest.raises(AssertionError):
        CS.consensus_host(kp, min_inliers=3, **c)
    with pytest.raises(AssertionError):
        CS.consensus_host(kp, min_inliers=12, **c)
    with pytest.raises(AssertionError):
        CS.consensus_host(kp, inlier_px=0.0, **c)


def test_twin_is_vectorised(golden):
    """96 problems, 165 triples each, in well under a second."""
    g = golden('keypoints.npz')
    kp, _ = planted(g, 4, 96)
    t = time.perf_counter()
    o = CS.consensus_host(kp, inlier_px=TAU, min_inliers=MIN_INLIERS, **cam(g))
    dt = time.perf_counter() - t
    assert not o['status'].any() and dt < 1.0, dt


def test_config_keys(tmp_path):
    from spef_amd.config import keypoint_consensus, keypoint_refine, load_config
    cfg = load_config(None)
    assert cfg.MODEL.HEAD.KEYPOINTS_CONSENSUS_PX == 0.0 and cfg.MODEL.HEAD.KEYPOINTS_CONSENSUS_MIN_INLIERS == 0
    assert keypoint_consensus(cfg) is None and keypoint_refine(cfg) is None
    p = tmp_path / 'c.yaml'
    p.write_text('MODEL:\n  HEAD:\n    ORI: keypoints\n    POS: keypoints\n    KEYPOINTS_CONSENSUS_PX: 8\n')
    assert keypoint_consensus(load_config(str(p))) == (8.0, None)
    p.write_text('MODEL:\n  HEAD:\n    KEYPOINTS_CONSENSUS_PX: 6.5\n    KEYPOINTS_CONSENSUS_MIN_INLIERS: 7\n')
    assert keypoint_consensus(load_config(str(p))) == (6.5, 7)
    p.write_text('MODEL:\n  HEAD:\n    KEYPOINTS_CONSENSUS_SEED: 1\n')
    with pytest.raises(KeyError):
        load_config(str(p))


def test_does_not_import_the_oracle():
    assert 'oracle' not in open(CS.__file__).read()
