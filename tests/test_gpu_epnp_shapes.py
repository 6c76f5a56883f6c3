"""GPU: the batched EPnP decode (csrc/k_epnp.hip + spef_set_keypoints) away from the one 11-point Tango model and the
two reference cameras: every point count the ABI accepts (4..16) at its ends, a non-square off-centre camera, the
distortion edges (4-coefficient form, the icdist < 0 fallback of undistortPoints), status bit 8, the sigmoid's tails
and a failed spef_set_keypoints. The inputs and the oracle's answers come from tests/epnp_inputs.py, once per run; the
bounds are those of tests/test_gpu_keypoints.py."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

from oracle import decode_ref as D
from spef_amd import _lib as L
from spef_amd import blob as Bl
from spef_amd.arch import mobilenet_v2
from spef_amd.weights import synthetic_state_dict

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epnp_inputs as I  # noqa: E402
from refine_inputs import noisy  # noqa: E402

pytestmark = pytest.mark.gpu

# GPU against oracle: the bounds of test_epnp_matches_oracle_on_noisy_keypoints
ANG_MED, ANG_MAX, POS_MED, POS_MAX = 1e-4, 0.1, 1e-5, 1e-3
# GPU against the true pose, noise-free: the bounds of test_epnp_noise_free_kat
KAT_ANG, KAT_POS = 5e-4, 2e-4


@pytest.fixture(scope='module')
def eng(golden):
    from spef_amd.engine import Engine
    arch = mobilenet_v2('keypoints')
    e = Engine(Bl.pack(synthetic_state_dict(arch, seed=1001, head_std=0.002), arch, dtype='fp32'), 'cuda:0')
    _golden_cfg(e, golden)
    yield e
    e.close()


def _golden_cfg(eng, golden):
    g = golden('keypoints.npz')
    eng.set_keypoint_refine(None)
    eng.set_keypoints(g['kp3d'], g['K'], float(g['nu']), float(g['nv']))
    return g


@contextlib.contextmanager
def _configured(eng, golden, pts, cam, dist=None):
    """Another model / camera for the body; the golden configuration again afterwards, whatever happened."""
    try:
        eng.set_keypoints(pts, cam.K, cam.nu, cam.nv, dist)
        yield
    finally:
        _golden_cfg(eng, golden)


def _decode(eng, kp, apply_sigmoid=False):
    out = eng.decode_keypoints(torch.from_numpy(np.ascontiguousarray(kp)).cuda(), apply_sigmoid=apply_sigmoid)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _errors(out, q, t):
    ang = D.angle_deg_stable(out['ori'], q)
    dp = np.linalg.norm(out['pos'].astype(np.float64) - t, axis=1)
    return ang, dp


def _assert_matches_oracle(tag, out, rq, rt):
    ang, dp = _errors(out, rq, rt)
    print(f'{tag}: angle median {np.median(ang):.2e} max {ang.max():.2e} deg, position median {np.median(dp):.2e} '
          f'max {dp.max():.2e} m, status rows {np.flatnonzero(out["status"]).tolist()}')
    assert not out['status'].any()
    assert np.median(ang) < ANG_MED and ang.max() < ANG_MAX
    assert np.median(dp) < POS_MED and dp.max() < POS_MAX


def _assert_row_alone(eng, kp, out, row):
    """B = 1 and the block index: the row decoded alone equals the row of the batch bit for bit."""
    lone = _decode(eng, kp[row:row + 1])
    for k in ('ori', 'pos', 'status', 'keypoints'):
        assert np.array_equal(_bits(lone[k][0]), _bits(out[k][row])), k


@pytest.mark.parametrize('px', I.NOISE_PX)
@pytest.mark.parametrize('camera', I.CAMERAS)
@pytest.mark.parametrize('n', I.SWEEP_N)
def test_point_count_sweep_matches_oracle(eng, golden, n, camera, px):
    """(a): n = 6, 7, 12 and 16 = EPNP_MAXN seeded points in +-0.5 m, the SPEED camera and a non-square off-centre
    one, the first 64 golden poses, noise-free and with 1 px Gaussian noise: the kernel against oracle/epnp_ref.py at
    the bounds of test_epnp_matches_oracle_on_noisy_keypoints, no status bit, and row 63 alone equal to row 63 of the
    batch. From n = 6 on the pose does not depend on the eigen-solver (SVD against eigh with random signs: the
    oracle's float32 outputs are identical), so the comparison is meaningful at these bounds."""
    g = golden('keypoints.npz')
    c = I.case(g, n, camera, px)
    assert c['inside'] >= 0.9, c['inside']
    with _configured(eng, golden, c['pts'], c['cam']):
        out = _decode(eng, c['kp'])
        _assert_row_alone(eng, c['kp'], out, I.B - 1)
    _assert_matches_oracle(f'n = {n}, {camera} camera, {px} px', out, c['rq'], c['rt'])


@pytest.mark.parametrize('camera', I.CAMERAS)
@pytest.mark.parametrize('n', I.KAT_MODELS)
def test_noise_free_known_answers(eng, golden, n, camera):
    """(b): noise-free projections of the first 64 golden poses, n = 5, 6, 16 and the 8 corners of a +-0.3 m cube,
    both cameras: the true pose within the bounds of test_epnp_noise_free_kat (5e-4 deg, 2e-4 m). The oracle, through
    the same float32 pixels, is within 1.05e-4 deg and 7.3e-5 m of the truth on these inputs (its own measurement:
    the far poses, 29 m, see one float32 pixel ulp as ~3e-5 m). n = 5 and the cube are compared with the truth only:
    at n = 5 the null space of M^T M is 2-dimensional and with noise the tail of the solve depends on the basis a
    solver returns (3.1 deg between SVD and eigh on the 1 px rows; noise-free it is well defined); the cube has three equal PCA eigenvalues, so its control-point
    axes are arbitrary and the host Jacobi and the oracle's SVD need not choose the same ones."""
    g = golden('keypoints.npz')
    c = I.case(g, n, camera, 0.0)
    assert c['inside'] >= 0.9, c['inside']
    with _configured(eng, golden, c['pts'], c['cam']):
        out = _decode(eng, c['kp'])
    ang, dp = _errors(out, c['q'], c['t'])
    print(f'known answers, model {n}, {camera} camera: angle max {ang.max():.2e} deg, position max {dp.max():.2e} m')
    assert not out['status'].any()
    assert ang.max() < KAT_ANG and dp.max() < KAT_POS


@pytest.mark.parametrize('px', I.NOISE_PX)
def test_four_points_properties_only(eng, golden, px):
    """(c): n = 4, the fewest points the ABI accepts (the four spanning Tango points of test_lane_bounds). M^T M has
    8 rows, so its null space is 4-dimensional and EPnP's answer depends on the basis the eigen-solver returns for
    it, even noise-free: that is the algorithm's limit, not the
    kernel's (the oracle with SVD and with eigh + random signs are 43 deg apart on these rows), so there is no
    comparison with the oracle or the truth. Every row either reports bit 8 or holds a
    finite position and a unit quaternion."""
    g = golden('keypoints.npz')
    pts = np.ascontiguousarray(g['kp3d'][[0, 2, 5, 10]], np.float32)
    assert np.linalg.svd(pts - pts.mean(0), compute_uv=False).min() > 0.05
    cam = I.speed_camera(g)
    q, t = I.poses(g, 'speed')
    kp = I.add_noise(I.project(cam, pts, q, t), cam, px, 4)
    with _configured(eng, golden, pts, cam):
        out = _decode(eng, kp)
        _assert_row_alone(eng, kp, out, I.B - 1)
    bad = (out['status'] & 8) != 0
    print(f'n = 4, {px} px: rows with bit 8: {np.flatnonzero(bad).tolist()}')
    assert not (out['status'] & ~8).any()
    ok = ~bad
    assert np.isfinite(out['pos'][ok]).all() and np.isfinite(out['ori'][ok]).all()
    assert np.abs(np.linalg.norm(out['ori'][ok].astype(np.float64), axis=1) - 1).max(initial=0) < 1e-6


def test_every_approximation_wins(golden):
    """(d): a condition on the inputs of (a), by the oracle alone (tests/test_epnp_inputs_host.py checks it without a
    GPU): over the 512 noisy rows each of the three beta approximations -- one per wave in the kernel -- has the lowest
    reprojection error in at least 5 % of the rows, so agreement with the oracle in (a) covers every wave's path."""
    win = I.noisy_sweep_winners(golden('keypoints.npz'))
    counts = np.bincount(win, minlength=4)[1:]
    print(f'winning approximation 1 / 2 / 3 over {win.size} noisy rows: {counts.tolist()}')
    assert win.size == 512 and counts.sum() == 512 and (counts >= 0.05 * win.size).all()


@pytest.mark.parametrize('kind', I.DIST_KINDS)
def test_distortion_edges_match_oracle(eng, golden, kind):
    """(e): the SPEED+ K, n = 11, 1 px noise, GPU against oracle on the same pixels at the bounds of (a).
    '4coef_mild': the fixture's (k1, k2, p1, p2) without k3; '4coef' and '5coef': k1 = -12 without and with k3, so
    that 1 + k1 r^2 + ... turns negative for the outermost keypoints and undistortPoints keeps the distorted point
    (icdist < 0): the oracle's undistort_points takes that branch for 51 and 52 of the 704 points, in 17 rows, and for
    none with the mild coefficients. The pixels are the fixture's projections, no physical image through that lens:
    the same input on both sides is what the comparison needs."""
    gp = golden('keypoints_speedplus.npz')
    c = I.distortion_case(gp, kind)
    fell = c['fell']
    print(f'{kind}: fallback points {int(fell.sum())} of {fell.size}, in {int(fell.any(1).sum())} rows')
    if kind == '4coef_mild':
        assert not fell.any()
    else:
        assert fell.sum() >= 1 and fell.mean() < 0.5
    with _configured(eng, golden, gp['kp3d'], c['cam'], c['dist']):
        out = _decode(eng, c['kp'])
        _assert_row_alone(eng, c['kp'], out, I.B - 1)
    _assert_matches_oracle(f'distortion {kind}', out, c['rq'], c['rt'])


def _unit_and_finite(out, r):
    return (np.isfinite(out['ori'][r]).all() and np.isfinite(out['pos'][r]).all()
            and abs(np.linalg.norm(out['ori'][r].astype(np.float64)) - 1) < 1e-6)


def test_status_rows(eng, golden):
    """(f): golden configuration, 8 noisy rows. A NaN keypoint (row 1) sets bit 8; a NaN in the origin pair (row 2) is
    dropped with the origin before EPnP, so the row decodes to its clean result; 11 keypoints at one pixel (row 3) give
    bit 8 or a finite pose with a unit quaternion; the other rows equal those of the clean batch bit for bit."""
    g = _golden_cfg(eng, golden)
    kp = noisy(g, 5, 3.0, 8)
    clean = _decode(eng, kp)
    assert not clean['status'].any()
    bad = kp.copy()
    bad[1, 2 + 2 * 4] = np.nan
    bad[2, 1] = np.nan
    bad[3, 2::2], bad[3, 3::2] = 0.4, 0.6
    out = _decode(eng, bad)
    print(f'status rows: {out["status"].tolist()}')
    assert out['status'][1] == 8
    assert out['status'][3] == 8 or (out['status'][3] == 0 and _unit_and_finite(out, 3))
    for r in (0, 2, 4, 5, 6, 7):
        assert out['status'][r] == 0
        for k in ('ori', 'pos'):
            assert np.array_equal(_bits(out[k][r]), _bits(clean[k][r])), (k, r)


def test_sigmoid_tails(eng, golden):
    """(f): logits of +-20, +-90 and +-inf through apply_sigmoid: 'keypoints' equals the float32 sigmoid at the
    tolerance of test_sigmoid_then_epnp, and is exactly 0 or 1 where that is."""
    g = _golden_cfg(eng, golden)
    inside = np.all((g['kp2d'] > 1e-3) & (g['kp2d'] < 1 - 1e-3), axis=1)
    kp = g['kp2d'][inside][:8].astype(np.float64)
    logit = np.log(kp / (1 - kp)).astype(np.float32)
    for r, (col, v) in enumerate([(0, 20.0), (23, -20.0), (5, 90.0), (6, -90.0), (1, np.inf), (22, -np.inf)]):
        logit[r, col] = v
    with np.errstate(over='ignore'):
        sig = D.sigmoid_f32(logit)
    assert sig[2, 5] == 1 and sig[3, 6] == 0 and sig[4, 1] == 1 and sig[5, 22] == 0
    out = _decode(eng, logit, apply_sigmoid=True)
    np.testing.assert_allclose(out['keypoints'], sig, rtol=2e-6, atol=1e-7)
    exact = (sig == 0) | (sig == 1)
    assert np.array_equal(out['keypoints'][exact], sig[exact])
    for r in (6, 7):            # untouched rows still decode
        assert out['status'][r] == 0 and _unit_and_finite(out, r)


def _coplanar():
    pts = np.random.default_rng(6).uniform(-0.5, 0.5, (6, 3)).astype(np.float32)
    pts[:, 2] = 0.0             # z == 0 exactly: the third control point coincides with the centroid, det == 0
    return pts


def test_failed_set_keypoints_keeps_the_configuration(eng, golden):
    """(g): spef_set_keypoints is all or nothing. A coplanar model (ERR_ARG: degenerate), n = 3 and n = 17 (ERR_ARG)
    leave the golden configuration in place: decode and refine give the results they gave before, bit for bit."""
    g = _golden_cfg(eng, golden)
    try:
        kp = noisy(g, 5, 3.0, 8)
        a = _decode(eng, kp)

        def refine():
            r = eng.refine_keypoints(torch.from_numpy(kp).cuda(), torch.from_numpy(a['ori']).cuda(),
                                     torch.from_numpy(a['pos']).cuda(), max_iters=50, huber_px=4.0, want_cov=True)
            return {k: v.cpu().numpy() for k, v in r.items()}
        ra = refine()
        cam = I.second_camera()
        for pts in (_coplanar(), np.zeros((3, 3), np.float32) + np.eye(3, dtype=np.float32),
                    np.random.default_rng(17).uniform(-0.5, 0.5, (17, 3)).astype(np.float32)):
            with pytest.raises(AssertionError):          # _lib.check: ERR_ARG
                eng.set_keypoints(pts, cam.K, cam.nu, cam.nv, [-0.2, 0.1, 0.0, 0.0])
            assert eng.lib.spef_set_keypoints(eng.ctx, pts.ctypes.data, pts.shape[0], cam.K.ctypes.data, cam.nu,
                                              cam.nv) == L.ERR_ARG
            assert np.array_equal(eng._kp[0], g['kp3d'])
            b = _decode(eng, kp)
            for k in ('keypoints', 'ori', 'pos', 'status'):
                assert np.array_equal(_bits(b[k]), _bits(a[k])), (k, pts.shape)
            rb = refine()
            for k in ('ori', 'pos', 'fit', 'cov', 'iters', 'status'):
                assert np.array_equal(_bits(rb[k]), _bits(ra[k])), (k, pts.shape)
    finally:
        _golden_cfg(eng, golden)


def test_failed_set_keypoints_leaves_a_fresh_context_unconfigured(eng, golden):
    """(g): on a context that never had keypoints the same failing call leaves it unconfigured: decode and refine
    return ERR_STATE and write nothing."""
    from spef_amd.engine import Engine, _ptr, _stream
    g = golden('keypoints.npz')
    cam = I.second_camera()
    kp = torch.from_numpy(noisy(g, 5, 3.0, 8)).cuda()
    sentinel = 12345.0
    q = torch.full((8, 4), sentinel, device='cuda')
    t = torch.full((8, 3), sentinel, device='cuda')
    kpo = torch.full_like(kp, sentinel)
    st = torch.full((8,), 77, dtype=torch.int32, device='cuda')
    empty = Engine(None, 'cuda:0')
    try:
        with pytest.raises(AssertionError):
            empty.set_keypoints(_coplanar(), cam.K, cam.nu, cam.nv)
        assert getattr(empty, '_kp', None) is None
        s = _stream(empty.device)
        assert empty.lib.spef_decode_keypoints(empty.ctx, _ptr(kp), 8, 0, _ptr(kpo), _ptr(q), _ptr(t), _ptr(st),
                                               s) == L.ERR_STATE
        assert empty.lib.spef_refine_keypoints(empty.ctx, _ptr(kp), None, 8, 50, 4.0, _ptr(q), _ptr(t), None, None,
                                               None, _ptr(st), s) == L.ERR_STATE
        torch.cuda.synchronize()
    finally:
        empty.close()
    assert (q == sentinel).all().item() and (t == sentinel).all().item() and (kpo == sentinel).all().item()
    assert (st == 77).all().item()
