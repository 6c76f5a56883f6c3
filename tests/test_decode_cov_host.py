"""The NumPy twin of the pose covariance of the soft-classification decode (spef_amd/spe/decode_cov.py): its inverse
Markley matrix against the reference's own ``h_inv`` (tests/golden/decode_cov.npz), the properties of its theta and t
blocks, its status bits, and the gating scenario that motivates it (``PoseTrackerHost``)."""
import numpy as np
import pytest

from oracle import decode_ref as D
from spef_amd.spe import decode_cov as DC
from spef_amd.spe import track as TK


@pytest.fixture(scope='module')
def fx(golden):
    go, gp, gc = golden('decode_ori.npz'), golden('decode_pos.npz'), golden('decode_cov.npz')
    hist, grid = go['hist'], gp['grid']
    soft = gc['planted_soft']                                             # [3 temperatures][4 rows][1728]
    quat = np.stack([D.decode_orientation_batch(s, hist) for s in soft])  # their own decode, float32
    return dict(hist=hist, grid=grid, rand_soft=go['rand_soft'], rand_hinv=gc['rand_hinv'], soft=soft, quat=quat,
                planted_hinv=gc['planted_hinv'], raised=gc['planted_raised'], temps=gc['temps'], enc=gp['enc'])


def hinv_bound(p, hist, want):
    """(2^-22 + 1e-12 cond(a)) max|h_inv|: float32 rounding with a 4x margin, plus the inverse's sensitivity to a
    1728-term float64 sum taken in another order; cond(a) from the float64 a."""
    return (2.0 ** -22 + 1e-12 * np.linalg.cond(DC.markley_matrix(p, hist))) * np.abs(want).max()


def test_hinv_matches_the_reference(fx):
    rows = [(p, h) for p, h in zip(fx['rand_soft'], fx['rand_hinv'])]
    assert not fx['raised'].any() and np.array_equal(fx['temps'], np.float32([1.0, 0.5, 0.2]))
    rows += [(fx['soft'][t, i], fx['planted_hinv'][t, i]) for t in range(3) for i in range(4)]
    assert len(rows) == 28
    worst = 0.0
    for p, want in rows:
        out = DC.decode_cov_host(p[None], None, np.float32([[1, 0, 0, 0]]), np.zeros((1, 3)), fx['hist'])
        assert out['cov_status'][0] == 0 and out['ori_hinv'].dtype == np.float32
        err, tol = np.abs(out['ori_hinv'][0].astype(np.float64) - want).max(), hinv_bound(p, fx['hist'], want)
        worst = max(worst, err / tol)
        assert err <= tol
    print(f'largest |d h_inv| / bound: {worst:.3f}')


def test_qlog_rows_is_track_qlog(fx):
    """The all-rows-at-once Log of the twin equals spe.track.qlog / qmul row by row, bit for bit."""
    q = fx['quat'][2, 0].astype(np.float64)
    qc = q / np.sqrt(q @ q) * [1.0, -1.0, -1.0, -1.0]
    h = fx['hist']
    loop = np.stack([TK.qlog(TK.qmul(h[i], qc)) for i in range(h.shape[0])])
    assert np.array_equal(loop, DC.qlog_rows(TK.qmul(h.T, qc).T))
    tiny = np.array([[1.0, 1e-9, 0, 0], [-1.0, 0, 2e-9, 0], [1.0, 0, 0, 0]])      # the series branch, the flip
    assert np.array_equal(np.stack([TK.qlog(d) for d in tiny]), DC.qlog_rows(tiny))


def test_one_hot_pdf():
    """All the mass on one bin that is its own decode: the theta block is exactly 0, a has rank one (status 2)."""
    bins = np.array([[1.0, 0, 0, 0], [0.5, 0.5, 0.5, 0.5], [0, 1.0, 0, 0], [0.5, -0.5, 0.5, 0.5], [0, 0, 0.6, 0.8]])
    for k in (0, 1, 3):
        p = np.zeros((1, 5), np.float32)
        p[0, k] = 1.0
        out = DC.decode_cov_host(p, None, bins[k:k + 1].astype(np.float32), np.zeros((1, 3)), bins, floor_var=(0, 0))
        assert out['cov_status'][0] == DC.HINV
        assert not out['cov'][0, :3, :3].any() and np.isnan(out['ori_hinv']).all()
        assert np.array_equal(out['cov'][0, 3:, 3:], 100.0 * np.eye(3, dtype=np.float32))


def test_theta_block_properties(fx):
    tr = np.empty((3, 4))
    for t in range(3):
        out = DC.decode_cov_host(fx['soft'][t], None, fx['quat'][t], np.zeros((4, 3)), fx['hist'], dtype=np.float64)
        assert not out['cov_status'].any()
        for i in range(4):
            blk = out['cov'][i, :3, :3]
            assert np.array_equal(blk, blk.T) and np.linalg.eigvalsh(blk).min() >= 0
            assert not out['cov'][i, :3, 3:].any() and not out['cov'][i, 3:, :3].any()
            tr[t, i] = np.trace(blk)
    print('sigma [deg] per temperature and row:\n', np.degrees(np.sqrt(tr)))
    assert (tr[0] > tr[1]).all() and (tr[1] > tr[2]).all()


def test_uniform_pdf_is_wide(fx):
    n = fx['hist'].shape[0]
    p = np.full((1, n), 1.0 / n, np.float32)
    q = D.decode_orientation_batch(p, fx['hist'])
    out = DC.decode_cov_host(p, None, q, np.zeros((1, 3)), fx['hist'], dtype=np.float64)
    sigma = np.sqrt(np.trace(out['cov'][0, :3, :3]))
    print(f'uniform PDF: trace^1/2 = {sigma:.3f} rad')
    assert sigma > 2.0


def test_t_block(fx):
    """The encoded SPEED positions about their own decode: PSD, and no wider than one grid cell's diagonal plus the
    spread the encoding itself gives every axis ((smooth / bins)^2 / 12 with the fixture's smooth = 100, 10 bins)."""
    grid, enc = fx['grid'], fx['enc']
    pos = D.decode_position_batch(enc, grid)
    out = DC.decode_cov_host(None, enc, np.tile(np.float32([1, 0, 0, 0]), (len(enc), 1)), pos, None, grid,
                             dtype=np.float64)
    assert not out['cov_status'].any()
    cell = np.array([np.diff(np.unique(grid[:, k])).max() for k in range(3)])
    limit = (cell ** 2).sum() + 3 * (100 / 10) ** 2 / 12
    for b in range(len(enc)):
        blk = out['cov'][b, 3:, 3:]
        assert np.array_equal(blk, blk.T) and np.linalg.eigvalsh(blk).min() >= 0
        assert np.array_equal(out['cov'][b, :3, :3], 100.0 * np.eye(3))
        e = grid - pos[b].astype(np.float64)                                       # the centred form, term by term
        want = sum(float(enc[b, i]) * np.outer(e[i], e[i]) for i in range(len(grid))) / enc[b].astype(np.float64).sum()
        assert np.abs(blk - want).max() <= 1e-12 * np.abs(want).max()
        assert np.trace(blk) < limit
    print(f'largest t-block trace {np.trace(out["cov"][:, 3:, 3:], axis1=1, axis2=2).max():.3f} m^2, limit {limit:.3f}')


def test_status_bits_floors_and_modes(fx):
    hist, grid = fx['hist'], fx['grid']
    op = np.stack([fx['soft'][2, 0]] * 5)
    pp = np.stack([fx['enc'][0]] * 5)
    q = np.tile(fx['quat'][2, 0], (5, 1))
    t = np.tile(D.decode_position_batch(pp[:1], grid), (5, 1))
    op[1, 7] = np.nan
    op[2] = 0.0
    pp[3, 5] = np.nan
    pp[4] = 0.0
    q[4] = np.nan
    out = DC.decode_cov_host(op, pp, q, t, hist, grid, dtype=np.float64)
    assert out['cov_status'].tolist() == [0, DC.ORI | DC.HINV, DC.ORI | DC.HINV, DC.POS, DC.ORI | DC.POS]
    for b, (nan_o, nan_p) in enumerate([(0, 0), (1, 0), (1, 0), (0, 1), (1, 1)]):
        assert np.isnan(out['cov'][b, :3, :3]).all() == bool(nan_o) and np.isnan(out['cov'][b, 3:, 3:]).all() == bool(nan_p)
        assert np.isfinite(out['cov'][b, :3, :3]).all() != bool(nan_o)
        assert not out['cov'][b, :3, 3:].any() and not out['cov'][b, 3:, :3].any()
    assert np.isnan(out['ori_hinv'][1]).all() and np.isnan(out['ori_hinv'][2]).all()
    assert np.isfinite(out['ori_hinv'][[0, 3, 4]]).all()                        # inv(a) does not depend on the pose

    fl = DC.decode_cov_host(op[:1], pp[:1], q[:1], t[:1], hist, grid, floor_var=(0.25, 4.0), dtype=np.float64)
    diff = fl['cov'][0] - out['cov'][0]
    assert np.allclose(np.diag(diff), [0.25] * 3 + [4.0] * 3, rtol=0, atol=1e-12) and not (diff - np.diag(np.diag(diff))).any()
    reg = DC.decode_cov_host(None, None, q[:1], t[:1], fixed_var=(3.0, 7.0), floor_var=(0.25, 4.0))
    assert np.array_equal(reg['cov'][0], np.diag([3.0] * 3 + [7.0] * 3).astype(np.float32)) and reg['cov_status'][0] == 0
    for bad in (dict(fixed_var=(-1.0, 1.0)), dict(floor_var=(0.0, np.nan))):
        with pytest.raises(AssertionError):
            DC.decode_cov_host(None, None, q[:1], t[:1], **bad)


def test_gating_scenario(fx):
    """A still track of the T = 0.2 planted PDF of one pose whose frame 5 is the T = 0.2 PDF of another pose, the one
    farthest from it: with the fixed r = (100, 100) the Mahalanobis gate cannot fire; with the PDFs' own covariance it
    does. q = 1e-4, p0 = 1, chi2(6 dof, 99 %) = 16.81."""
    quat = fx['quat'][2].astype(np.float64)
    ang = 2 * np.arccos(np.minimum(1.0, np.abs(quat[1:] @ quat[0])))
    k = 1 + int(np.argmax(ang))
    assert ang.max() > 1.0, ang                                                    # the scenario's own precondition
    rows = [0] * 8
    rows[5] = k
    q = fx['quat'][2][rows]
    t = np.tile(np.float32([0.1, -0.2, 9.0]), (8, 1))
    prm = dict(q=1e-4, p0=1.0, gate_chi2=16.81)
    cov = DC.decode_cov_host(fx['soft'][2][rows], None, q, t, fx['hist'], fixed_var=TK.DEFAULTS['r'])['cov']
    fixed = TK.PoseTrackerHost(1, **prm).step(q, t)
    pdf = TK.PoseTrackerHost(1, **prm).step(q, t, cov)
    print(f'outlier {np.degrees(ang.max()):.1f} deg off; d2 with r = 100: {fixed["mahalanobis"][5]:.3f}, with the '
          f'PDF covariance: {pdf["mahalanobis"][5]:.1f}; sigma [deg] {np.degrees(np.sqrt(np.trace(cov[0, :3, :3]))):.1f}')
    assert not fixed['track_status'].any()
    assert pdf['track_status'][5] & TK.GATED and not pdf['track_status'][:5].any()
