"""The host twin of the scoring kernels (spef_amd/score.py): the arithmetic the kernels of csrc/k_score.hip follow,
against the reference's own get_score (tests/golden/score.npz) and against NumPy's statistics; the row flags; the
binding table."""
import numpy as np
import pytest

from spef_amd import _lib
from spef_amd import score as SC


def _poses(n, seed, ori_noise=0.05, pos_noise=0.1):
    rng = np.random.Generator(np.random.PCG64(seed))
    qt = rng.normal(size=(n, 4))
    qt = (qt / np.linalg.norm(qt, axis=1, keepdims=True)).astype(np.float32)
    tt = (rng.normal(size=(n, 3)) * [0.3, 0.3, 3.0] + [0, 0, 10]).astype(np.float32)
    qp = qt + rng.normal(size=(n, 4)).astype(np.float32) * np.float32(ori_noise)
    qp = (qp / np.linalg.norm(qp, axis=1, keepdims=True)).astype(np.float32)
    qp[::3] *= -1                                         # q and -q are the same rotation
    tp = (tt + rng.normal(size=(n, 3)) * pos_noise).astype(np.float32)
    return qp, tp, qt, tt


def test_twin_matches_reference_fixture(golden):
    """The specified arithmetic lands 2.4e-6 (ori_score, ori_error), 1.9e-6 (esa_score), 1.0e-7 (pos_score), 8.9e-9
    (pos_error) from the reference's get_score (the float32 dot product near 1, where acos is ill-conditioned):
    1e-5 for the orientation and ESA figures, 1e-6 for the position figures."""
    g = golden('score.npz')
    rows, flags = SC.score_rows(g['q_pred'], g['t_pred'], g['q_true'], g['t_true'])
    assert not flags.any() and np.isfinite(rows).all()
    got = SC.get_score({'ori': g['q_true'], 'pos': g['t_true']}, {'ori': g['q_pred'], 'pos': g['t_pred']})
    for k, tol in (('ori_score', 1e-5), ('ori_error', 1e-5), ('esa_score', 1e-5), ('pos_score', 1e-6),
                   ('pos_error', 1e-6)):
        rel = abs(got[k] / float(g[k]) - 1)
        print(f'{k}: twin {got[k]!r} fixture {float(g[k])!r} rel {rel:.2e}')
        assert rel < tol, (k, rel)
    # 2 atan2(|a - b|, |a + b|) is the angle between the unit quaternions (oracle.decode_ref.angle_deg_stable), half
    # the rotation angle: ori_rad = 2 * ori_stable to the acos form's own resolution near 0 (~0.04 deg = 7e-4 rad)
    assert np.abs(2 * rows[:, 4] - rows[:, 2]).max() < 7e-4


@pytest.mark.parametrize('n', [1, 2, 3, 64, 257, 1800])
def test_twin_statistics_match_numpy(n):
    qp, tp, qt, tt = _poses(n, seed=n)
    rows, flags = SC.score_rows(qp, tp, qt, tt)
    assert not flags.any()
    st = SC.score_stats(rows, flags)
    assert st['n'] == n and st['n_bad'] == 0 and st['n_dropped'] == 0 and st['flags'] == 0
    deg, pe = rows[:, 3], rows[:, 0]
    for tag, x in (('ori', deg), ('pos', pe)):            # order statistics: exactly NumPy's on the float32 rows
        med = np.median(x)
        assert st[f'{tag}_median'] == float(med)
        assert st[f'{tag}_mad'] == float(np.median(np.abs(x - med)))
        assert st[f'{tag}_min'] == float(x.min()) and st[f'{tag}_max'] == float(x.max())
    # means and std: two summation orders of non-negative float64 terms differ by at most n * 2^-52 relative
    tol = n * 2.0 ** -52
    x64 = rows.astype(np.float64)
    for k, want in (('ori_score', x64[:, 2].mean()), ('pos_score', x64[:, 1].mean()), ('pos_error', x64[:, 0].mean()),
                    ('ori_error', x64[:, 2].mean() * 180 / np.pi), ('ori_std', x64[:, 3].std()),
                    ('pos_std', x64[:, 0].std())):
        assert abs(st[k] - want) <= tol * abs(want) + 1e-300, (k, st[k], want)
    assert st['esa_score'] == st['ori_score'] + st['pos_score']


def test_flags():
    q = np.array([[0.5, 0.5, 0.5, 0.5]], np.float32)
    t = np.array([[0.1, -0.2, 8.0]], np.float32)
    rows, flags = SC.score_rows(-q, t, q, t)              # q against -q: no error at all
    assert flags[0] == 0 and (rows[0] == 0).all()
    rows, flags = SC.score_rows(q * np.float32(1.02), t, q, t)           # unnormalised: dot = 1.0404 > 1.01
    assert flags[0] == SC.FLAG_DOT and np.isnan(rows[0]).all()
    rows, flags = SC.score_rows(q * np.float32(1.004), t, q, t)          # 1 < dot <= 1.01: clamped, not flagged
    assert flags[0] == 0 and rows[0, 2] == 0
    bad = t.copy()
    bad[0, 1] = np.nan
    rows, flags = SC.score_rows(q, bad, q, t)
    assert flags[0] == SC.FLAG_NONFINITE and np.isnan(rows[0]).all()
    rows, flags = SC.score_rows(q, t, q, np.zeros((1, 3), np.float32))
    assert flags[0] == SC.FLAG_ZERO_TARGET and np.isnan(rows[0]).all()
    rows, flags = SC.score_rows(q, t, q, t, status=np.array([4]))
    assert flags[0] == SC.FLAG_STATUS and np.isnan(rows[0]).all()
    with pytest.raises(ValueError):
        SC.get_score({'ori': q, 'pos': t}, {'ori': q * np.float32(1.02), 'pos': t})


def test_flagged_rows_enter_no_statistic():
    qp, tp, qt, tt = _poses(40, seed=7)
    tp[5, 0] = np.inf
    tt[17] = 0
    rows, flags = SC.score_rows(qp, tp, qt, tt)
    st = SC.score_stats(rows, flags, n_dropped=3)
    keep = np.ones(40, bool)
    keep[[5, 17]] = False
    assert st['n'] == 38 and st['n_bad'] == 2 and st['n_dropped'] == 3
    assert st['flags'] == (SC.FLAG_NONFINITE | SC.FLAG_ZERO_TARGET)
    assert st['pos_median'] == float(np.median(rows[keep, 0])) and st['ori_max'] == float(rows[keep, 3].max())
    assert abs(st['pos_error'] - rows[keep, 0].astype(np.float64).mean()) < 1e-14
    empty = SC.score_stats(rows[[5, 17]], flags[[5, 17]])
    assert empty['n'] == 0 and empty['n_bad'] == 2
    assert all(np.isnan(empty[k]) for k in SC.STAT_FIELDS if k not in ('n', 'n_bad', 'n_dropped', 'flags'))


def test_binding_table():
    for name in ('spef_score_create', 'spef_score_reset', 'spef_score_step', 'spef_score_finalize',
                 'spef_score_destroy'):
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 4
    assert len(SC.STAT_FIELDS) == 19 and len(SC.ROW_FIELDS) == 5
