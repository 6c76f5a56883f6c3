"""CPU: the pose tracker's NumPy twin (spef_amd/spe/track.py), the specification of csrc/k_track.hip."""
import os
import sys

import numpy as np
import pytest

from spef_amd.spe import track as TK

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_inputs as TI  # noqa: E402


def _run(inputs, n_streams=1, **params):
    trk = TK.PoseTrackerHost(n_streams, **(params or TI.PARAMS))
    qm, tm, cov, st = inputs
    return trk.step(qm, tm, cov, st), trk


@pytest.fixture(scope='module')
def runs():
    """The twin on the H3 / H4 / H5 inputs, each alone; computed once and left unchanged."""
    return {k: _run(f())[0] for k, f in (('standard', TI.standard), ('dropouts', TI.dropouts), ('jump', TI.jump))}


def test_noise_free_known_answer():
    """H1: 16 noise-free frames of the constant-rate trajectory give back w and v to 1e-12."""
    q, t = TI.truth(16)
    trk = TK.PoseTrackerHost(1, q=0, p0=1, r=1e-10)
    out = trk.step(q, t)
    err_w = np.abs(out['rates'][-1, :3] - TI.W_TRUE).max()
    err_v = np.abs(out['rates'][-1, 3:] - TI.V_TRUE).max()
    print(f'rate errors after 16 frames: w {err_w:.2e} rad, v {err_v:.2e} m')
    assert not out['track_status'].any()
    assert err_w <= 1e-12 and err_v <= 1e-12


def test_reference_anchor(golden):
    """H2: configured like the reference's KalmanFilterPosSimple (q = p0 = 1, r = 100, no gate, no covariance) the
    position output is the reference's, to 1e-12 m."""
    g = golden('kalman_pos.npz')
    assert g['pos_in'].shape == (40, 3) and g['pos_in'].dtype == np.float64
    out = TK.PoseTrackerHost(1, **TI.ANCHOR).step(np.tile([1.0, 0, 0, 0], (40, 1)), g['pos_in'])
    diff = np.abs(out['pos'] - g['pos_out']).max()
    print(f'largest difference from the reference filter: {diff:.2e} m')
    assert not out['track_status'].any()
    assert diff <= 1e-12
    assert TK.DEFAULTS == dict(q=(1.0,) * 4, p0=(1.0,) * 4, r=(100.0, 100.0), cov_scale=1.0, gate_chi2=0.0,
                               max_coast=0)


def test_smoothing(runs):
    """H3: no row is flagged, and over frames 32..63 the tracked median errors are at most half the measurements'."""
    qm, tm, _, _ = TI.standard()
    q, t = TI.truth()
    out = runs['standard']
    a_m, a_t = np.degrees(TI.angle_rad(qm, q))[32:], np.degrees(TI.angle_rad(out['ori'], q))[32:]
    p_m, p_t = np.linalg.norm(tm - t, axis=1)[32:], np.linalg.norm(out['pos'] - t, axis=1)[32:]
    print(f'orientation median {np.median(a_m):.3f} -> {np.median(a_t):.3f} deg, position {np.median(p_m):.4f} -> '
          f'{np.median(p_t):.4f} m, largest d2 {out["mahalanobis"].max():.2f}')
    assert not out['track_status'].any()
    assert out['mahalanobis'].max() < 0.9 * TI.GATE
    assert np.median(a_t) <= 0.5 * np.median(a_m)
    assert np.median(p_t) <= 0.5 * np.median(p_m)


def test_dropouts_and_outlier(runs):
    """H4: status 1 on the frames whose decode failed, 2 on the outlier, 0 elsewhere; no other row near the gate; the
    coasted output at the outlier is closer to the truth than its measurement."""
    qm, tm, _, _ = TI.dropouts()
    q, t = TI.truth()
    out = runs['dropouts']
    want = np.zeros(TI.N, np.int32)
    want[20:26] = 1
    want[40] = 2
    d2 = out['mahalanobis']
    others = np.delete(np.arange(TI.N), list(range(20, 26)) + [40])
    print(f'd2 at the outlier {d2[40]:.0f}, largest elsewhere {d2[others].max():.2f}')
    assert np.array_equal(out['track_status'], want)
    assert np.all(np.isnan(d2[20:26])) and d2[40] > TI.GATE
    assert np.all(np.abs(d2[others] - TI.GATE) > 0.1 * TI.GATE)
    assert TI.angle_rad(out['ori'][40], q[40]) < TI.angle_rad(qm[40], q[40])
    assert np.linalg.norm(out['pos'][40] - t[40]) < np.linalg.norm(tm[40] - t[40])
    assert np.all(np.isfinite(out['ori'])) and np.all(np.isfinite(out['pos']))


def test_reinitialisation(runs):
    """H5: a permanent jump is gated for max_coast = 3 frames, then the track starts again from the measurement."""
    qm, tm, _, _ = TI.jump()
    out = runs['jump']
    want = np.zeros(TI.N, np.int32)
    want[30:34] = (2, 2, 2, 6)
    assert np.array_equal(out['track_status'], want)
    assert np.array_equal(out['ori'][33], qm[33] / np.linalg.norm(qm[33])) and np.array_equal(out['pos'][33], tm[33])
    assert np.array_equal(out['rates'][33], np.zeros(6))


def test_cutting(runs):
    """H6: one call of T = 64, 64 calls of T = 1 and 5 + 59 agree bit for bit in outputs and state; three streams
    side by side equal each one alone; state -> set_state into a fresh tracker continues bit for bit."""
    keys = ('ori', 'pos', 'mahalanobis', 'track_status', 'cov', 'rates')
    inp = TI.dropouts()
    whole, trk = _run(inp)
    for cuts in ([1] * 64, [5, 59]):
        t2 = TK.PoseTrackerHost(1, **TI.PARAMS)
        parts, a = [], 0
        for n in cuts:
            parts.append(t2.step(*(x[a:a + n] for x in inp)))
            a += n
        for k in keys:
            assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k], equal_nan=True), (k, cuts[0])
        assert np.array_equal(t2.state(), trk.state())
    three, trk3 = _run(TI.three_streams(), 3)
    for s, name in enumerate(('standard', 'dropouts', 'jump')):
        for k in keys:
            assert np.array_equal(three[k][s::3], runs[name][k], equal_nan=True), (name, k)
    assert np.array_equal(trk3.state(1, 1), trk.state())
    first = TK.PoseTrackerHost(1, **TI.PARAMS)
    first.step(*(x[:23] for x in inp))                  # cut inside the dropout
    second = TK.PoseTrackerHost(1, **TI.PARAMS)
    second.set_state(first.state())
    rest = second.step(*(x[23:] for x in inp))
    for k in keys:
        assert np.array_equal(rest[k], whole[k][23:], equal_nan=True), k
    assert np.array_equal(second.state(), trk.state())
    assert first.state().shape == (1, TK.STATE_DOUBLES)


def test_edges():
    """H7: an invalid first frame passes through (status 9); a NaN in cov falls back to r; an S that is not positive
    definite counts as invalid; the output quaternion never flips sign although the inputs' signs alternate."""
    qm, tm, cov, st = TI.standard()
    bad = st.copy()
    bad[0] = 8
    qx = qm.copy()
    qx[0] = [3.0, 0, 0, 4.0]
    out = _run((qx, tm, cov, bad))[0]
    assert out['track_status'][0] == 9 and np.isnan(out['mahalanobis'][0]) and out['track_status'][1] == 0
    assert np.array_equal(out['ori'][0], qx[0]) and np.array_equal(out['pos'][0], tm[0])
    assert np.array_equal(out['ori'][1], qm[1] / np.linalg.norm(qm[1])) and out['mahalanobis'][1] == 0.0
    nanq = qm.copy()
    nanq[0, 2] = np.nan
    assert _run((nanq, tm, cov, st))[0]['track_status'][0] == 9
    assert _run((np.zeros_like(qm), tm, cov, st))[0]['track_status'].tolist() == [9] * TI.N

    p = dict(TI.PARAMS, r=(1e-4, 1e-2), gate_chi2=0.0)
    holes = cov.copy()
    holes[5, 2, 3] = np.nan
    fixed = cov.copy()
    fixed[5] = np.diag(np.repeat([1e-4, 1e-2], 3))
    a, b = _run((qm, tm, holes, st), **p)[0], _run((qm, tm, fixed, st), **p)[0]
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert not a['track_status'].any()

    neg = cov.copy()
    neg[7] = -np.eye(6) * 10.0
    out = _run((qm, tm, neg, st))[0]
    assert out['track_status'][7] == 1 and np.isnan(out['mahalanobis'][7]) and not np.delete(out['track_status'], 7).any()

    alt = qm * np.where(np.arange(TI.N) % 2, -1.0, 1.0)[:, None]
    out = _run((alt, tm, cov, st))[0]
    assert np.all(np.sum(out['ori'][1:] * out['ori'][:-1], axis=1) > 0)
    ref = _run((qm, tm, cov, st))[0]
    assert np.allclose(out['ori'], ref['ori'], atol=1e-12) and not out['track_status'].any()
    with pytest.raises(AssertionError):
        TK.PoseTrackerHost(1, r=-1.0)
    with pytest.raises(AssertionError):
        TK.PoseTrackerHost(1, gate_chi2=float('nan'))
