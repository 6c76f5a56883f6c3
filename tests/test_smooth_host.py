"""CPU: the pose smoother's NumPy twin (spef_amd/spe/smooth.py) against an independent textbook RTS pass, against a batch
solution that has no recursion in it, and against what the smoothing theorem guarantees; what three planted errors
move; and that the cases of tests/smooth_cases.py reach the branches they are meant to."""
import os
import sys

import numpy as np
import pytest

from spef_amd.spe import smooth as SM
from spef_amd.spe import track as TK

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smooth_cases as SC  # noqa: E402
import track_cases as TC  # noqa: E402
import track_inputs as TI  # noqa: E402

TEN = tuple(n for n in SC.NAMES if n != 'bad_pivot')      # the cases the tracker itself produced


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize('name', SC.NAMES)
def test_twin_matches_textbook(name):
    """smooth_status equal on every row; every other output of the rows that have a track within max(10 x the twin's
    sensitivity to a 1e-9 relative perturbation of the measurements, 16 float32 ulps) of the output's largest
    magnitude, and finite in the same places."""
    r = SC.reference(name)
    assert np.array_equal(r.twin['smooth_status'], r.text['smooth_status'])
    m = SC.smoothed(r.twin)
    for k in SC.KEYS:
        err, same = TC.error(r.twin[k][m], r.text[k][m], r.bounds[k])
        print(f'{name} {k}: twin against textbook {err:.2e} of the tolerance {r.bounds[k].tol:.2e}')
        assert same and err <= 1.0, (name, k)
    assert np.isnan(r.twin['cov'][~m]).all() and np.isnan(r.twin['rates'][~m]).all()
    assert np.array_equal(_bits(r.twin['ori'][~m]), _bits(r.filt['ori'][~m]))
    assert np.array_equal(_bits(r.twin['pos'][~m]), _bits(r.filt['pos'][~m]))


def test_positions_equal_the_batch_solution():
    """Independent of the recursion: block-diagonal cov, no gate, so the (t, v) sub-filter is linear. The twin's
    smoothed positions of H3 cut to 16 frames equal the dense solution over all 16 frames at once (96 unknowns),
    under the rule (the bound from the twin's own sensitivity on these 16 frames)."""
    c = TC.case('h3')
    n = SC.BATCH_FRAMES
    prm = TC.NO_GATE
    rows = slice(0, n)

    def run(q, p):
        filt, hist = SM.record(TK.PoseTrackerHost(1, **prm), q[rows], p[rows], c.cov[rows], c.status[rows])
        assert not filt['track_status'].any()
        return SM.PoseSmootherHost(**prm).smooth(hist, filt['ori'], filt['pos'])
    twin, pert = run(c.quat, c.pos), run(*TC.perturbed(c))
    b = SC.bound(c, twin, pert, 'pos')
    want = SC.batch_positions(prm, c.pos[rows], c.cov[rows])
    err, same = TC.error(twin['pos'], want, b)
    print(f'smoothed positions against the batch solution: {err:.2e} of the tolerance {b.tol:.2e}')
    assert same and err <= 1.0
    filt_err = np.abs(SM.record(TK.PoseTrackerHost(1, **prm), c.quat[rows], c.pos[rows], c.cov[rows],
                                c.status[rows])[0]['pos'] - want).max()
    assert filt_err > 1e3 * b.tol * b.mag          # the filter's own positions are nowhere near it


@pytest.mark.parametrize('name', SC.NAMES)
def test_what_the_theorem_guarantees(name):
    """The last row of every segment is the filter's bit for bit; P^s is symmetric bit for bit; on every smoothed row
    no eigenvalue of P - P^s is below -16 float32 ulps of max|P|."""
    r = SC.reference(name)
    st, hist = r.twin['smooth_status'], r.hist[:, 0]
    ends = (st & SM.SEGMENT_END) != 0
    assert ends[-1] or st[-1] == SM.NO_TRACK
    assert np.array_equal(_bits(r.twin['ori'][ends]), _bits(r.filt['ori'][ends]))
    assert np.array_equal(_bits(r.twin['pos'][ends]), _bits(r.filt['pos'][ends]))
    assert np.array_equal(_bits(r.twin['cov'][ends]), _bits(hist[ends, 16:].reshape(-1, 12, 12)[:, :6, :6]))
    m = SC.smoothed(r.twin)
    assert np.array_equal(_bits(r.twin['cov'][m]), _bits(r.twin['cov'][m].transpose(0, 2, 1)))
    # the full 12 x 12 P^s is not an output: run the pass again and keep it
    worst = 0.0
    sm = SM.PoseSmootherHost(**SC.base(name).params)
    Ps = None
    for k in range(len(st) - 1, -1, -1):
        if st[k] == SM.NO_TRACK:
            continue
        P = hist[k, 16:].reshape(12, 12)
        if st[k] == SM.SMOOTHED:
            G, Pm, _, _, ok = sm.gain(hist[k])
            assert ok
            Pn = P + G @ (Ps - Pm) @ G.T
            assert np.allclose(Pn[:6, :6], r.twin['cov'][k], rtol=1e-9, atol=1e-12 * np.abs(P).max())
            if name != 'bad_pivot':          # whose planted P is not a covariance
                low = np.linalg.eigvalsh(P - 0.5 * (Pn + Pn.T)).min() / np.abs(P).max()
                worst = min(worst, low)
            Ps = Pn
        else:
            Ps = P
    print(f'{name}: smallest eigenvalue of P - P^s relative to max|P|: {worst:.2e}')
    assert worst >= -TC.ULP16


def test_one_frame_returns_the_filter():
    c = TC.case('h3')
    filt, hist = SM.record(TK.PoseTrackerHost(1, **c.params), c.quat[:7], c.pos[:7], c.cov[:7], c.status[:7])
    out = SM.PoseSmootherHost(**c.params).smooth(hist, filt['ori'][3:4], filt['pos'][3:4], first=3, T=1)
    assert out['smooth_status'].tolist() == [SM.SEGMENT_END]
    assert np.array_equal(_bits(out['ori']), _bits(filt['ori'][3:4]))
    assert np.array_equal(_bits(out['pos']), _bits(filt['pos'][3:4]))
    assert np.array_equal(_bits(out['cov']), _bits(filt['cov'][3:4]))
    assert np.array_equal(_bits(out['rates']), _bits(filt['rates'][3:4]))


@pytest.mark.parametrize('name', ('h3', 'h4'))
def test_smoothing_lowers_the_error(name):
    """What makes it worth having. A precondition on the inputs: the textbook smoother's RMS orientation and position
    errors against the true trajectory are strictly below the textbook filter's. Then the twin's must be too."""
    r = SC.reference(name)
    tf, ts = SC.rms_errors(r.text_filt), SC.rms_errors(r.text)
    assert ts[0] < tf[0] and ts[1] < tf[1], 'precondition: the textbook pass does not improve on its filter'
    f, s = SC.rms_errors(r.filt), SC.rms_errors(r.twin)
    print(f'{name}: RMS orientation {f[0]:.2e} -> {s[0]:.2e} rad, position {f[1]:.2e} -> {s[1]:.2e} m')
    assert s[0] < f[0] and s[1] < f[1]


@pytest.mark.parametrize('variant,name,key', (('no_transition', 'h3', 'pos'),
                                              ('error_against_posterior', 'fast_rotation', 'ori'),
                                              ('sign_flipped', 'h3', 'cov')))
def test_planted_errors_are_far_above_the_tolerance(variant, name, key):
    """F^T dropped from P F^T, e formed against x_k instead of x-_{k+1}, P^s_{k+1} - P- with the sign flipped: each,
    planted in the textbook pass, moves the named output of the named case by more than 100 tolerances."""
    r, c = SC.reference(name), SC.base(name)
    bad, _ = SC.textbook_rts(c.params, r.text_hist, r.text_filt['ori'], r.text_filt['pos'], variant=variant)
    m = SC.smoothed(r.twin)
    err, _ = TC.error(bad[key][m], r.twin[key][m], r.bounds[key])
    print(f'{variant} on {name}: moves {key} by {err:.2e} tolerances')
    assert err > 100.0


def test_cases_reach_their_branches():
    """From the textbook's diagnostics: every smooth_status occurs; a re-initialisation splits a chain (cov_scale, h5:
    the row before a row with track_status & 4 is a segment end, and rows on both sides are smoothed); a coasted
    stretch does not (long_invalid, h4); no tolerance exceeds 1e-4; and the ten cases the tracker produced have a
    well-conditioned P- everywhere."""
    seen = set()
    for name in SC.NAMES:
        r = SC.reference(name)
        seen |= set(r.text['smooth_status'].tolist())
        for k in SC.KEYS:
            assert r.bounds[k].tol <= 1e-4, (name, k)
    assert seen == {0, 1, 2, 2 | 4}
    for name in ('cov_scale', 'h5'):
        r = SC.reference(name)
        ts, st = r.text_filt['track_status'], r.text['smooth_status']
        re = np.flatnonzero(ts & TK.REINIT)
        assert re.size >= 1 and (re > 1).all()
        for k in re:
            assert st[k - 1] == SM.SEGMENT_END and st[k - 2] == SM.SMOOTHED and st[k] == SM.SMOOTHED
    for name in ('long_invalid', 'h4'):
        r = SC.reference(name)
        coasted = (r.text_filt['track_status'] & TK.INVALID) != 0
        assert coasted.sum() >= 6 and (r.text['smooth_status'][coasted] == SM.SMOOTHED).all()
    for name in TEN:
        d = SC.reference(name).diag
        assert np.nanmin(d['pivot']) > 1e-6 and np.nanmax(d['cond']) < 1e9, name
    assert SC.reference('bad_pivot').text['smooth_status'][SC.BAD_PIVOT_ROW] == (SM.SEGMENT_END | SM.BAD_PIVOT)
    assert SC.reference('bad_rows').text['smooth_status'][:2].tolist() == [SM.NO_TRACK, SM.NO_TRACK]
