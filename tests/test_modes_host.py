"""The NumPy twin of the multi-hypothesis orientation decode (spef_amd/spe/modes.py) and of its association in the pose
tracker (``PoseTrackerHost.step_modes``): against the reference's own encode / decode (oracle/decode_ref.py) on unimodal
PDFs and on mixtures of two orientations, on edge rows, and on the two-peak video sequences that motivate it."""
import os
import sys

import numpy as np
import pytest

from oracle import decode_ref as D
from spef_amd.spe import decode_cov as DC
from spef_amd.spe import modes as MD
from spef_amd.spe import track as TK

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import modes_inputs as MI  # noqa: E402

# The twin's worst figures on the 500 mixtures of MI.mixture_cases() (the same on both tables, whose non-zero bins are
# the same): a mode is at most 0.4887 deg further from its orientation than the plain decode of that orientation's own
# PDF is, and its mass at most 0.009472 off the mixing weight. The bounds are twice that.
EXCESS_MEASURED_DEG, MASS_MEASURED = 0.4887, 0.009472
EXCESS_BOUND_DEG, MASS_BOUND = 2 * EXCESS_MEASURED_DEG, 2 * MASS_MEASURED


@pytest.fixture(scope='module')
def tabs():
    return MI.tables()


def _align(q, ref):
    return q if q @ ref >= 0 else -q


@pytest.mark.parametrize('n', [1728, 1232])
def test_unimodal_is_the_plain_decode(tabs, n):
    """200 random orientations encoded with smooth 3: one mode, equal to the reference's decode to float32 rounding of
    the components (the eigenvector's sign is arbitrary there), mass exactly 1, the theta block ``decode_cov``'s to
    1e-12 of its largest entry."""
    tab = tabs[n]
    h = tab[0]
    rng = np.random.Generator(np.random.PCG64(n))
    worst = 0.0
    for _ in range(200):
        p = MI.encode(MI.rand_quat(rng), tab)
        q, m, blk, st, _ = MD.decode_modes_row(p, h, k_max=4)
        assert st == 0 and len(m) == 1 and m[0] == 1.0
        ref = D.decode_orientation(p, h)
        got = _align(q[0], ref).astype(np.float32)
        assert np.all(np.abs(got - ref) <= np.spacing(np.maximum(np.abs(ref), np.float32(2.0 ** -24))))
        assert q[0][0] >= 0 and abs(q[0] @ q[0] - 1.0) < 1e-14
        want, ok = DC.theta_block(p, q[0], h)
        assert ok
        err = np.abs(blk[0] - want).max() / np.abs(want).max()
        worst = max(worst, err)
        assert err <= 1e-12
        out = MD.decode_modes_host(p[None], h, k_max=4)
        assert out['mode_quat'].dtype == np.float32 and out['n_modes'][0] == 1 and np.isnan(out['mode_quat'][0, 1:]).all()
        assert np.isnan(out['mode_mass'][0, 1:]).all() and np.isnan(out['mode_cov'][0, 1:]).all()
    print(f'{n}: largest theta block difference {worst:.2e} of its largest entry')


@pytest.mark.parametrize('n', [1728, 1232])
def test_mixtures_give_both_orientations(tabs, n):
    """500 mixtures of two orientations at least 60 deg apart, the first with weight in [0.55, 0.7], default
    parameters, k_max = 4: exactly two modes in weight order, every one of the 500. A mode's angular error may exceed
    that of the plain decode of its orientation's own unimodal PDF by EXCESS_BOUND_DEG = 2 x 0.4887 deg (the twin's
    worst excess on these cases), its mass may differ from the mixing weight by MASS_BOUND = 2 x 0.009472."""
    tab = tabs[n]
    h = tab[0]
    excess, mass_err, margin = 0.0, 0.0, np.inf
    for qa, qb, w in MI.mixture_cases():
        q, m, _, st, mg = MD.decode_modes_row(MI.mixture_pdf(qa, qb, w, tab), h, k_max=4)
        assert st == 0 and len(m) == 2 and m[0] > m[1]
        margin = min(margin, mg)
        for k, (qt, wt) in enumerate(((qa, w), (qb, 1.0 - w))):
            plain = D.decode_orientation(MI.encode(qt, tab), h)
            ex = MI.angle_deg(q[k], qt) - MI.angle_deg(plain, qt)
            excess, mass_err = max(excess, ex), max(mass_err, abs(m[k] - wt))
            assert ex <= EXCESS_BOUND_DEG and abs(m[k] - wt) <= MASS_BOUND
    print(f'{n}: worst excess {excess:.4f} deg (bound {EXCESS_BOUND_DEG:.4f}), worst mass error {mass_err:.6f} (bound '
          f'{MASS_BOUND:.6f}), smallest margin {margin:.2e}')


def test_edge_rows(tabs):
    tab = tabs[1728]
    h = tab[0]
    # a NaN in p, an infinity, all zero: status 1, no mode, NaN outputs
    good = MI.encode(np.array([1.0, 0, 0, 0]), tab)
    for bad in (np.where(np.arange(h.shape[0]) == 7, np.nan, good), np.where(np.arange(h.shape[0]) == 7, np.inf, good),
                np.zeros(h.shape[0])):
        out = MD.decode_modes_host(bad[None].astype(np.float32), h, k_max=2)
        assert out['modes_status'][0] == MD.INVALID and out['n_modes'][0] == 0
        assert np.isnan(out['mode_quat']).all() and np.isnan(out['mode_mass']).all() and np.isnan(out['mode_cov']).all()
    # one-hot: that bin, mass 1, the theta block is the floor alone
    for j in (0, 5, 1000):
        p = np.zeros(h.shape[0], np.float32)
        p[j] = 0.25
        q, m, blk, st, _ = MD.decode_modes_row(p, h, k_max=4, floor_var=1e-4)
        assert st == 0 and len(m) == 1 and m[0] == 1.0
        assert np.abs(q[0] - MD.canonical(h[j])).max() < 1e-15
        assert np.abs(blk[0] - 1e-4 * np.eye(3)).max() < 1e-15
    # uniform: finite, status 0, the masses sum to 1
    out = MD.decode_modes_host(np.full((1, h.shape[0]), 1.0 / h.shape[0], np.float32), h, k_max=4, dtype=np.float64)
    n = out['n_modes'][0]
    assert out['modes_status'][0] == 0 and 1 <= n <= 4
    assert np.isfinite(out['mode_quat'][0, :n]).all() and np.isfinite(out['mode_cov'][0, :n]).all()
    assert abs(out['mode_mass'][0, :n].sum() - 1.0) < 1e-12 and np.all(np.diff(out['mode_mass'][0, :n]) <= 0)
    # k_max = 1 is the plain decode even of a mixture
    qa, qb, w = MI.mixture_cases(1)[0]
    p = MI.mixture_pdf(qa, qb, w, tab)
    q, m, blk, st, _ = MD.decode_modes_row(p, h, k_max=1)
    ref = D.decode_orientation(p, h)
    assert len(m) == 1 and m[0] == 1.0 and np.abs(_align(q[0], ref) - ref).max() < 2.0 ** -23
    assert np.abs(blk[0] - DC.theta_block(p, q[0], h)[0]).max() <= 1e-12 * np.abs(blk[0]).max()
    # rounds = 0: the seeds' clusters as they are, still both orientations (a grid step or so coarser)
    q, m, _, st, _ = MD.decode_modes_row(p, h, k_max=4, rounds=0)
    assert st == 0 and len(m) == 2 and MI.angle_deg(q[0], qa) < 15 and MI.angle_deg(q[1], qb) < 15
    assert abs(m.sum() - 1.0) < 1e-12


def test_parameter_validation():
    h = np.eye(4)
    p = np.float32([0.4, 0.3, 0.2, 0.1])
    for kw in (dict(k_max=0), dict(k_max=5), dict(sep_deg=0.0), dict(sep_deg=181.0), dict(sep_deg=np.nan),
               dict(seed_rel=-0.1), dict(seed_rel=1.5), dict(min_mass=-1e-3), dict(k_max=4, min_mass=0.3),
               dict(min_mass=np.inf), dict(rounds=-1), dict(rounds=9), dict(floor_var=-1.0), dict(floor_var=np.nan)):
        with pytest.raises(AssertionError):
            MD.decode_modes_row(p, h, **kw)
    with pytest.raises(AssertionError):
        MD.decode_modes_row(p[:3], h)
    assert MD.decode_modes_row(p, h, k_max=2, min_mass=0.5)[3] == 0


@pytest.fixture(scope='module')
def sequences(tabs):
    """The two-peak sequences decoded once: per sequence the truth, the modes, the plain decode and the covariances."""
    tab = tabs[1728]
    h = tab[0]
    qs, pdf = MI.two_peak_sequences(tab)
    T = qs.shape[1]
    pos = np.tile(MI.POS, (T, 1))
    cov = np.zeros((T, 6, 6))
    cov[:, 3:, 3:] = MI.POS_VAR * np.eye(3)
    out = []
    for s in range(qs.shape[0]):
        md = MD.decode_modes_host(pdf[s], h, k_max=2, dtype=np.float64)
        plain = np.stack([D.decode_orientation(p, h) for p in pdf[s]]).astype(np.float64)
        cov_plain = cov.copy()
        for t in range(T):
            cov_plain[t, :3, :3] = DC.theta_block(pdf[s, t], plain[t], h)[0]
        out.append(dict(truth=qs[s], md=md, plain=plain, cov_plain=cov_plain, pos=pos, cov=cov))
    return out


def _errors(out, truth):
    return np.array([MI.angle_deg(q, t) for q, t in zip(out['ori'], truth)])


def test_association_resolves_the_two_peak_sequences(sequences):
    """20 sequences of 40 frames whose PDF holds the true orientation and its 180 deg flip about body z with weights in
    [0.3, 0.7]: the tracker fed every mode and choosing by likelihood is never more than 10 deg off; fed the plain
    decode it is off on more than half the frames; fed the heaviest mode alone it is off more often than never."""
    err = {'plain': [], 'heaviest': [], 'associated': []}
    for sq in sequences:
        md = sq['md']
        heavy_cov = sq['cov'].copy()
        heavy_cov[:, :3, :3] = md['mode_cov'][:, 0]
        err['plain'].append(_errors(TK.PoseTrackerHost(1, **MI.TRACK).step(sq['plain'], sq['pos'], sq['cov_plain']),
                                    sq['truth']))
        err['heaviest'].append(_errors(TK.PoseTrackerHost(1, **MI.TRACK).step(md['mode_quat'][:, 0], sq['pos'],
                                                                              heavy_cov), sq['truth']))
        o = TK.PoseTrackerHost(1, **MI.TRACK).step_modes(md['mode_quat'], md['mode_mass'], md['mode_cov'],
                                                         md['n_modes'], sq['pos'], sq['cov'])
        err['associated'].append(_errors(o, sq['truth']))
    err = {k: np.concatenate(v) for k, v in err.items()}
    for k, e in err.items():
        print(f'{k}: median {np.median(e):.2f} deg, max {e.max():.2f} deg, off by more than 10 deg {100 * (e > 10).mean():.1f} %')
    off = {k: (e > 10).mean() for k, e in err.items()}
    assert off['associated'] == 0.0
    assert off['plain'] > 0.5
    assert off['heaviest'] > 0.0
    assert np.median(err['associated']) < np.median(err['heaviest']) < np.median(err['plain'])


def test_step_modes_matches_the_textbook_filter(sequences):
    """An independent restatement (tests/modes_inputs.py: np.linalg.inv, slogdet, an explicit Gaussian log-likelihood):
    the chosen indices and the track status agree exactly, the poses to 1e-9."""
    worst = 0.0
    for sq in sequences:
        md = sq['md']
        o = TK.PoseTrackerHost(1, **MI.TRACK).step_modes(md['mode_quat'], md['mode_mass'], md['mode_cov'],
                                                         md['n_modes'], sq['pos'], sq['cov'])
        assert o['cost_gap'].min() > 1e-6                    # no choice hangs on rounding
        tb = MI.TextbookTracker(**MI.TRACK)
        for t in range(len(sq['pos'])):
            n = md['n_modes'][t]
            cands = [(md['mode_quat'][t, k], md['mode_mass'][t, k], md['mode_cov'][t, k]) for k in range(n)]
            q, p, k, ts = tb.step(cands, sq['pos'][t], sq['cov'][t])
            assert k == o['chosen'][t] and ts == o['track_status'][t], t
            worst = max(worst, np.abs(q - o['ori'][t]).max(), np.abs(p - o['pos'][t]).max())
    print(f'largest pose difference {worst:.2e}')
    assert worst <= 1e-9


def test_step_modes_with_one_candidate_is_step(sequences):
    """K = 1: bit-identical to ``step`` fed the same quaternion and C_0, in every output and in the state; invalid
    candidates (a NaN quaternion, a zero mass, n_modes = 0, a decode status) coast or pass through as ``step`` does."""
    sq = sequences[3]
    md = sq['md']
    T = len(sq['pos'])
    q, m, c = md['mode_quat'][:, :1].copy(), md['mode_mass'][:, :1].copy(), md['mode_cov'][:, :1].copy()
    n = np.ones(T, np.int32)
    status = np.zeros(T, np.int32)
    q[5] = np.nan
    m[9] = 0.0
    n[12] = 0
    status[15] = 1
    C0 = sq['cov'].copy()
    C0[:, :3, :3] = c[:, 0]
    qs = q[:, 0].copy()
    qs[[9, 12]] = np.nan                                      # what an invalid candidate is to ``step``
    for first_bad in (False, True):
        a, b = TK.PoseTrackerHost(1, **MI.TRACK), TK.PoseTrackerHost(1, **MI.TRACK)
        rows = slice(5, T) if first_bad else slice(0, T)      # from row 5 on: no track yet, the row passes through
        o1 = a.step_modes(q[rows], m[rows], c[rows], n[rows], sq['pos'][rows], sq['cov'][rows], status[rows])
        o2 = b.step(qs[rows], sq['pos'][rows], C0[rows], status[rows])
        for k in ('ori', 'pos', 'mahalanobis', 'track_status', 'cov', 'rates'):
            assert np.array_equal(o1[k], o2[k], equal_nan=True), k
        assert np.array_equal(a.state(), b.state())
        want = np.where(np.isin(np.arange(T), [5, 9, 12, 15]), -1, 0)[rows]
        assert np.array_equal(o1['chosen'], want)
        assert set(np.unique(o1['track_status'])) >= {0, 1}
