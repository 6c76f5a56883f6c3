"""GPU: the multi-hypothesis orientation decode (csrc/k_modes.hip, ``spef_decode_modes``) against its NumPy twin
(spef_amd/spe/modes.py) on the device's own PDFs, the tracker's association step (``spef_track_step_modes``) against
``PoseTrackerHost.step_modes``, and the way up through Engine, SPEMi355x and Inference.

Shapes: B in {1, 3, 65}; orientation tables of 1728 and 1232 bins (the reference's), 257 (one bin past a 256-thread
stride) and 5 (fewer bins than threads, barely more than k_max); k_max in {1, 2, 4}; rounds in {0, 3}. Tolerances: an
output is float64 arithmetic rounded once to float32, so 2^-22 (float32 rounding with a 4x margin, the BLOCK_TOL of
tests/test_gpu_decode_cov.py) of 1 for a mass, of the block's largest entry for a theta block, and for a quaternion
component 2^-22 + 1e-12 l_1 / (l_1 - l_2): the eigenvector's sensitivity to a sum taken in another order. Rows whose
twin margin is below 1e-9 (a discrete decision at rounding distance from its threshold) are compared for status, n_modes
and finiteness only; the seeds below leave none."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from oracle import decode_ref as D
from spef_amd import _lib as L
from spef_amd.spe import modes as MD
from spef_amd.spe import track as TK

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import modes_inputs as MI  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 2.0 ** -22
ULP16 = 16 * 2.0 ** -23             # tests/test_gpu_track.py
MARGIN = 1e-9
CLS, REG = L.CLASSIFICATION, L.REGRESSION
KEYS = ('ori', 'pos', 'mahalanobis', 'track_status', 'cov', 'rates', 'chosen')


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items() if isinstance(v, torch.Tensor)}


def _rand_quats(n):
    h = np.random.Generator(np.random.PCG64(n)).standard_normal((n, 4))
    return h / np.linalg.norm(h, axis=1, keepdims=True)


@pytest.fixture(scope='module')
def tables(golden):
    return {1728: golden('decode_ori.npz')['hist'], 1232: D.orientation_histogram(12, True)[0], 257: _rand_quats(257),
            5: _rand_quats(5)}


@pytest.fixture(scope='module')
def engines(tables):
    from spef_amd.engine import Engine
    made = {}

    def get(n_ori):
        if n_ori not in made:
            e = Engine(None, 'cuda:0')
            e.set_decode_tables(tables[n_ori], None)
            made[n_ori] = e
        return made[n_ori]
    yield get
    for e in made.values():
        e.close()


def bump_logits(h, B, seed):
    """Row b: the log of a sum of 1 + b % 3 bumps exp(kappa (q_j . h_i)^2) of three widths with unequal weights around
    random directions (tests/test_gpu_decode_cov.py's ``logits``, with more than one bump), float32."""
    rng = np.random.Generator(np.random.PCG64(seed))
    kappas = (4.0, 30.0, 200.0) if len(h) > 100 else (1.0, 4.0, 12.0)      # a few bins: keep more than one in play
    lo = np.empty((B, len(h)))
    for b in range(B):
        nb = 1 + b % 3
        q0 = rng.standard_normal((nb, 4))
        q0 /= np.linalg.norm(q0, axis=1, keepdims=True)
        kappa = kappas[(b // 3) % 3]
        w = np.log(rng.uniform(0.5, 1.0, nb))
        lo[b] = np.logaddexp.reduce(kappa * (q0 @ h.T) ** 2 + w[:, None], axis=0)
    return lo.astype(np.float32)


def device_pdf(eng, lo):
    """The device's own softmax of the logits (spef_decode's ori_soft)."""
    B = lo.shape[0]
    dec = eng.decode(CLS, REG, torch.from_numpy(lo).cuda(), torch.zeros((B, 3), device='cuda'))
    return dec['ori_soft']


def assert_matches_twin(dev, pdf, bins, prm, tag):
    """``dev``: the device's outputs as NumPy; the twin runs on the same PDF rows. -> the number of rows compared by
    value."""
    twin = MD.decode_modes_host(pdf, bins, dtype=np.float64, **prm)
    assert np.array_equal(dev['modes_status'], twin['modes_status']), tag
    assert np.array_equal(dev['n_modes'], twin['n_modes']), (tag, dev['n_modes'], twin['n_modes'])
    for k in ('mode_quat', 'mode_mass', 'mode_cov'):
        assert np.array_equal(np.isnan(dev[k]), np.isnan(twin[k])), (tag, k)
        assert np.isfinite(dev[k][~np.isnan(twin[k])]).all(), (tag, k)
    skip = twin['margin'] < MARGIN
    assert skip.sum() <= 0.02 * len(skip), (tag, 'rows at rounding distance from a decision', np.flatnonzero(skip))
    worst = [0.0, 0.0, 0.0]
    for b in np.flatnonzero(~skip):
        for k in range(twin['n_modes'][b]):
            want, got = twin['mode_quat'][b, k], dev['mode_quat'][b, k].astype(np.float64)
            got = got if got @ want >= 0 else -got
            tol = TOL + 1e-12 / twin['eig_gap'][b, k]
            err = np.abs(got - want).max()
            worst[0] = max(worst[0], err / tol)
            assert err <= tol, (tag, b, k, err, tol)
            err = abs(float(dev['mode_mass'][b, k]) - twin['mode_mass'][b, k])
            worst[1] = max(worst[1], err)
            assert err <= TOL, (tag, b, k, err)
            want, got = twin['mode_cov'][b, k], dev['mode_cov'][b, k].astype(np.float64)
            assert np.array_equal(got, got.T), (tag, b, k)
            err = np.abs(got - want).max() / np.abs(want).max()
            worst[2] = max(worst[2], err)
            assert err <= TOL, (tag, b, k, err)
    print(f'{tag}: {int((~skip).sum())} rows; quaternion {worst[0]:.3f} of its bound, mass {worst[1]:.2e}, theta block '
          f'{worst[2]:.2e} of its largest entry (bound {TOL:.2e})')
    return int((~skip).sum())


# ---------------------------------------------------------------------------------------- kernel against twin
@pytest.mark.parametrize('n_ori', [1728, 1232, 257, 5])
@pytest.mark.parametrize('B', [1, 3, 65])
def test_kernel_matches_twin(engines, tables, n_ori, B):
    eng, h = engines(n_ori), tables[n_ori]
    pdf = device_pdf(eng, bump_logits(h, B, 100 * n_ori + B))
    host = pdf.cpu().numpy()
    for k_max in (1, 2, 4):
        for rounds in (0, 3):
            prm = dict(k_max=k_max, rounds=rounds, floor_var=1e-6)
            dev = _np(eng.decode_modes(pdf, **prm))
            assert dev['mode_quat'].shape == (B, k_max, 4) and dev['mode_cov'].shape == (B, k_max, 3, 3)
            assert not dev['modes_status'].any()
            n = assert_matches_twin(dev, host, h, prm, f'{n_ori} B={B} k_max={k_max} rounds={rounds}')
            assert n == B                                   # the seeds leave no row at rounding distance
            unit = np.linalg.norm(dev['mode_quat'].astype(np.float64), axis=2)
            live = ~np.isnan(unit)
            assert np.abs(unit[live] - 1).max() < 1e-6 and (dev['mode_quat'][..., 0][live] >= 0).all()
            assert (np.diff(dev['mode_mass'], axis=1)[live[:, 1:]] <= 0).all()
            if k_max == 1:                                  # one mode: the plain decode, mass exactly 1
                assert (dev['mode_mass'] == 1.0).all() and (dev['n_modes'] == 1).all()


def test_one_mode_is_decode_and_decode_cov(engines, tables):
    """k_max = 1 on the device: the quaternion is spef_decode's up to sign and float32 rounding, the theta block
    spef_decode_cov's."""
    eng, h = engines(1728), tables[1728]
    lo = torch.from_numpy(bump_logits(h, 9, 9)).cuda()
    dec = eng.decode(CLS, REG, lo, torch.zeros((9, 3), device='cuda'), want_cov=True)
    md = _np(eng.decode_modes(dec, k_max=1))
    assert 'mode_quat' in dec and dec['n_modes'].eq(1).all().item()
    q, q1 = dec['ori'].cpu().numpy().astype(np.float64), md['mode_quat'][:, 0].astype(np.float64)
    q1 *= np.sign((q * q1).sum(1))[:, None]
    assert np.abs(q - q1).max() <= 2.0 ** -23
    blk, want = md['mode_cov'][:, 0].astype(np.float64), dec['cov'].cpu().numpy()[:, :3, :3].astype(np.float64)
    assert np.abs(blk - want).max() <= TOL * np.abs(want).max()


def test_edge_rows(engines, tables):
    """A NaN, an infinity and an all-zero row: status 1, no mode, NaN outputs, the neighbours untouched. One-hot rows: one
    mode, that bin, the theta block the floor alone. A uniform row: finite, masses summing to 1."""
    eng, h = engines(1728), tables[1728]
    n = h.shape[0]
    good = device_pdf(eng, bump_logits(h, 8, 5)).cpu().numpy()
    pdf = good.copy()
    pdf[1, 7] = np.nan
    pdf[2, 1500] = np.inf
    pdf[3] = 0.0
    pdf[4] = 0.0
    pdf[4, 1000] = 0.25
    pdf[5] = 0.0
    pdf[5, 0] = 1.0
    pdf[6] = 1.0 / n
    prm = dict(k_max=4, floor_var=1e-4)
    dev = _np(eng.decode_modes(torch.from_numpy(pdf).cuda(), **prm))
    assert dev['modes_status'].tolist() == [0, 1, 1, 1, 0, 0, 0, 0]
    assert dev['n_modes'][1:4].tolist() == [0, 0, 0] and dev['n_modes'][4:6].tolist() == [1, 1]
    for k in ('mode_quat', 'mode_mass', 'mode_cov'):
        assert np.isnan(dev[k][1:4]).all(), k
    for b, j in ((4, 1000), (5, 0)):
        assert np.abs(dev['mode_quat'][b, 0] - MD.canonical(h[j]).astype(np.float32)).max() <= 2.0 ** -23
        assert dev['mode_mass'][b, 0] == 1.0
        # the floor alone, to the theta block's tolerance: the Markley average of one bin is that bin to float64
        # rounding, not bit for bit, which leaves entries of 1e-32
        assert np.abs(dev['mode_cov'][b, 0].astype(np.float64) - 1e-4 * np.eye(3)).max() <= TOL * 1e-4
    m = dev['n_modes'][6]
    assert np.isfinite(dev['mode_quat'][6, :m]).all() and abs(dev['mode_mass'][6, :m].astype(np.float64).sum() - 1) < 1e-6
    assert_matches_twin(dev, pdf, h, prm, 'edge rows')


def test_rows_do_not_depend_on_the_batch(engines, tables):
    """A row's outputs are bit-identical at B = 1 and inside B = 65."""
    eng, h = engines(1232), tables[1232]
    pdf = device_pdf(eng, bump_logits(h, 65, 123265))
    big = _np(eng.decode_modes(pdf, k_max=4))
    for b in (0, 1, 17, 64):
        one = _np(eng.decode_modes(pdf[b:b + 1].contiguous(), k_max=4))
        for k in big:
            assert np.array_equal(_bits(one[k][0]), _bits(big[k][b])), (b, k)


def test_decode_modes_argument_errors(engines, tables):
    """SPEF_ERR_ARG / SPEF_ERR_STATE with nothing enqueued."""
    from spef_amd.engine import Engine, _ptr, _stream
    eng = engines(257)
    lib, st = eng.lib, _stream(eng.device)
    pdf = device_pdf(eng, bump_logits(tables[257], 2, 1))
    mq, mm = torch.full((2, 2, 4), 7.0, device='cuda'), torch.full((2, 2), 7.0, device='cuda')
    mc = torch.full((2, 2, 9), 7.0, device='cuda')
    nm, ms = (torch.full((2,), 77, dtype=torch.int32, device='cuda') for _ in range(2))

    def params(**kw):
        p = dict(k_max=2, rounds=3, sep_deg=45.0, seed_rel=0.1, min_mass=0.05, floor_var=0.0)
        p.update(kw)
        return L.ModesParams(p['k_max'], p['rounds'], p['sep_deg'], p['seed_rel'], p['min_mass'], p['floor_var'])

    def call(ctx=eng.ctx, pdf=pdf, n=257, B=2, prm=params(), mq=mq, mm=mm, mc=mc, nm=nm, ms=ms):
        return lib.spef_decode_modes(ctx, _ptr(pdf), n, B, C.byref(prm) if prm is not None else None, _ptr(mq), _ptr(mm),
                                     _ptr(mc), _ptr(nm), _ptr(ms), st)
    for kw in (dict(ctx=None), dict(pdf=None), dict(prm=None), dict(mq=None), dict(mm=None), dict(mc=None), dict(nm=None),
               dict(ms=None), dict(B=0), dict(B=-1), dict(n=256), dict(n=1728)):
        assert call(**kw) == L.ERR_ARG, kw
    nan, inf = float('nan'), float('inf')
    for kw in (dict(k_max=0), dict(k_max=5), dict(rounds=-1), dict(rounds=9), dict(sep_deg=0.0), dict(sep_deg=180.5),
               dict(sep_deg=nan), dict(seed_rel=-0.1), dict(seed_rel=1.1), dict(seed_rel=inf), dict(min_mass=-0.1),
               dict(min_mass=0.51), dict(k_max=4, min_mass=0.26), dict(min_mass=nan), dict(floor_var=-1.0),
               dict(floor_var=inf)):
        assert call(prm=params(**kw)) == L.ERR_ARG, kw
    bare = Engine(None, 'cuda:0')                          # no orientation table
    try:
        assert call(ctx=bare.ctx) == L.ERR_STATE
    finally:
        bare.close()
    torch.cuda.synchronize()
    assert (mq == 7).all().item() and (mm == 7).all().item() and (mc == 7).all().item()
    assert (nm == 77).all().item() and (ms == 77).all().item()
    assert call(prm=params(sep_deg=180.0, min_mass=0.5)) == L.OK
    with pytest.raises(AssertionError):
        eng.decode_modes(pdf, k_max=5)


# ---------------------------------------------------------------------------------------- the tracker's association
N_STREAMS, N_T = 3, 40


@pytest.fixture(scope='module')
def track_eng():
    from spef_amd.engine import Engine
    e = Engine(None, 'cuda:0')
    yield e
    e.close()


@pytest.fixture(scope='module')
def track_inputs():
    """Three of the two-peak sequences as S = 3 streams, T = 40, time-major, with four candidates per row, rounded to the
    float32 the kernel reads: the twin's modes (one on the clean frames, then two) and two decoys (mode 0 turned 90 deg
    about body x with mass 0.15, the last mode turned 90 deg about body y with mass 0.1, each with its mode's theta block). On every third time step the four are
    rolled by two, so the modes sit in slots 2 and 3 (and K = 2 then sees the decoys alone: gating and restarts). A few
    rows carry a decode status, no candidates or a NaN first candidate."""
    tab = MI.tables()[1728]
    _, pdf = MI.two_peak_sequences(tab, seed=11, n_seq=N_STREAMS, n_frames=N_T)
    md = MD.decode_modes_host(pdf.transpose(1, 0, 2).reshape(N_T * N_STREAMS, -1), tab[0], k_max=4)
    B = N_T * N_STREAMS
    rng = np.random.Generator(np.random.PCG64(5))
    pos = (MI.POS + 0.01 * np.arange(N_T)[:, None, None] * [1.0, -0.5, 2.0] + rng.normal(0, 0.02, (N_T, N_STREAMS, 3)))
    cov = np.zeros((B, 6, 6), np.float32)
    cov[:, :3, :3] = np.nan                                  # never read: every candidate brings its own theta block
    cov[:, 3:, 3:] = (MI.POS_VAR * np.eye(3) + 1e-3).astype(np.float32)
    status = np.zeros(B, np.int32)
    q, m, c = md['mode_quat'].copy(), md['mode_mass'].copy(), md['mode_cov'].copy()
    r = np.sqrt(0.5)
    for b in range(B):
        last = md['n_modes'][b] - 1                          # the clean frames have one mode: slot 1 stays NaN, invalid
        q[b, 2], q[b, 3] = MI.qmul(q[b, 0], [r, r, 0, 0]), MI.qmul(q[b, last], [r, 0, r, 0])
        m[b, 2:], c[b, 2], c[b, 3] = (0.15, 0.1), c[b, 0], c[b, last]
        if (b // N_STREAMS) % 3 == 1:
            q[b], m[b], c[b] = np.roll(q[b], 2, axis=0), np.roll(m[b], 2), np.roll(c[b], 2, axis=0)
    n = np.full(B, 4, np.int32)
    status[3 * 10 + 1] = 1
    n[3 * 14 + 2] = 0
    q[3 * 20 + 0, 0] = np.nan
    return dict(mode_quat=q, mode_mass=m, mode_cov=c, n_modes=n,
                pos=pos.reshape(B, 3).astype(np.float32), cov=cov, status=status)


def _dec(d, K, rows=slice(None)):
    out = {k: torch.from_numpy(np.ascontiguousarray(v[rows])).cuda() for k, v in d.items()}
    for k in ('mode_quat', 'mode_mass', 'mode_cov'):
        out[k] = out[k][:, :K].contiguous()
    out['n_modes'] = out['n_modes'].clamp(max=K)
    return out


def _twin(d, K, pert=None):
    q, pos = d['mode_quat'][:, :K].astype(np.float64), d['pos'].astype(np.float64)
    if pert is not None:
        q, pos = q * (1 + 1e-9 * pert.choice([-1.0, 1.0], q.shape)), pos * (1 + 1e-9 * pert.choice([-1.0, 1.0], pos.shape))
    return TK.PoseTrackerHost(N_STREAMS, **MI.TRACK).step_modes(q, d['mode_mass'][:, :K], d['mode_cov'][:, :K],
                                                                np.minimum(d['n_modes'], K), pos, d['cov'], d['status'])


def test_one_candidate_is_track_step(track_eng, track_inputs):
    """K = 1: every output and the state equal spef_track_step's on the same quaternion and C_0, bit for bit."""
    d = _dec(track_inputs, 1)
    a, b = track_eng.tracker(N_STREAMS, **MI.TRACK), track_eng.tracker(N_STREAMS, **MI.TRACK)
    o1 = _np(a.step_modes(d, N_T, want_cov=True, want_rates=True))
    c0 = d['cov'].clone()
    c0[:, :3, :3] = d['mode_cov'][:, 0]
    quat = d['mode_quat'][:, 0].clone()
    quat[d['n_modes'] < 1] = float('nan')
    o2 = _np(b.step({'ori': quat.contiguous(), 'pos': d['pos'], 'cov': c0, 'status': d['status']}, N_T, want_cov=True,
                    want_rates=True))
    for k in o2:
        assert np.array_equal(_bits(o1[k]), _bits(o2[k])), k
    assert np.array_equal(_bits(a.state().cpu().numpy()), _bits(b.state().cpu().numpy()))
    bad = (d['n_modes'] < 1).cpu().numpy() | (d['status'] != 0).cpu().numpy() | np.isnan(o2['mahalanobis'])
    assert np.array_equal(o1['chosen'], np.where(bad, -1, 0))
    assert set(np.unique(o1['track_status'])) >= {0, 1}
    a.close()
    b.close()


@pytest.mark.parametrize('K', [2, 4])
def test_association_matches_twin(track_eng, track_inputs, K):
    """``chosen`` and the track status equal the twin's; every other output is within test_gpu_track.py's tolerance
    (ten times the twin's sensitivity to a 1e-9 relative perturbation of the measurements, never below 16 float32 ulps,
    relative to the output's largest magnitude). No row's cost gap is below 1e-9, so every stream is compared whole."""
    twin = _twin(track_inputs, K)
    pert = _twin(track_inputs, K, np.random.default_rng(0))
    assert twin['cost_gap'].min() > 1e-9
    trk = track_eng.tracker(N_STREAMS, **MI.TRACK)
    dev = _np(trk.step_modes(_dec(track_inputs, K), N_T, want_cov=True, want_rates=True))
    trk.close()
    assert np.array_equal(dev['chosen'], twin['chosen']) and np.array_equal(dev['track_status'], twin['track_status'])
    assert set(range(-1, K)) <= set(np.unique(twin['chosen'])) and set(np.unique(twin['track_status'])) >= {0, 1}
    for k in ('ori', 'pos', 'mahalanobis', 'cov', 'rates'):
        fin = np.isfinite(twin[k])
        assert np.array_equal(np.isfinite(dev[k]), fin), k
        mag = np.abs(twin[k][fin]).max()
        sens = np.abs(twin[k] - pert[k])[fin].max() / mag
        tol = max(10 * sens, ULP16)
        err = np.abs(dev[k].astype(np.float64) - twin[k])[fin].max() / mag
        print(f'K={K} {k}: sensitivity {sens:.2e}, tolerance {tol:.2e}, kernel against twin {err:.2e}')
        assert err <= tol, k


def test_cutting_a_sequence(track_eng, track_inputs):
    """T = 7 in one call and cut 3 + 4: bit-identical outputs and state."""
    S = N_STREAMS
    trk = track_eng.tracker(S, **MI.TRACK)
    whole = _np(trk.step_modes(_dec(track_inputs, 2, slice(0, 7 * S)), 7, want_cov=True, want_rates=True))
    state = trk.state().cpu().numpy()
    trk.reset()
    parts = [_np(trk.step_modes(_dec(track_inputs, 2, slice(a * S, b * S)), b - a, want_cov=True, want_rates=True))
             for a, b in ((0, 3), (3, 7))]
    for k in KEYS:
        assert np.array_equal(_bits(np.concatenate([p[k] for p in parts])), _bits(whole[k])), k
    assert np.array_equal(_bits(trk.state().cpu().numpy()), _bits(state))
    trk.close()


def test_track_step_modes_argument_errors(track_eng, track_inputs):
    from spef_amd.engine import _ptr, _stream
    lib, st = track_eng.lib, _stream(track_eng.device)
    trk = track_eng.tracker(N_STREAMS, **MI.TRACK)
    d = _dec(track_inputs, 2, slice(0, 6))
    qo, po = torch.full((6, 4), 7.0, device='cuda'), torch.full((6, 3), 7.0, device='cuda')
    ts, ch = (torch.full((6,), 77, dtype=torch.int32, device='cuda') for _ in range(2))

    def step(tr=trk.handle, mq=d['mode_quat'], mm=d['mode_mass'], mc=d['mode_cov'], nm=d['n_modes'], K=2, pos=d['pos'],
             cov=d['cov'], T=2, S=3, qo=qo, po=po, ts=ts, ch=ch):
        return lib.spef_track_step_modes(tr, _ptr(mq), _ptr(mm), _ptr(mc), _ptr(nm), K, _ptr(pos), _ptr(cov),
                                         _ptr(d['status']), T, S, _ptr(qo), _ptr(po), None, None, None, _ptr(ts),
                                         _ptr(ch), st)
    for kw in (dict(tr=None), dict(mq=None), dict(mm=None), dict(mc=None), dict(nm=None), dict(pos=None), dict(cov=None),
               dict(qo=None), dict(po=None), dict(ts=None), dict(ch=None), dict(K=0), dict(K=5), dict(S=2), dict(T=0)):
        assert step(**kw) == L.ERR_ARG, kw
    torch.cuda.synchronize()
    assert (qo == 7).all().item() and (po == 7).all().item() and (ts == 77).all().item() and (ch == 77).all().item()
    assert not trk.state().any().item()
    assert step() == L.OK
    torch.cuda.synchronize()
    assert (ch == 0).all().item() and trk.state()[:, 0].eq(1).all().item()
    trk.close()


# ---------------------------------------------------------------------------------------- end to end
def test_predict_tracked_with_modes(golden):
    """A head whose orientation logits are two-peaked -- planted by bias, as ``weights.plant_keypoint_head`` plants
    keypoints: log of 0.6 encode(q) + 0.4 encode(q flipped 180 deg about body z) -- through
    ``predict_tracked(modes=2)`` and ``Inference.tracker_modes``: the still pose carries 'modes' with both peaks, the
    tracked orientation follows the planted true peak, and the call equals decode -> decode_cov -> decode_modes ->
    step_modes at engine level bit for bit. modes = 0 returns today's keys; a
    head without an orientation PDF raises."""
    from spef_amd.arch import mobilenet_v2
    from spef_amd.inference import Inference
    from spef_amd.spe.keypoints import KeyPoints
    from spef_amd.spe.spe_utils import SPEUtils
    from spef_amd.weights import synthetic_state_dict
    g = golden('keypoints.npz')

    class Cam:
        K, nu, nv = g['K'], float(g['nu']), float(g['nv'])
    su = SPEUtils(Cam, 'classification', 12, 3, False, 'classification', keypoints_path=KeyPoints(Cam, g['kp3d']))
    tab = MI.tables()[1728]
    assert np.array_equal(tab[0], su.orientation.histogram)
    q_true = MI.rand_quat(np.random.Generator(np.random.PCG64(3)))
    q_flip = MI.qmul(q_true, MI.FLIP_Z)
    sd = synthetic_state_dict(mobilenet_v2('ursonet', su.orientation.n_bins, su.position.n_bins), seed=1001,
                              head_std=2e-4)
    sd['head.ori.1.bias'] = np.log(MI.mixture_pdf(q_true, q_flip, 0.6, tab).astype(np.float64) + 1e-12).astype(np.float32)
    x = torch.from_numpy(np.random.Generator(np.random.PCG64(31)).random((4, 3, 64, 64), dtype=np.float32))
    p = dict(q=MI.TRACK['q'], gate_chi2=MI.TRACK['gate_chi2'], max_coast=MI.TRACK['max_coast'])
    seq = Inference(sd, 'gpu_mi355x', su)
    try:
        spe = seq.inference_engine
        still, tracked, lat = spe.predict_tracked(x, 1, modes=2, **p)
        assert lat > 0 and set(tracked) == {'ori', 'pos', 'mahalanobis', 'track_status', 'chosen'}
        m = still['modes']
        assert set(m) == {'quat', 'mass', 'n', 'chosen'} and m['quat'].shape == (4, 2, 4)
        assert m['n'].tolist() == [2] * 4 and m['chosen'].tolist() == [0] * 4 and not tracked['track_status'].any()
        for t in range(4):
            assert MI.angle_deg(m['quat'][t, 0], q_true) < 8 and MI.angle_deg(m['quat'][t, 1], q_flip) < 8
            assert abs(m['mass'][t, 0] - 0.6) < 0.02 and abs(m['mass'][t, 1] - 0.4) < 0.02
            assert MI.angle_deg(tracked['ori'][t], q_true) < 8           # the planted true peak
        eng = spe.engine
        dec = eng.decode(CLS, CLS, *eng.forward(x.cuda()), want_cov=True, fixed_var=(100.0, 100.0))
        eng.decode_modes(dec, k_max=2)
        trk = eng.tracker(1, **p)
        want = _np(trk.step_modes(dec, 4))
        trk.close()
        for k in tracked:
            assert np.array_equal(_bits(tracked[k]), _bits(want[k])), k
        assert np.array_equal(_bits(m['quat']), _bits(dec['mode_quat'].cpu().numpy()))
        spe.tracker(1, **p).reset()
        still0, tracked0, _ = spe.predict_tracked(x, 1, **p)            # modes = 0: today's path and keys
        assert 'modes' not in still0 and set(tracked0) == {'ori', 'pos', 'mahalanobis', 'track_status'}
        with pytest.raises(AssertionError):
            spe.predict_tracked(x, 1, modes=5, **p)
        mode = spe.ori_mode
        spe.ori_mode = REG                                               # no orientation PDF: refused before any launch
        try:
            with pytest.raises(AssertionError):
                spe.predict_tracked(x, 1, modes=2, **p)
        finally:
            spe.ori_mode = mode
        # Inference forwards tracker_modes
        seq.reset()
        seq.tracker_params, seq.tracker_modes = p, 2
        run = seq.predict_sequence(x, 'Tracker')
        assert len(run) == 4
        for t, (s1, _, v1) in enumerate(run):
            assert s1['modes']['quat'].shape == (2, 4) and s1['modes']['n'] == 2 and v1['chosen'] == 0
            assert MI.angle_deg(v1['ori'], q_true) < 8
    finally:
        seq.close()
