"""GPU: the pose smoother (csrc/k_smooth.hip: spef_track_history, spef_track_step_hist, spef_track_history_push,
spef_track_smooth) on the cases of tests/smooth_cases.py against its NumPy twin and the independent textbook pass; the
recording step against spef_track_step bit for bit; windows, stream counts and the argument checks; and the smoothed
poses of SPEMi355x.predict_tracked(smooth=True) / Inference.predict_sequence(..., 'Smoother').

tests/test_smooth_host.py holds the twin to the textbook pass, to a batch solution and to what the theorem guarantees,
and measures what three planted errors move."""
import os
import sys

import numpy as np
import pytest
import torch

from spef_amd import _lib as L
from spef_amd import blob as Bl
from spef_amd.arch import mobilenet_v2
from spef_amd.spe import smooth as SM
from spef_amd.spe import track as TK
from spef_amd.weights import synthetic_state_dict

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smooth_cases as SC  # noqa: E402
import track_cases as TC  # noqa: E402
import track_inputs as TI  # noqa: E402

pytestmark = pytest.mark.gpu

N = TI.N
FILT = TC.KEYS + ('track_status',)
SMOOTH = SC.KEYS + ('smooth_status',)


@pytest.fixture(scope='module')
def eng():
    from spef_amd.engine import Engine
    e = Engine(None, 'cuda:0')
    yield e
    e.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _stack(cases, rows=slice(None), src=None):
    """The cases side by side as the streams of one tracker (stream i = case src[i]) -> the decode dict of time-major
    device rows, T."""
    src = np.arange(len(cases)) if src is None else src

    def rows_of(field):
        x = np.stack([getattr(c, field)[rows] for c in cases], axis=1)[:, src]
        return torch.from_numpy(np.ascontiguousarray(x.reshape((-1,) + x.shape[2:]))).cuda()
    d = {'ori': rows_of('quat'), 'pos': rows_of('pos'), 'status': rows_of('status')}
    if cases[0].cov is not None:
        d['cov'] = rows_of('cov')
    return d, d['ori'].shape[0] // len(src)


def _split(out, S, i):
    return {k: v.reshape((-1, S) + v.shape[1:])[:, i] for k, v in out.items()}


def _run(eng, cases, src=None, want_cov=True):
    """One tracker over the stacked cases, recorded -> (filter outputs, state, history rows [T x S x 160], smoother
    outputs), NumPy."""
    d, T = _stack(cases, src=src)
    S = d['ori'].shape[0] // T
    trk = eng.tracker(S, **cases[0].params)
    h = trk.history(T)
    out = trk.step(d, T, want_cov=True, want_rates=True, history=h)
    sm = h.smooth(out, want_cov=want_cov, want_rates=True)
    res = _np(out), trk.state().cpu().numpy(), h.rows().cpu().numpy(), _np(sm)
    h.close()
    trk.close()
    return res


@pytest.fixture(scope='module')
def dev(eng):
    """{case: (filter outputs of its stream, smoother outputs of its stream)}: one recorded launch and one smoothing
    per group of tests/smooth_cases.py. A group that holds bad_pivot is smoothed from a second history, built by
    set_state + push from the first one's rows with that case's row spoiled."""
    res = {}
    for names in SC.GROUPS:
        cases = [SC.base(n) for n in names]
        S = len(names)
        d, T = _stack(cases)
        trk = eng.tracker(S, **cases[0].params)
        h = trk.history(T)
        out = trk.step(d, T, want_cov=True, want_rates=True, history=h)
        if 'bad_pivot' in names:
            rows = h.rows().cpu().numpy()
            i = names.index('bad_pivot')
            rows[:, i:i + 1] = SC.spoil('bad_pivot', rows[:, i:i + 1].copy())
            ts = out['track_status'].reshape(T, S)
            h.reset()
            for f in range(T):
                trk.set_state(rows[f])
                h.push(ts[f].contiguous())
            assert np.array_equal(_bits(h.rows().cpu().numpy()), _bits(rows))
        sm = _np(h.smooth(out, want_cov=True, want_rates=True))
        out = _np(out)
        h.close()
        trk.close()
        for i, n in enumerate(names):
            res[n] = (_split(out, S, i), _split(sm, S, i))
    return res


@pytest.mark.parametrize('name', SC.NAMES)
def test_kernel_matches_twin_and_textbook(dev, name):
    """smooth_status equals the twin's and the textbook pass's; every other output of the rows that have a track is
    within max(10 x the twin's sensitivity to a 1e-9 perturbation of the measurements, 16 float32 ulps) of the output's
    largest magnitude of both, and finite exactly where the reference rounded to float32 is. Rows without a track come
    back as the filter returned them bit for bit, with NaN in cov and rates; the smoothed quaternion stays in the
    hemisphere of the filter's; cov is symmetric bit for bit; a segment end is the filter's row bit for bit."""
    r, c = SC.reference(name), SC.base(name)
    filt, got = dev[name]
    assert np.array_equal(got['smooth_status'], r.twin['smooth_status'])
    assert np.array_equal(got['smooth_status'], r.text['smooth_status'])
    m = SC.smoothed(r.twin)
    for k in SC.KEYS:
        b = r.bounds[k]
        for label, ref in (('twin', r.twin), ('textbook', r.text)):
            err, same = TC.error(got[k][m], ref[k][m], b, cast=True)
            unit = 'absolute bound' if b.absolute is not None else f'tolerance {b.tol:.2e}'
            print(f'{name} {k}: kernel against {label} {err:.2e} of the {unit}')
            assert same and err <= 1.0, (name, k, label)
    assert np.array_equal(_bits(got['ori'][~m]), _bits(c.quat[~m]))
    assert np.array_equal(_bits(got['pos'][~m]), _bits(c.pos[~m]))
    assert np.isnan(got['cov'][~m]).all() and np.isnan(got['rates'][~m]).all()
    for k in SC.KEYS:
        assert np.isfinite(got[k][m]).all(), k
    assert np.all(np.sum(got['ori'][m].astype(np.float64) * filt['ori'][m], axis=1) > 0)
    assert np.array_equal(_bits(got['cov'][m]), _bits(got['cov'][m].transpose(0, 2, 1)))
    ends = (got['smooth_status'] & SM.SEGMENT_END) != 0
    for k in ('ori', 'pos', 'rates'):
        assert np.array_equal(_bits(got[k][ends]), _bits(filt[k][ends])), k
    if name != 'bad_pivot':          # whose recorded P is not the filter's
        assert np.array_equal(_bits(got['cov'][ends]), _bits(filt['cov'][ends]))
    if name == 'bad_rows':
        assert (~m).sum() == 2


def _three(eng, T_parts=(N,), history=True, push=False):
    """three_streams() through one tracker in calls of T_parts frames -> (outputs, state, history rows or None)."""
    quat, pos, cov, status = TI.three_streams()
    d = {'ori': torch.from_numpy(quat.astype(np.float32)).cuda(), 'pos': torch.from_numpy(pos.astype(np.float32)).cuda(),
         'cov': torch.from_numpy(cov.astype(np.float32)).cuda(), 'status': torch.from_numpy(status.astype(np.int32)).cuda()}
    trk = eng.tracker(3, **TI.PARAMS)
    h = trk.history(N) if history else None
    parts, at = [], 0
    for T in T_parts:
        rows = slice(3 * at, 3 * (at + T))
        o = trk.step({k: v[rows] for k, v in d.items()}, T, want_cov=True, want_rates=True,
                     history=None if push else h)
        if push:
            assert T == 1
            h.push(o['track_status'])
        parts.append(_np(o))
        at += T
    out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    state = trk.state().cpu().numpy()
    rows = None
    if history:
        assert h.count == N and int(h.device_count().item()) == N
        rows = h.rows().cpu().numpy()
        h.close()
    trk.close()
    return out, state, rows


@pytest.fixture(scope='module')
def three(eng):
    return _three(eng)


def test_step_hist_equals_step(eng, three):
    """spef_track_step_hist against spef_track_step on three_streams(): every output and the final fp64 state are equal
    bit for bit; the last history row is that state with the track status in slot 2."""
    out, state, rows = three
    want, want_state, _ = _three(eng, history=False)
    for k in FILT:
        assert np.array_equal(_bits(out[k]), _bits(want[k])), k
    assert np.array_equal(_bits(state), _bits(want_state))
    last = rows[-1].copy()
    assert np.array_equal(last[:, 2], out['track_status'][-3:].astype(np.float64))
    last[:, 2] = 0.0
    assert np.array_equal(_bits(last), _bits(state))
    assert np.array_equal(rows[:, :, 2].reshape(-1), out['track_status'].astype(np.float64))
    assert set(out['track_status'].tolist()) >= {0, 1, 2, 6}


def test_recording_in_pieces_and_by_push(eng, three):
    """5 + 59 frames recorded equal one call of 64 bit for bit, history rows included; push after each of 64 T = 1
    steps gives step_hist's rows bit for bit."""
    out, state, rows = three
    for parts, push in (((5, 59), False), ((1,) * N, True)):
        o, s, r = _three(eng, parts, push=push)
        for k in FILT:
            assert np.array_equal(_bits(o[k]), _bits(out[k])), (k, push)
        assert np.array_equal(_bits(s), _bits(state)) and np.array_equal(_bits(r), _bits(rows)), push


def test_sub_window(eng):
    """first = 10, T = 30 of a recorded 64 equals the twin run on that window (under the rule of the whole case), and
    the window's last row is the filter's."""
    names = SC.GROUPS[0][:3]
    cases = [SC.base(n) for n in names]
    d, T = _stack(cases)
    trk = eng.tracker(3, **cases[0].params)
    h = trk.history(T)
    out = trk.step(d, T, history=h)
    win = {k: out[k][3 * 10:3 * 40] for k in ('ori', 'pos')}
    got = _np(h.smooth(win, first=10, T=30, want_cov=True, want_rates=True))
    filt = _np(win)
    h.close()
    trk.close()
    for i, n in enumerate(names):
        r = SC.reference(n)
        twin = SM.PoseSmootherHost(**cases[i].params).smooth(r.hist, r.filt['ori'][10:40], r.filt['pos'][10:40],
                                                             first=10, T=30)
        g = _split(got, 3, i)
        assert np.array_equal(g['smooth_status'], twin['smooth_status']) and g['smooth_status'][-1] == SM.SEGMENT_END
        for k in SC.KEYS:
            err, same = TC.error(g[k], twin[k], r.bounds[k], cast=True)
            assert same and err <= 1.0, (n, k)
        assert np.array_equal(_bits(g['ori'][-1]), _bits(_split(filt, 3, i)['ori'][-1]))


def test_stream_counts_and_no_cov(eng):
    """The ten streams of the first tracker case group: at S = 3 and at S = 65 (the ten tiled, more than one wave's
    worth of streams) every copy equals its original at S = 10 bit for bit, filter, history and smoother. Without
    cov_out, 'ori', 'pos' and 'rates' are the same bit for bit."""
    names = TC.GROUPS[0]
    cases = [TC.case(n) for n in names]
    out, state, rows, sm = _run(eng, cases)
    for src in (np.arange(3), np.arange(65) % len(names)):
        o, s, r, m = _run(eng, cases, src=src)
        S = len(src)
        for k in FILT:
            assert np.array_equal(_bits(o[k].reshape((N, S) + o[k].shape[1:])),
                                  _bits(out[k].reshape((N, len(names)) + out[k].shape[1:])[:, src])), (S, k)
        assert np.array_equal(_bits(s), _bits(state[src])) and np.array_equal(_bits(r), _bits(rows[:, src])), S
        for k in SMOOTH:
            assert np.array_equal(_bits(m[k].reshape((N, S) + m[k].shape[1:])),
                                  _bits(sm[k].reshape((N, len(names)) + sm[k].shape[1:])[:, src])), (S, k)
    _, _, _, plain = _run(eng, cases, want_cov=False)
    assert 'cov' not in plain
    for k in ('ori', 'pos', 'rates', 'smooth_status'):
        assert np.array_equal(_bits(plain[k]), _bits(sm[k])), k


def test_argument_errors(eng):
    """A capacity too large, first + T beyond the count, a history of a tracker with another S, more frames than the
    capacity and a NULL required pointer: each returns SPEF_ERR_ARG and writes nothing."""
    import ctypes as C
    from spef_amd.engine import _ptr, _stream
    lib, st = eng.lib, _stream(eng.device)
    cases = [TC.case(n) for n in ('h3', 'h4', 'h5')]
    d, _ = _stack(cases, slice(0, 8))
    trk, other = eng.tracker(3, **TI.PARAMS), eng.tracker(2, **TI.PARAMS)
    try:
        hp = C.c_void_p()
        assert (2 ** 31 - 1) * 3 * 36 > 2 ** 31 - 1
        assert lib.spef_track_history_create(trk.handle, 2 ** 31 - 1, C.byref(hp)) == L.ERR_ARG
        assert lib.spef_track_history_create(trk.handle, (2 ** 31 - 1) // (3 * 36) + 1, C.byref(hp)) == L.ERR_ARG
        assert lib.spef_track_history_create(trk.handle, 0, C.byref(hp)) == L.ERR_ARG and not hp.value
        h, h2 = trk.history(8), other.history(8)
        qo, po = torch.full((24, 4), 7.0, device='cuda'), torch.full((24, 3), 7.0, device='cuda')
        ts = torch.full((24,), 77, dtype=torch.int32, device='cuda')
        extra = [torch.full(s, 7.0, device='cuda') for s in ((24,), (24, 6, 6), (24, 6))]

        def step(hist, T, S, quat=d['ori']):
            return lib.spef_track_step_hist(trk.handle, hist.handle, _ptr(quat), _ptr(d['pos']), _ptr(d['cov']),
                                            _ptr(d['status']), T, S, _ptr(qo), _ptr(po), _ptr(extra[0]), _ptr(extra[1]),
                                            _ptr(extra[2]), _ptr(ts), st)
        assert step(h2, 8, 3) == L.ERR_ARG          # the history of a tracker with S = 2
        assert step(h, 8, 2) == L.ERR_ARG           # S is not the tracker's
        assert step(h, 9, 3) == L.ERR_ARG           # more frames than the capacity
        assert step(h, 8, 3, quat=None) == L.ERR_ARG
        assert lib.spef_track_history_push(h2.handle, trk.handle, _ptr(ts), st) == L.ERR_ARG
        assert lib.spef_track_history_push(h.handle, trk.handle, None, st) == L.ERR_ARG
        torch.cuda.synchronize()
        assert all((x == 7).all().item() for x in [qo, po] + extra) and (ts == 77).all().item()
        assert not trk.state().any().item() and h.count == 0 and int(h.device_count().item()) == 0

        five = {k: v[:15] for k, v in d.items()}     # five of the eight frames
        out = trk.step(five, 5, history=h)
        assert step(h, 4, 3) == L.ERR_ARG           # 5 + 4 > 8
        ss = torch.full((24,), 77, dtype=torch.int32, device='cuda')

        def smooth(first, T, quat=qo, status=ss):
            return lib.spef_track_smooth(h.handle, first, T, _ptr(quat), _ptr(po), _ptr(extra[1]), _ptr(extra[2]),
                                         _ptr(status), st)
        assert smooth(0, 6) == L.ERR_ARG and smooth(3, 3) == L.ERR_ARG and smooth(-1, 2) == L.ERR_ARG
        assert smooth(0, 0) == L.ERR_ARG and smooth(0, 5, quat=None) == L.ERR_ARG
        assert smooth(0, 5, status=None) == L.ERR_ARG
        assert lib.spef_track_history_get(h.handle, 0, 6, _ptr(extra[1]), st) == L.ERR_ARG
        torch.cuda.synchronize()
        assert all((x == 7).all().item() for x in [qo, po] + extra) and (ss == 77).all().item()
        got = h.smooth(out)                          # and the accepted call still works
        assert got['smooth_status'].reshape(5, 3)[-1].tolist() == [2, 2, 2]
        h.close()
        h2.close()
    finally:
        trk.close()
        other.close()


def test_predict_tracked_and_predict_sequence(golden):
    """predict_tracked(smooth=True) (64 x 64 frames, T = 4, S = 2) returns the keys of smooth=False and
    'smooth_status'; its last time step equals smooth=False bit for bit, 'mahalanobis' and 'track_status' are the
    filter's, and the smoothed rows equal PoseHistory.smooth called by hand on the same decode. With modes=2 it records
    through push and gives the same kind of result. predict_sequence(x, 'Smoother') returns T triples whose pose_video
    carries 'smooth_status', the last frame being the tracker's; predict(x, 'Smoother') raises ValueError."""
    from spef_amd.inference import Inference
    from spef_amd.spe.spe_utils import SPEUtils
    from spef_amd.spe.keypoints import KeyPoints
    from spef_amd.spe_mi355x import SPEMi355x
    g = golden('keypoints.npz')

    class Cam:
        K, nu, nv = g['K'], float(g['nu']), float(g['nv'])
    su = SPEUtils(Cam, 'classification', 12, 3, False, 'classification', keypoints_path=KeyPoints(Cam, g['kp3d']))
    sd = synthetic_state_dict(mobilenet_v2('ursonet', su.orientation.n_bins, su.position.n_bins), seed=1001)
    x = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).random((8, 3, 64, 64), dtype=np.float32))
    p = dict(gate_chi2=16.81, r=(9.0, 4.0))
    spe = SPEMi355x(Bl.pack(sd, dtype='fp16'), 'cuda:0', su)
    try:
        still0, plain, _ = spe.predict_tracked(x, n_streams=2, pdf_cov=True, floor_var=(1e-4, 1e-2), **p)
        spe.tracker(2, **p).reset()
        still, got, lat = spe.predict_tracked(x, n_streams=2, pdf_cov=True, floor_var=(1e-4, 1e-2), smooth=True, **p)
        assert lat > 0 and set(got) == set(plain) | {'smooth_status'} and set(still) == set(still0)
        assert got['ori'].shape == (8, 4) and got['pos'].shape == (8, 3) and got['smooth_status'].shape == (8,)
        for k in ('mahalanobis', 'track_status'):
            assert np.array_equal(_bits(got[k]), _bits(plain[k])), k
        ss = got['smooth_status']
        assert ss[6:].tolist() == [2, 2] and set(ss.tolist()) <= {0, 2} and (ss == 0).any()
        for k in ('ori', 'pos'):
            assert np.array_equal(_bits(got[k][ss == 2]), _bits(plain[k][ss == 2])), k
            assert (_bits(got[k][ss == 0]) != _bits(plain[k][ss == 0])).any(), k
        eng = spe.engine
        dec = eng.decode(L.CLASSIFICATION, L.CLASSIFICATION, *eng.forward(x.cuda()), want_cov=True, fixed_var=(9.0, 4.0),
                         floor_var=(1e-4, 1e-2))
        trk = eng.tracker(2, **p)
        h = trk.history(4)
        want = _np(h.smooth(trk.step(dec, 4, history=h)))
        h.close()
        trk.close()
        for k in ('ori', 'pos', 'smooth_status'):
            assert np.array_equal(_bits(got[k]), _bits(want[k])), k

        spe.tracker(1, **p).reset()
        _, m_plain, _ = spe.predict_tracked(x, 1, modes=2, **p)
        spe.tracker(1, **p).reset()
        _, m_got, _ = spe.predict_tracked(x, 1, modes=2, smooth=True, **p)
        assert set(m_got) == set(m_plain) | {'smooth_status'}
        for k in ('mahalanobis', 'track_status', 'chosen'):
            assert np.array_equal(_bits(m_got[k]), _bits(m_plain[k])), k
        assert m_got['smooth_status'][-1] == 2 and np.array_equal(_bits(m_got['ori'][-1]), _bits(m_plain['ori'][-1]))
    finally:
        spe.close()

    seq = Inference(sd, 'gpu_mi355x', su)
    try:
        tracked = seq.predict_sequence(x[:5], 'Tracker')
        seq.reset()
        run = seq.predict_sequence(x[:5], 'Smoother')
        assert len(run) == 5
        for t, ((s1, lat, v1), (s0, _, v0)) in enumerate(zip(run, tracked)):
            assert lat > 0 and set(s1) == set(s0) and set(v1) == set(v0) | {'smooth_status'}
            assert v1['smooth_status'] == (2 if t == 4 else 0)
            assert v1['track_status'] == v0['track_status']
        assert np.array_equal(_bits(run[4][2]['ori']), _bits(tracked[4][2]['ori']))
        assert np.array_equal(_bits(run[4][2]['pos']), _bits(tracked[4][2]['pos']))
        assert not np.array_equal(_bits(run[0][2]['pos']), _bits(tracked[0][2]['pos']))
        with pytest.raises(ValueError):
            seq.predict(x[:1], 'Smoother')
    finally:
        seq.close()
