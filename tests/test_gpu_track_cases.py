"""GPU: the pose tracker kernel (csrc/k_track.hip) on the cases of tests/track_cases.py -- full, correlated, badly
scaled and asymmetric covariances, a fast rotation, either sign and any length of the measured quaternion, a still
target, a 3 rad innovation, the fixed r, cov_scale, every status word, the bad rows of the host tests, 2,048 frames --
against its NumPy twin and against the independent textbook filter, and at the largest S the interface accepts.

tests/test_track_cases_host.py holds the twin to the textbook filter on the same cases, shows that the cases reach the
branches they are meant to, and measures what four planted errors move."""
import os
import sys

import numpy as np
import pytest
import torch

from spef_amd import _lib as L
from spef_amd.spe import track as TK

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu

OUT = TC.KEYS + ('track_status',)
MAX_STREAMS = 65536            # the largest n_streams spef_track_create accepts


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


def _group(names):
    cases = [TC.case(n) for n in names]
    prm = [repr(TK.check_params(**c.params)) for c in cases]
    assert len(set(prm)) == 1 and len({c.cov is None for c in cases}) == 1 and len({len(c.quat) for c in cases}) == 1
    return cases


def _split(out, S, i):
    return {k: v.reshape((-1, S) + v.shape[1:])[:, i] for k, v in out.items()}


@pytest.fixture(scope='module')
def dev(eng):
    """{case: (outputs of its stream, its state row afterwards)}: one launch per group of tests/track_cases.py."""
    res = {}
    for names in TC.GROUPS:
        cases = _group(names)
        d, T = _stack(cases)
        trk = eng.tracker(len(names), **cases[0].params)
        out = _np(trk.step(d, T, want_cov=True, want_rates=True))
        state = trk.state().cpu().numpy()
        trk.close()
        for i, n in enumerate(names):
            res[n] = (_split(out, len(names), i), state[i])
    return res


@pytest.mark.parametrize('name', TC.NAMES)
def test_kernel_matches_twin_and_textbook(dev, name):
    """track_status equals the twin's and the textbook filter's; every other output of the tracked rows is within the
    rule of test_kernel_matches_twin (tests/test_gpu_track.py) of both -- max(10 x the twin's sensitivity to a 1e-9
    perturbation, 16 float32 ulps) of the output's largest magnitude, absolute where the twin's output is identically
    zero -- and finite exactly where the reference rounded to float32 is. Rows that passed through come back bit for
    bit, with NaN in d2, cov and the rates."""
    r, c = TC.reference(name), TC.case(name)
    got, _ = dev[name]
    assert np.array_equal(got['track_status'], r.twin['track_status'])
    assert np.array_equal(got['track_status'], r.text['track_status'])
    m = TC.tracked(r.twin)
    for k in TC.KEYS:
        b = r.bounds[k]
        for label, ref in (('twin', r.twin), ('textbook', r.text)):
            err, same = TC.error(got[k][m], ref[k][m], b, cast=True)
            unit = 'absolute bound' if b.absolute is not None else f'tolerance {b.tol:.2e}'
            print(f'{name} {k}: kernel against {label} {err:.2e} of the {unit}')
            assert same and err <= 1.0, (name, k, label)
    assert np.array_equal(_bits(got['ori'][~m]), _bits(c.quat[~m]))
    assert np.array_equal(_bits(got['pos'][~m]), _bits(c.pos[~m]))
    for k in ('mahalanobis', 'cov', 'rates'):
        assert np.isnan(got[k][~m]).all(), k
    if name == 'bad_rows':
        assert (~m).sum() == 2


def test_final_state_in_fp64(dev):
    """The outputs are float32, so their comparison cannot see below 6e-8 what the kernel's rcp_nr / rsq_nr (hardware
    estimates plus Newton steps) do where the twin divides and takes square roots. The state row after the last frame
    is fp64: have and the coast count equal the twin's, and q, t, (w, v) and the 12 x 12 P are within the bounds of
    'ori', 'pos', 'rates' and 'cov' of their largest magnitude. Measured: 9.7e-14 at the most (the rates after the
    2,048 frames of long), 1.5e-14 or less after 64 frames (rates of correlated), 4.7e-15 on badly_scaled, whose S is
    the worst conditioned."""
    for name in TC.NAMES:
        r, (_, st) = TC.reference(name), dev[name]
        assert np.array_equal(st[:3], r.state[:3]), name
        line = []
        for key, part in (('ori', slice(3, 7)), ('pos', slice(7, 10)), ('rates', slice(10, 16)), ('cov', slice(16, 160))):
            b, want = r.bounds[key], r.state[part]
            assert np.isfinite(st[part]).all()
            d = np.abs(st[part] - want)
            if b.absolute is not None:
                err, allow = (d / b.absolute).max(), 1.0
            else:
                err, allow = d.max() / np.abs(want).max(), b.tol
            line.append(f'{key} {err:.1e}')
            assert err <= allow, (name, key)
        print(f'{name}: fp64 state against the twin, relative to the largest entry: ' + ', '.join(line))


def test_signs_of_the_quaternion(dev):
    """Measurements of either sign give the same track bit for bit (double_cover = H3, outputs and state), and in
    no case does the output quaternion change hemisphere between consecutive tracked frames."""
    (a, sa), (b, sb) = dev['double_cover'], dev['h3']
    for k in OUT:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert np.array_equal(_bits(sa), _bits(sb))
    for n in TC.NAMES:
        o = dev[n][0]['ori'][TC.tracked(dev[n][0])].astype(np.float64)
        assert np.all(np.sum(o[1:] * o[:-1], axis=1) > 0), n
    w = dev['fast_rotation'][0]['ori'][:, 0]
    assert int((np.diff(np.sign(w)) != 0).sum()) >= 3


def test_long_run(eng, dev):
    """2,048 frames of one stream: the 6 x 6 cov output is symmetric bit for bit on every frame, the final 12 x 12 P
    is symmetric bit for bit with no eigenvalue below -16 float32 ulps of its largest entry, and 1,000 + 1,048 frames
    in two calls change nothing, bit for bit, in outputs or state."""
    out, state = dev['long']
    assert np.array_equal(_bits(out['cov']), _bits(out['cov'].transpose(0, 2, 1)))
    P = state[16:].reshape(12, 12)
    assert state[0] == 1 and np.array_equal(_bits(P), _bits(P.T))
    low = np.linalg.eigvalsh(P).min()
    print(f'smallest eigenvalue of P after {TC.LONG_T} frames: {low:.3e}, largest entry {np.abs(P).max():.3e}')
    assert low >= -TC.ULP16 * np.abs(P).max()
    cases = _group(('long',))
    trk = eng.tracker(1, **cases[0].params)
    parts = []
    for rows in (slice(0, 1000), slice(1000, TC.LONG_T)):
        d, T = _stack(cases, rows)
        parts.append(_np(trk.step(d, T, want_cov=True, want_rates=True)))
    for k in OUT:
        assert np.array_equal(_bits(np.concatenate([p[k] for p in parts])), _bits(out[k])), k
    assert np.array_equal(_bits(trk.state().cpu().numpy()[0]), _bits(state))
    trk.close()


def test_largest_stream_count(eng):
    """S = 65,536, the most spef_track_create accepts. A step of T = 911 (T * S * 36 > 2^31 - 1) returns SPEF_ERR_ARG
    and writes nothing; no accepted call of that size is made. At T = 2, with the ten streams of the first case group
    tiled across the tracker, every copy equals its original bit for bit in outputs and in state."""
    from spef_amd.engine import _ptr, _stream
    names = TC.GROUPS[0]
    cases = _group(names)
    small, T = _stack(cases, slice(0, 2))
    ref_trk = eng.tracker(len(names), **cases[0].params)
    want = _np(ref_trk.step(small, T, want_cov=True, want_rates=True))
    want_state = ref_trk.state().cpu().numpy()
    ref_trk.close()

    trk = eng.tracker(MAX_STREAMS, **cases[0].params)
    try:
        assert 911 * MAX_STREAMS * 36 > 2 ** 31 - 1 >= 910 * MAX_STREAMS * 36
        qo, po = torch.full((20, 4), 7.0, device='cuda'), torch.full((20, 3), 7.0, device='cuda')
        ts = torch.full((20,), 77, dtype=torch.int32, device='cuda')
        extra = [torch.full(s, 7.0, device='cuda') for s in ((20,), (20, 6, 6), (20, 6))]
        assert eng.lib.spef_track_step(trk.handle, _ptr(small['ori']), _ptr(small['pos']), _ptr(small['cov']),
                                       _ptr(small['status']), 911, MAX_STREAMS, _ptr(qo), _ptr(po), _ptr(extra[0]),
                                       _ptr(extra[1]), _ptr(extra[2]), _ptr(ts), _stream(eng.device)) == L.ERR_ARG
        torch.cuda.synchronize()
        assert all((x == 7).all().item() for x in [qo, po] + extra) and (ts == 77).all().item()
        assert not trk.state().any().item()

        src = np.arange(MAX_STREAMS) % len(names)
        wide, T = _stack(cases, slice(0, 2), src)
        got = _np(trk.step(wide, T, want_cov=True, want_rates=True))
        state = trk.state().cpu().numpy()
        for k in OUT:
            g = got[k].reshape((T, MAX_STREAMS) + got[k].shape[1:])
            w = want[k].reshape((T, len(names)) + want[k].shape[1:])[:, src]
            assert np.array_equal(_bits(g), _bits(w)), k
        assert np.array_equal(_bits(state), _bits(want_state[src]))
        assert state[:, 0].all() and not got['track_status'].any()
    finally:
        trk.close()
