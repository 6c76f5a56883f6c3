"""The batched video path on the GPU (csrc/k_video.hip, spef_video_* in include/spef.h, Engine.video_filter,
SPEMi355x.predict_video, Inference.predict_sequence, StreamPipeline.submit(video=...)): the adaptive PDF filter, the
decode of the filtered PDFs and the pole rule, against the reference fixture, the host twin
(spef_amd.temporal.filter_sequences), the decode oracle and the per-frame Inference.predict loop.

Tolerances: PDFs rtol 1e-5 (atol 1e-12) and distances rtol 1e-5 for l2 / kl / js / hellinger / tv -- a NumPy
emulation of the kernel's arithmetic (float32 elementwise, float64 sums) is within 2.6e-6 / 1.2e-7 of the fixture,
which leaves ~4x for expf / logf / sqrtf differences; rtol 1e-4 for wasserstein, where the fixture's own float32
cumsum puts that emulation 3.6e-5 / 2.9e-5 away. Decode: 1e-3 degrees and 1e-4, as tests/test_gpu_inference.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import decode_ref as D
from spef_amd import temporal as TP

pytestmark = pytest.mark.gpu

ORI = dict(n=0.8, alpha=16.49)       # the Inference engine's filters (inference.py:38-39)
POS = dict(n=0.5, alpha=48.64)


def _rtol(metric):
    return 1e-4 if metric == 'wasserstein' else 1e-5


# ---------------------------------------------------------------------------------------- shared, read-only
@pytest.fixture(scope='module')
def tables():
    return {1728: D.orientation_histogram(12, False)[0], 1232: D.orientation_histogram(12, True)[0],
            27: D.orientation_histogram(3, False)[0], 'pos1000': D.position_histogram(10),
            'pos27': D.position_histogram(3)}


@pytest.fixture(scope='module')
def engines(tables):
    """Weightless contexts with decode tables: (n_ori, n_pos) -> Engine."""
    from spef_amd.engine import Engine
    made = {}

    def get(n_ori, n_pos):
        if (n_ori, n_pos) not in made:
            e = Engine(None, 'cuda:0')
            e.set_decode_tables(tables[n_ori], tables[f'pos{n_pos}'])
            made[(n_ori, n_pos)] = e
        return made[(n_ori, n_pos)]
    yield get
    for e in made.values():
        e.close()


def _step(vf, ori, pos, still=None, want_filtered=True):
    """One VideoFilter.step on PDFs [T, S, n] given directly (no network) -> NumPy dict (+ 'still')."""
    T, S = ori.shape[:2]
    q = np.tile(np.array([1, 0, 0, 0], np.float32), (T * S, 1)) if still is None else still.reshape(T * S, 4)
    dec = {'ori_soft': torch.from_numpy(np.ascontiguousarray(ori.reshape(T * S, -1))).cuda(),
           'pos_soft': torch.from_numpy(np.ascontiguousarray(pos.reshape(T * S, -1))).cuda(),
           'ori': torch.from_numpy(np.ascontiguousarray(q)).cuda()}
    out = vf.step(dec, T, want_filtered=want_filtered)
    torch.cuda.synchronize()
    res = {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}
    res['still'] = dec['ori'].cpu().numpy()
    return res


def _peaks(T, S, n, speed, seed=0):
    """Unnormalised peaked PDFs [T, S, n]: a Gaussian bump on a small floor whose centre drifts `speed` widths per
    step, a different start and speed per stream."""
    i = np.arange(n, dtype=np.float64)
    sigma = max(1.2, 0.02 * n)
    x = np.empty((T, S, n), np.float32)
    for s in range(S):
        c0, v = n * (0.3 + 0.1 * s), speed * sigma * (1.0 + 0.1 * s)
        for t in range(T):
            x[t, s] = ((np.exp(-0.5 * ((i - c0 - v * t) / sigma) ** 2) + 1e-5) * (1.0 + 0.1 * t + 0.3 * s))
    return x


def _weights(x, cfg, metric):
    _, d, _ = TP.filter_sequences(x, cfg['n'], cfg['alpha'], metric)
    return np.exp(-np.float32(cfg['alpha']) * d[1:])


def _moving(T, S, n, cfg, metric):
    """_peaks at the drift speed that puts the smallest blend weight at 0.3 (bisection on the host twin); the test
    then checks that every weight lies in [0.2, 0.9]: the filter really blends."""
    lo, hi = 1e-4, 3.0
    for _ in range(30):
        mid = np.sqrt(lo * hi)
        if _weights(_peaks(T, S, n, mid), cfg, metric).min() > 0.3:
            lo = mid
        else:
            hi = mid
    x = _peaks(T, S, n, lo)
    w = _weights(x, cfg, metric)
    assert w.min() >= 0.2 and w.max() <= 0.9, (metric, n, w.min(), w.max())
    return x


# ---------------------------------------------------------------------------------------- 1. golden
@pytest.mark.parametrize('metric', TP.METRICS)
def test_video_filter_matches_reference_fixture(golden, engines, metric):
    g = golden('temporal_pdf.npz')
    seq = np.ascontiguousarray(g['seq'][:, None, :].astype(np.float32))           # T = 6, S = 1, n = 1728
    pos_in = _peaks(seq.shape[0], 1, 1000, 0.1)
    eng = engines(1728, 1000)
    for cfg, tag in ((ORI, 'ori'), (POS, 'pos')):       # both settings through the orientation head
        vf = eng.video_filter(1, metric, n_ori=cfg['n'], alpha_ori=cfg['alpha'])
        out = _step(vf, seq, pos_in)
        vf.close()
        pe = np.abs(out['ori_soft'] / g[f'{metric}_{tag}_pdf'] - 1).max()
        print(f'{metric} {tag}: max rel pdf {pe:.3e}, dist {out["ori_distance"]} vs {g[f"{metric}_{tag}_dist"]}')
        np.testing.assert_allclose(out['ori_soft'], g[f'{metric}_{tag}_pdf'], rtol=_rtol(metric), atol=1e-12)
        np.testing.assert_allclose(out['ori_distance'], g[f'{metric}_{tag}_dist'], rtol=_rtol(metric))
        assert not out['status'].any()


# ---------------------------------------------------------------------------------------- 2. host twin
@pytest.mark.parametrize('metric', TP.METRICS)
@pytest.mark.parametrize('n_ori,n_pos', [(1728, 1000), (1232, 1000), (27, 27)])
def test_video_filter_matches_host_twin(engines, metric, n_ori, n_pos):
    T, S = 5, 3
    xo, xp = _moving(T, S, n_ori, ORI, metric), _moving(T, S, n_pos, POS, metric)
    wo, do, _ = TP.filter_sequences(xo, ORI['n'], ORI['alpha'], metric)
    wp, dp, _ = TP.filter_sequences(xp, POS['n'], POS['alpha'], metric)
    eng = engines(n_ori, n_pos)
    vf = eng.video_filter(S, metric)
    out = _step(vf, xo, xp)
    r = _rtol(metric)
    for name, got, want in (('ori pdf', out['ori_soft'], wo.reshape(T * S, -1)), ('pos pdf', out['pos_soft'],
                            wp.reshape(T * S, -1)), ('ori dist', out['ori_distance'], do.reshape(-1)),
                            ('pos dist', out['pos_distance'], dp.reshape(-1))):
        print(f'{metric} n={n_ori}/{n_pos} {name}: max rel {np.abs((got - want) / np.where(want == 0, 1, want)).max():.3e}')
        np.testing.assert_allclose(got, want, rtol=r, atol=1e-12 if 'pdf' in name else 0, err_msg=name)
    assert not out['status'].any()
    # streams do not leak into each other: permuting them permutes every output, bit for bit
    perm = [2, 0, 1]
    vf.reset()
    out2 = _step(vf, np.ascontiguousarray(xo[:, perm]), np.ascontiguousarray(xp[:, perm]))
    vf.close()
    for k in ('ori_soft', 'pos_soft', 'ori_distance', 'pos_distance', 'ori', 'pos', 'status'):
        a = out[k].reshape((T, S) + out[k].shape[1:])[:, perm]
        np.testing.assert_array_equal(out2[k].reshape(a.shape), a, err_msg=k)


# ---------------------------------------------------------------------------------------- 3. state
@pytest.mark.parametrize('metric', ['l2', 'wasserstein'])
def test_video_state_split_and_reset(engines, metric):
    T, S = 6, 3
    xo, xp = _moving(T, S, 1728, ORI, metric), _moving(T, S, 1000, POS, metric)
    eng = engines(1728, 1000)
    vf = eng.video_filter(S, metric)
    one = _step(vf, xo, xp)
    vf.reset()
    a, b = _step(vf, xo[:2], xp[:2]), _step(vf, xo[2:], xp[2:])
    for k in ('ori_soft', 'pos_soft', 'ori_distance', 'pos_distance', 'ori', 'pos', 'status'):
        np.testing.assert_array_equal(np.concatenate([a[k], b[k]]), one[k], err_msg=k)
    # without the filtered PDFs (the library's own chunk buffers): the same poses and distances
    vf.reset()
    lean = _step(vf, xo, xp, want_filtered=False)
    assert lean['ori_soft'] is None and lean['pos_soft'] is None
    for k in ('ori_distance', 'pos_distance', 'ori', 'pos', 'status'):
        np.testing.assert_array_equal(lean[k], one[k], err_msg=k)
    # reset(stream=1): only stream 1's next frame passes through with distance 0
    vf.reset(stream=1)
    nxt = _step(vf, xo[:1], xp[:1])
    assert nxt['ori_distance'][1] == 0 and nxt['pos_distance'][1] == 0
    assert (nxt['ori_distance'][[0, 2]] > 0).all() and (nxt['pos_distance'][[0, 2]] > 0).all()
    np.testing.assert_array_equal(nxt['ori_soft'][1], one['ori_soft'][1])      # = the normalised frame itself
    assert not np.array_equal(nxt['ori_soft'][0], one['ori_soft'][0])
    vf.close()


def test_video_set_state_continues_a_sequence(engines):
    """spef_video_set_state: a second filter loaded with the state after two steps continues like the first."""
    T, S = 4, 2
    xo, xp = _moving(T, S, 1728, ORI, 'l2'), _moving(T, S, 1000, POS, 'l2')
    eng = engines(1728, 1000)
    vf = eng.video_filter(S)
    one = _step(vf, xo, xp)
    vf.close()
    vf2 = eng.video_filter(S)
    for s in range(S):
        r = 1 * S + s                                             # the state after time step 1
        vf2.set_state(s, one['ori_soft'][r], one['pos_soft'][r], one['still'][r], one['ori'][r])
    rest = _step(vf2, xo[2:], xp[2:])
    vf2.close()
    for k in ('ori_soft', 'pos_soft', 'ori_distance', 'pos_distance', 'ori', 'pos'):
        np.testing.assert_allclose(rest[k], one[k][2 * S:], rtol=1e-6, atol=1e-12, err_msg=k)


def test_video_argument_errors_enqueue_nothing(engines, tables):
    from spef_amd import _lib as L
    from spef_amd.engine import Engine
    eng = engines(1728, 1000)
    lib = eng.lib
    h = C.c_void_p()
    assert lib.spef_video_create(eng.ctx, 2, 6, 0.8, 16.49, 0.5, 48.64, C.byref(h)) == L.ERR_ARG     # unknown metric
    assert lib.spef_video_create(eng.ctx, 2, -1, 0.8, 16.49, 0.5, 48.64, C.byref(h)) == L.ERR_ARG
    assert lib.spef_video_create(eng.ctx, 0, 0, 0.8, 16.49, 0.5, 48.64, C.byref(h)) == L.ERR_ARG     # n_streams < 1
    assert h.value is None
    with pytest.raises(AssertionError):
        eng.video_filter(2, 'cosine')
    bare = Engine(None, 'cuda:0')                                                                    # no tables
    assert lib.spef_video_create(bare.ctx, 2, 0, 0.8, 16.49, 0.5, 48.64, C.byref(h)) == L.ERR_STATE
    bare.set_decode_tables(tables[1728], None)                                                       # only one
    assert lib.spef_video_create(bare.ctx, 2, 0, 0.8, 16.49, 0.5, 48.64, C.byref(h)) == L.ERR_STATE
    bare.close()

    vf = eng.video_filter(2)
    T, S = 2, 2
    dev = 'cuda:0'
    oi = torch.rand(T * S, 1728, device=dev)
    pi = torch.rand(T * S, 1000, device=dev)
    outs = {k: torch.full(shape, -7.0, device=dev) for k, shape in
            (('of', (T * S, 1728)), ('od', (T * S,)), ('pf', (T * S, 1000)), ('pd', (T * S,)), ('q', (T * S, 4)),
             ('p', (T * S, 3)))}
    st = torch.full((T * S,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def call(t, s, ori=oi):
        p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
        return lib.spef_video_step(eng.ctx, vf.handle, p(ori), p(pi), t, s, None, p(outs['of']), p(outs['od']),
                                   p(outs['pf']), p(outs['pd']), p(outs['q']), p(outs['p']), p(st), None)
    assert call(T, 3) == L.ERR_ARG            # S != n_streams
    assert call(T, 1) == L.ERR_ARG
    assert call(0, S) == L.ERR_ARG            # T < 1
    assert call(-1, S) == L.ERR_ARG
    assert call(T, S, None) == L.ERR_ARG      # null input
    assert lib.spef_video_reset(vf.handle, 2, None) == L.ERR_ARG
    assert lib.spef_video_set_state(vf.handle, -1, None, None, None, None, None) == L.ERR_ARG
    torch.cuda.synchronize()
    assert all(bool((v == -7).all()) for v in outs.values()) and bool((st == -7).all())   # nothing ran
    # the first real step still is the stream's first frame: nothing above touched the state
    assert call(T, S) == L.OK
    torch.cuda.synchronize()
    assert bool((outs['od'][:S] == 0).all()) and bool((outs['od'][S:] > 0).all()) and not bool(st.any())
    vf.close()


# ---------------------------------------------------------------------------------------- 4. decode
def test_video_decode_and_status_bits(engines, tables):
    T, S = 5, 3
    xo, xp = _moving(T, S, 1728, ORI, 'l2'), _moving(T, S, 1000, POS, 'l2')
    eng = engines(1728, 1000)
    vf = eng.video_filter(S)
    out = _step(vf, xo, xp)
    rq = D.decode_orientation_batch(out['ori_soft'], tables[1728])
    assert D.angle_deg_stable(out['ori'], rq).max() < 1e-3
    rp = D.decode_position_batch(out['pos_soft'], tables['pos1000'])
    assert np.abs(out['pos'] - rp).max() < 1e-4
    # bad frames: an all-zero position row sets bit 2, a NaN row sets bits 1 and 4 (an all-zero orientation row: 1);
    # their distance is NaN, they pass through unfiltered, and the stream goes on from its last good frame
    bo, bp = xo.copy(), xp.copy()
    bp[1, 0] = 0.0
    bo[2, 1, 5] = np.nan
    bp[2, 1, 5] = np.nan
    bo[3, 2] = 0.0
    vf.reset()
    bad = _step(vf, bo, bp)
    vf.close()
    st = bad['status'].reshape(T, S)
    assert st[1, 0] & 2 and not st[1, 0] & 1
    assert st[2, 1] & 1 and st[2, 1] & 4
    assert st[3, 2] & 1 and not st[3, 2] & 2
    flagged = np.zeros((T, S), bool)
    flagged[1, 0] = flagged[2, 1] = flagged[3, 2] = True
    assert not st[~flagged].any()
    pd, od = bad['pos_distance'].reshape(T, S), bad['ori_distance'].reshape(T, S)
    assert np.isnan(pd[1, 0]) and np.isnan(pd[2, 1]) and np.isnan(od[2, 1]) and np.isnan(od[3, 2])
    assert np.isfinite(od[1, 0]) and np.isfinite(pd[3, 2])      # the other head of the same frame is filtered
    assert (bad['pos_soft'].reshape(T, S, -1)[1, 0] == 0).all()
    wo, do, _ = TP.filter_sequences(bo, ORI['n'], ORI['alpha'], 'l2')
    wp, dp, _ = TP.filter_sequences(bp, POS['n'], POS['alpha'], 'l2')
    np.testing.assert_allclose(bad['ori_soft'], wo.reshape(T * S, -1), rtol=1e-5, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(bad['pos_soft'], wp.reshape(T * S, -1), rtol=1e-5, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(bad['ori_distance'], do.reshape(-1), rtol=1e-5, equal_nan=True)
    np.testing.assert_allclose(bad['pos_distance'], dp.reshape(-1), rtol=1e-5, equal_nan=True)


# ---------------------------------------------------------------------------------------- 5. pole
def _raw_sign(q):
    """The decode's eigenvector of a one-hot PDF at a bin with quaternion q: +-q with its largest component > 0."""
    return q * np.sign(q[np.argmax(np.abs(q))])


def _host_pole(quats):
    """inference.py:136-144 over a sequence -> (poled quaternions, pole after each frame, flips, outliers)."""
    pole, out, poles, flips, outliers = None, [], [], 0, 0
    for q in quats:
        if pole is None:
            pole = q
        else:
            dot = np.dot(pole, q)
            if dot < 0:
                q = -q
                flips += 1
            if np.abs(dot) > 0.5:
                pole = q
            else:
                outliers += 1
        out.append(q)
        poles.append(pole)
    return np.stack(out), np.stack(poles), flips, outliers


def test_video_pole_continuity(engines, tables):
    h = tables[1728]
    raw = np.stack([_raw_sign(q) for q in h])
    # bins: start; a sign flip that moves the pole; an outlier (|dot| <= 0.5); a frame that agrees with the pole but
    # would be flipped had the outlier moved it; another flip
    mag = np.sort(np.abs(h), axis=1)
    clear = mag[:, 3] - mag[:, 2] > 0.05                # no tie for the largest component: the sign is certain
    dots = lambda p: raw @ p

    def pick(mask):
        assert (mask & clear).any()
        return int(np.argmax(mask & clear))
    a = pick(np.ones(len(h), bool))
    b = pick((dots(raw[a]) < -0.6) & (dots(raw[a]) > -0.95))
    pole = -raw[b]
    c = pick(np.abs(dots(pole)) < 0.3)
    outl = raw[c] if np.dot(pole, raw[c]) >= 0 else -raw[c]
    d = pick((dots(pole) > 0.55) & (dots(pole) < 0.95) & (dots(outl) < -0.1))
    e = pick((dots(raw[d]) < -0.6) & (dots(raw[d]) > -0.95))
    bins = [a, b, c, d, e, a]
    T = len(bins)
    xo = np.zeros((T, 2, 1728), np.float32)
    xo[np.arange(T), 0, bins] = 1.0                                 # stream 0: the crafted sequence
    xo[np.arange(T), 1, bins[::-1]] = 1.0                           # stream 1: the same bins backwards
    xp = _peaks(T, 2, 1000, 0.1)
    eng = engines(1728, 1000)
    # alpha = 0: weight 1, so every filtered PDF is the frame's own one-hot
    vf = eng.video_filter(2, 'l2', alpha_ori=0.0)
    unpoled = []
    for t in range(T):                                              # each frame alone after a reset: never flipped
        vf.reset()
        unpoled.append(_step(vf, xo[t:t + 1], xp[t:t + 1])['ori'])
    unpoled = np.stack(unpoled)                                     # [T, 2, 4]
    assert D.angle_deg_stable(unpoled[:, 0], h[bins]).max() < 1e-3
    vf.reset()
    still_in = np.ascontiguousarray(unpoled[::-1])                  # the still path: the reversed sequences
    out = _step(vf, xo, xp, still=still_in.copy())
    vf.close()
    got, got_still = out['ori'].reshape(T, 2, 4), out['still'].reshape(T, 2, 4)
    for s in range(2):
        want, poles, flips, outliers = _host_pole(unpoled[:, s])
        assert flips >= 1 and outliers >= 1, (s, flips, outliers)
        np.testing.assert_allclose(got[:, s], want, rtol=0, atol=1e-6)
        ws, _, _, _ = _host_pole(still_in[:, s])
        np.testing.assert_allclose(got_still[:, s], ws, rtol=0, atol=1e-6)
    # stream 0: the pole did not move on the outlier (frame 2), so frame 3 keeps its sign -- it would have been
    # negated against the outlier
    want, poles, _, _ = _host_pole(unpoled[:, 0])
    np.testing.assert_array_equal(poles[2], poles[1])
    assert np.dot(want[2], unpoled[3, 0]) < 0 < np.dot(poles[2], unpoled[3, 0])
    np.testing.assert_allclose(got[3, 0], unpoled[3, 0], rtol=0, atol=1e-6)


# ---------------------------------------------------------------------------------------- 6. end to end
@pytest.fixture(scope='module')
def model():
    from spef_amd.arch import mobilenet_v2
    from spef_amd.spe.spe_utils import SPEUtils
    from spef_amd.weights import synthetic_state_dict
    su = SPEUtils(None, 'classification', 12, 3, False, 'classification')
    sd = synthetic_state_dict(mobilenet_v2('ursonet', su.orientation.n_bins, su.position.n_bins), seed=1001)
    return su, sd


def _frames(count, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(rng.random((count, 3, 64, 64), dtype=np.float32))


def test_predict_sequence_equals_predict_loop_on_gpu(model):
    from spef_amd.inference import Inference
    su, sd = model
    x = _frames(5, 31)
    loop = Inference(sd, 'gpu_mi355x', su)
    want = [loop.predict(x[t:t + 1], 'Adaptative') for t in range(5)]
    loop.close()
    seq = Inference(sd, 'gpu_mi355x', su)
    got = seq.predict_sequence(x[:3]) + seq.predict_sequence(x[3:])      # one video in two calls
    assert len(got) == 5
    for (s1, lat, v1), (s2, _, v2) in zip(got, want):
        assert lat > 0 and set(s1) == set(s2) and set(v1) == set(v2)
        # the still pose, up to the bounds of tests/test_gpu_inference.py (the forward ran at another batch size)
        assert abs(float(np.dot(s1['ori'], s2['ori']))) == pytest.approx(1.0, abs=1e-6)
        np.testing.assert_allclose(s1['pos'], s2['pos'], rtol=0, atol=1e-4)
        np.testing.assert_allclose(s1['ori_soft'], s2['ori_soft'], rtol=1e-5, atol=1e-12)
        np.testing.assert_allclose(v1['ori_soft'], v2['ori_soft'], rtol=1e-5, atol=1e-12)
        np.testing.assert_allclose(v1['pos_soft'], v2['pos_soft'], rtol=1e-5, atol=1e-12)
        assert v1['ori_distance'] == pytest.approx(v2['ori_distance'], rel=1e-5, abs=1e-9)
        assert v1['pos_distance'] == pytest.approx(v2['pos_distance'], rel=1e-5, abs=1e-9)
        assert D.angle_deg_stable(v1['ori'][None], v2['ori'][None]).max() < 1e-3
        assert np.abs(v1['pos'] - v2['pos']).max() < 1e-4
    # the state is the one predict uses: a per-frame call continues the same video
    np.testing.assert_array_equal(seq.pdf_adapt_ori.previous_pdf, got[-1][2]['ori_soft'])
    _, _, v = seq.predict(x[4:5], 'Adaptative')
    assert v['ori_distance'] > 0 and v['pos_distance'] > 0          # not a first frame: the video goes on
    seq.reset()
    assert seq.pdf_adapt_ori.previous_pdf is None and seq.prev_video_ori is None
    first = seq.predict_sequence(x[:1])
    assert first[0][2]['ori_distance'] == 0 and first[0][2]['pos_distance'] == 0
    seq.close()


def test_pipeline_video_equals_predict_video(model):
    from spef_amd import _lib as L
    from spef_amd import blob as Bl
    from spef_amd.pipeline import StreamPipeline
    from spef_amd.spe_mi355x import SPEMi355x
    su, sd = model
    blob = Bl.pack(sd, dtype='fp16')
    T, S = 4, 2
    x = _frames(T * S, 32)
    spe = SPEMi355x(blob, 'cuda:0', su)
    still, video, lat = spe.predict_video(x, n_streams=S)
    assert lat > 0 and video['ori_soft'].shape == (T * S, su.orientation.n_bins) and video['ori'].shape == (T * S, 4)
    assert (video['ori_distance'][:S] == 0).all() and (video['ori_distance'][S:] > 0).all()
    spe.close()
    for graphs in (False, True):
        pipe = StreamPipeline(blob, 'cuda:0', depth=3, ori_bins=su.orientation.histogram,
                              pos_grid=su.position.histogram)
        pipe.use_graphs(graphs)
        vf = pipe.engine.video_filter(S)
        xs = [x[t * S:(t + 1) * S].cuda() for t in range(T)]
        outs = [pipe.submit(f, L.CLASSIFICATION, L.CLASSIFICATION, video=vf) for f in xs]
        pipe.synchronize()
        for t, d in enumerate(outs):
            v, r = d['video'], slice(t * S, (t + 1) * S)
            assert not v['status'].any().item()
            np.testing.assert_allclose(v['ori_soft'].cpu().numpy(), video['ori_soft'][r], rtol=1e-5, atol=1e-12)
            np.testing.assert_allclose(v['pos_soft'].cpu().numpy(), video['pos_soft'][r], rtol=1e-5, atol=1e-12)
            np.testing.assert_allclose(v['ori_distance'].cpu().numpy(), video['ori_distance'][r], rtol=1e-5, atol=1e-9)
            np.testing.assert_allclose(v['pos_distance'].cpu().numpy(), video['pos_distance'][r], rtol=1e-5, atol=1e-9)
            assert D.angle_deg_stable(v['ori'].cpu().numpy(), video['ori'][r]).max() < 1e-3
            assert np.abs(v['pos'].cpu().numpy() - video['pos'][r]).max() < 1e-4
            assert (np.abs(np.sum(d['ori'].cpu().numpy() * still['ori'][r], axis=1)) > 1 - 1e-6).all()
        vf.close()
        pipe.close()


def test_video_step_graph_capture(engines):
    """A video step captured on one stream (a linear graph) and replayed twice equals two eager steps bit for bit."""
    T, S = 2, 3
    xo, xp = _moving(T, S, 1728, ORI, 'l2'), _moving(T, S, 1000, POS, 'l2')
    eng = engines(1728, 1000)
    vf = eng.video_filter(S)
    eager = [_step(vf, xo, xp), _step(vf, xo, xp)]      # the second step filters the same frames against the state
    vf.reset()
    dec = {'ori_soft': torch.from_numpy(xo.reshape(T * S, -1)).cuda(), 'pos_soft': torch.from_numpy(xp.reshape(T * S, -1)).cuda(),
           'ori': torch.from_numpy(np.tile(np.array([1, 0, 0, 0], np.float32), (T * S, 1))).cuda()}
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = vf.step(dec, T)
    for k in range(2):
        g.replay()
        torch.cuda.synchronize()
        for name in ('ori_soft', 'pos_soft', 'ori_distance', 'pos_distance', 'ori', 'pos', 'status'):
            np.testing.assert_array_equal(out[name].cpu().numpy(), eager[k][name], err_msg=f'replay {k} {name}')
    assert (eager[1]['ori_distance'] > 0).all()
    del g
    vf.close()
