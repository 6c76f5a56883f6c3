"""Host side of the batched video path: ``spef_amd.temporal.filter_sequences`` (the CPU statement of what the device
filter in csrc/k_video.hip computes) against the reference fixture and against per-stream ``TemporalPDF``, and
``Inference.predict_sequence`` against T calls of ``Inference.predict`` with a stub engine. No GPU."""
import numpy as np
import pytest

from spef_amd import temporal as T

SETTINGS = ((0.8, 16.49, 'ori'), (0.5, 48.64, 'pos'))     # the Inference engine's filters (inference.py:38-39)


def _tol(metric):
    # float64 sums here, float32 sums in the fixture: 2.6e-6 (PDF) / 1.2e-7 (distance) apart; the fixture's own
    # float32 cumsum puts Wasserstein 3.6e-5 / 2.9e-5 away
    return 1e-4 if metric == 'wasserstein' else 1e-5


@pytest.mark.parametrize('metric', T.METRICS)
def test_filter_sequences_matches_reference_fixture(golden, metric):
    g = golden('temporal_pdf.npz')
    seq = g['seq'][:, None, :]                            # [T, S = 1, n]
    for n, alpha, tag in SETTINGS:
        pdf, dist, st = T.filter_sequences(seq, n, alpha, metric)
        assert pdf.dtype == np.float32 and dist.dtype == np.float32 and pdf.shape == seq.shape
        np.testing.assert_allclose(pdf[:, 0], g[f'{metric}_{tag}_pdf'], rtol=_tol(metric), atol=1e-12)
        np.testing.assert_allclose(dist[:, 0], g[f'{metric}_{tag}_dist'], rtol=_tol(metric), atol=1e-12)
        np.testing.assert_array_equal(st['pdf'][0], pdf[-1, 0])
        assert st['have'].all()


def _random_sequences(seed, t, s, n):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.random((t, s, n), dtype=np.float32) + np.float32(0.05)
    return x * rng.uniform(0.5, 2.0, (t, s, 1)).astype(np.float32)      # not normalised: the filter does that


@pytest.mark.parametrize('metric', T.METRICS)
def test_filter_sequences_equals_per_stream_temporal_pdf(metric):
    x = _random_sequences(3, 5, 3, 211)
    pdf, dist, _ = T.filter_sequences(x, 0.8, 16.49, metric)
    for s in range(3):
        f = T.TemporalPDF(0.8, 16.49, metric)
        for t in range(5):
            p, d = f.update_pdf(x[t, s])
            np.testing.assert_allclose(pdf[t, s], p, rtol=_tol(metric), atol=1e-12)
            np.testing.assert_allclose(dist[t, s], d, rtol=_tol(metric), atol=1e-9)
    assert (dist[0] == 0).all() and (dist[1:] > 0).all()


@pytest.mark.parametrize('metric', T.METRICS)
def test_filter_sequences_split_is_identical(metric):
    x = _random_sequences(4, 6, 2, 97)
    pdf, dist, st = T.filter_sequences(x, 0.5, 48.64, metric)
    p1, d1, s1 = T.filter_sequences(x[:2], 0.5, 48.64, metric)
    p2, d2, s2 = T.filter_sequences(x[2:], 0.5, 48.64, metric, state=s1)
    np.testing.assert_array_equal(np.concatenate([p1, p2]), pdf)
    np.testing.assert_array_equal(np.concatenate([d1, d2]), dist)
    np.testing.assert_array_equal(s2['pdf'], st['pdf'])


def test_filter_sequences_bad_frame_leaves_the_state():
    x = _random_sequences(5, 4, 2, 33)
    x[1, 0] = 0.0                                         # stream 0: an all-zero frame, then a NaN one
    x[2, 0, 7] = np.nan
    pdf, dist, _ = T.filter_sequences(x, 0.8, 16.49, 'l2')
    ref, rd, _ = T.filter_sequences(x[[0, 3]], 0.8, 16.49, 'l2')
    np.testing.assert_array_equal(pdf[3, 0], ref[1, 0])   # filtered against the last good frame
    assert np.isnan(dist[1, 0]) and np.isnan(dist[2, 0]) and dist[3, 0] == rd[1, 0]
    assert (pdf[1, 0] == 0).all() and np.isnan(pdf[2, 0, 7])
    full, _, _ = T.filter_sequences(x[:, 1:], 0.8, 16.49, 'l2')
    np.testing.assert_array_equal(pdf[:, 1], full[:, 0])  # the other stream is untouched
    with pytest.raises(ValueError):
        T.filter_sequences(x, metric='cosine')


def test_lib_declares_video_symbols():
    from spef_amd import _lib
    for name in ('spef_video_create', 'spef_video_reset', 'spef_video_step', 'spef_video_destroy',
                 'spef_video_set_state'):
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 4
    assert tuple(sorted(_lib.METRIC_IDS, key=_lib.METRIC_IDS.get)) == T.METRICS
    assert len(_lib.SIGNATURES['spef_video_step'][1]) == 15


# ---------------------------------------------------------------------------------------- Inference.predict_sequence
class _StubDevice:
    """Stands in for Engine + VideoFilter: decode of PDFs by the oracle, the filter by TemporalPDF per frame."""

    def __init__(self, su):
        import torch
        self.su = su
        self.device = torch.device('cpu')

    def decode(self, ori_mode, pos_mode, lo, lp, want_soft=True):
        import torch
        from oracle import decode_ref as D
        po, pp = D.softmax_f32(lo.numpy()), D.softmax_f32(lp.numpy())
        q = D.decode_orientation_batch(po, self.su.orientation.histogram).astype(np.float32)
        p = D.decode_position_batch(pp, self.su.position.histogram).astype(np.float32)
        return {'ori': torch.from_numpy(q), 'pos': torch.from_numpy(p),
                'status': torch.zeros(lo.shape[0], dtype=torch.int32)}


class _StubEngine:
    """predict() -> a fixed sequence of batch-1 pose dicts (what SPEMi355x.predict returns); predict_video() -> the
    same frames through the per-frame host filter, the way SPEMi355x.predict_video returns them (batched, poles
    applied)."""

    def __init__(self, poses, su):
        self.poses = list(poses)
        self.closed = False
        self.engine = _StubDevice(su)
        self.state = None
        self.video_calls = 0

    def predict(self, image):
        b = image.shape[0]
        take, self.poses = self.poses[:b], self.poses[b:]
        return {k: np.concatenate([p[k] for p in take]) for k in take[0]}, 1.25 * b

    def close(self):
        self.closed = True

    def video_filter(self, n_streams, metric, **params):
        assert n_streams == 1
        self.cfg = (metric, params)
        return self

    def set_state(self, stream, ori_pdf, pos_pdf, still_pole, video_pole):
        self.state = [ori_pdf, pos_pdf, still_pole, video_pole]

    @staticmethod
    def _pole(pole, q):
        if pole is None:
            return q, q
        dot = np.dot(pole, q)
        if dot < 0:
            q = -q
        return (q if np.abs(dot) > 0.5 else pole), q

    def predict_video(self, images, n_streams, metric, **params):
        import torch
        assert (metric, params) == self.cfg
        self.video_calls += 1
        b = images.shape[0]
        still, lat = self.predict(images)
        fo = T.TemporalPDF(params['n_ori'], params['alpha_ori'], metric)
        fp = T.TemporalPDF(params['n_pos'], params['alpha_pos'], metric)
        fo.previous_pdf, fp.previous_pdf, spole, vpole = self.state
        video = {k: [] for k in ('ori', 'pos', 'ori_soft', 'pos_soft', 'ori_distance', 'pos_distance')}
        still['ori'] = still['ori'].copy()
        for t in range(b):
            spole, still['ori'][t] = self._pole(spole, still['ori'][t])
            po, do = fo.update_pdf(still['ori_soft'][t])
            pp, dp = fp.update_pdf(still['pos_soft'][t])
            with np.errstate(divide='ignore'):
                dec = self.engine.decode(1, 1, torch.from_numpy(np.log(po)[None]), torch.from_numpy(np.log(pp)[None]))
            vpole, q = self._pole(vpole, dec['ori'][0].numpy())
            for k, v in zip(video, (q, dec['pos'][0].numpy(), po, pp, do, dp)):
                video[k].append(v)
        return still, {k: np.stack([np.asarray(a) for a in v]) for k, v in video.items()}, lat


def _poses(su, count, seed):
    """Still poses of slowly moving peaked PDFs, with a sign flip and an outlier among the quaternions."""
    rng = np.random.Generator(np.random.PCG64(seed))
    no, npos = su.orientation.n_bins, su.position.n_bins
    out = []
    for t in range(count):
        po = np.exp(-0.5 * ((np.arange(no) - 300 - 2 * t) / 6.0) ** 2).astype(np.float32) + np.float32(1e-4)
        pp = np.exp(-0.5 * ((np.arange(npos) - 500 - t) / 4.0) ** 2).astype(np.float32) + np.float32(1e-4)
        q = np.array([0.5, 0.5, 0.5, 0.5], np.float32) + rng.normal(0, 0.02, 4).astype(np.float32)
        q /= np.linalg.norm(q)
        if t % 3 == 1:
            q = -q                                        # a sign flip
        if t == 2:
            q = np.array([0.0, 0.0, 0.0, 1.0], np.float32)   # an outlier: |dot| = 0.5 with the pole
        out.append({'ori': q[None], 'pos': rng.normal(0, 1, (1, 3)).astype(np.float32),
                    'ori_soft': (po / po.sum())[None], 'pos_soft': (pp / pp.sum())[None]})
    return out


def _inference(poses, su):
    from spef_amd.inference import Inference
    stub = _StubEngine(poses, su)
    return Inference(None, 'gpu_host', su, engine_factories={'gpu_host': lambda m, s: stub}), stub


def _assert_triples_equal(a, b):
    assert len(a) == len(b)
    for (s1, l1, v1), (s2, l2, v2) in zip(a, b):
        assert l1 == l2
        for x, y in ((s1, s2), (v1, v2)):
            assert (x is None) == (y is None)
            if x is not None:
                assert set(x) == set(y)
                for k in x:
                    np.testing.assert_array_equal(np.asarray(x[k]), np.asarray(y[k]), err_msg=k)


@pytest.mark.parametrize('video_type', ['Adaptative', None])
def test_predict_sequence_equals_predict_loop(video_type):
    import torch
    from spef_amd.spe.camera import SpeedCamera
    from spef_amd.spe.keypoints import KeyPoints
    from spef_amd.spe.spe_utils import SPEUtils
    kp3d = np.random.default_rng(0).normal(0, 0.3, (11, 3)).astype(np.float32)
    su = SPEUtils(SpeedCamera, 'classification', 12, 3, False, 'classification',
                  keypoints_path=KeyPoints(SpeedCamera, kp3d))
    n = 7
    x = torch.zeros(n, 3, 8, 8)
    loop, _ = _inference(_poses(su, n, 11), su)
    want = [loop.predict(x[t:t + 1], video_type) for t in range(n)]
    # the same video as one sequence, and as predict / predict_sequence calls mixed on one state
    seq, stub = _inference(_poses(su, n, 11), su)
    got = seq.predict_sequence(x, video_type)
    _assert_triples_equal(got, want)
    assert 'keypoints' in got[0][0] and 'bbox' in got[0][0]
    assert stub.video_calls == (1 if video_type else 0)
    mix, _ = _inference(_poses(su, n, 11), su)
    got = mix.predict_sequence(x[:2], video_type) + [mix.predict(x[2:3], video_type)] + \
        mix.predict_sequence(x[3:], video_type)
    _assert_triples_equal(got, want)
    for a, b in ((mix.prev_still_ori, loop.prev_still_ori), (mix.prev_video_ori, loop.prev_video_ori),
                 (mix.pdf_adapt_ori.previous_pdf, loop.pdf_adapt_ori.previous_pdf)):
        assert (a is None) == (b is None)
        if a is not None:
            np.testing.assert_array_equal(a, b)
    mix.reset()
    assert mix.prev_video_ori is None and mix.pdf_adapt_pos.previous_pdf is None
    with pytest.raises(ValueError):
        mix.predict_sequence(x, 'Kalman')
