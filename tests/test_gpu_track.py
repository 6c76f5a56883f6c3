"""GPU: the pose tracker (csrc/k_track.hip) against its NumPy twin (spef_amd/spe/track.py), and its way up through
Engine, SPEMi355x, StreamPipeline and Inference."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from spef_amd import _lib as L
from spef_amd import blob as Bl
from spef_amd.arch import mobilenet_v2
from spef_amd.spe import track as TK
from spef_amd.weights import plant_keypoint_head, synthetic_state_dict

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_inputs as TI  # noqa: E402

pytestmark = pytest.mark.gpu

ULP16 = 16 * 2.0 ** -23          # the floor for a float32 output cast (COV_TOL of tests/test_gpu_refine.py)
KEYS = ('ori', 'pos', 'mahalanobis', 'track_status', 'cov', 'rates')


@pytest.fixture(scope='module')
def eng():
    from spef_amd.engine import Engine
    e = Engine(None, 'cuda:0')       # the tracker needs the context's device and profiler only
    yield e
    e.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _dec(q, t, c, s, rows=slice(None)):
    d = {'ori': torch.from_numpy(np.ascontiguousarray(q[rows])).cuda(),
         'pos': torch.from_numpy(np.ascontiguousarray(t[rows])).cuda()}
    if c is not None:
        d['cov'] = torch.from_numpy(np.ascontiguousarray(c[rows])).cuda()
    if s is not None:
        d['status'] = torch.from_numpy(np.ascontiguousarray(s[rows])).cuda()
    return d


@pytest.fixture(scope='module')
def inputs():
    """H3, H4 and H5 as S = 3, T = 64, rounded to the float32 the kernel reads."""
    q, t, c, s = TI.three_streams()
    return q.astype(np.float32), t.astype(np.float32), c.astype(np.float32), s.astype(np.int32)


@pytest.fixture(scope='module')
def whole(eng, inputs):
    """(T, S) = (64, 3) in one call: outputs and the state after it; computed once."""
    trk = eng.tracker(3, **TI.PARAMS)
    out = _np(trk.step(_dec(*inputs), TI.N, want_cov=True, want_rates=True))
    state = trk.state().cpu().numpy()
    trk.close()
    return out, state


def test_kernel_matches_twin(inputs, whole):
    """G1. track_status equals the twin's; every other output is within a tolerance relative to the output's largest
    magnitude: ten times the twin's own sensitivity to a 1e-9 relative perturbation of the measurements, but never
    below 16 float32 ulps. Measured sensitivities (relative to the largest magnitude): ori 1.1e-9, pos 1.3e-9,
    mahalanobis 2.1e-9, cov 0 (it does not depend on the measured values), rates 1.2e-7 -- so the floor, 1.9e-6,
    decides for every output."""
    q, t, c, s = inputs
    twin = TK.PoseTrackerHost(3, **TI.PARAMS).step(q, t, c, s)
    rng = np.random.default_rng(0)
    pert = TK.PoseTrackerHost(3, **TI.PARAMS).step(q * (1 + 1e-9 * rng.choice([-1.0, 1.0], q.shape)),
                                                   t * (1 + 1e-9 * rng.choice([-1.0, 1.0], t.shape)), c, s)
    dev, _ = whole
    assert np.array_equal(dev['track_status'], twin['track_status'])
    assert set(np.unique(twin['track_status'])) == {0, 1, 2, 6}
    for k in ('ori', 'pos', 'mahalanobis', 'cov', 'rates'):
        fin = np.isfinite(twin[k])
        assert np.array_equal(np.isfinite(dev[k]), fin), k
        mag = np.abs(twin[k][fin]).max()
        sens = np.abs(twin[k] - pert[k])[fin].max() / mag
        tol = max(10 * sens, ULP16)
        err = np.abs(dev[k].astype(np.float64) - twin[k])[fin].max() / mag
        print(f'{k}: sensitivity {sens:.2e}, tolerance {tol:.2e}, kernel against twin {err:.2e}')
        assert err <= tol, k


def test_cutting_on_the_device(eng, inputs, whole):
    """G2. (64, 3) in one call, 64 calls of T = 1 and 5 + 59 agree bit for bit in every output and in the state; so
    does a step that writes its pose over its input; at S = 65 every copy of a stream equals its original."""
    out, state = whole
    for cuts in ([1] * 64, [5, 59]):
        trk = eng.tracker(3, **TI.PARAMS)
        parts, a = [], 0
        for n in cuts:
            parts.append(_np(trk.step(_dec(*inputs, rows=slice(3 * a, 3 * (a + n))), n, want_cov=True, want_rates=True)))
            a += n
        for k in KEYS:
            assert np.array_equal(_bits(np.concatenate([p[k] for p in parts])), _bits(out[k])), (k, cuts[0])
        assert np.array_equal(_bits(trk.state().cpu().numpy()), _bits(state))
        trk.close()

    # in place: quat_out == quat, pos_out == pos
    from spef_amd.engine import _ptr, _stream
    trk = eng.tracker(3, **TI.PARAMS)
    d = _dec(*inputs)
    ts = torch.empty(3 * TI.N, dtype=torch.int32, device='cuda')
    assert eng.lib.spef_track_step(trk.handle, _ptr(d['ori']), _ptr(d['pos']), _ptr(d['cov']), _ptr(d['status']), TI.N, 3,
                                   _ptr(d['ori']), _ptr(d['pos']), None, None, None, _ptr(ts),
                                   _stream(eng.device)) == L.OK
    assert np.array_equal(_bits(d['ori'].cpu().numpy()), _bits(out['ori']))
    assert np.array_equal(_bits(d['pos'].cpu().numpy()), _bits(out['pos']))
    assert np.array_equal(ts.cpu().numpy(), out['track_status'])
    assert np.array_equal(_bits(trk.state().cpu().numpy()), _bits(state))
    trk.close()

    S = 65
    src = np.arange(S) % 3
    wide = tuple(np.ascontiguousarray(x.reshape((TI.N, 3) + x.shape[1:])[:, src]).reshape((TI.N * S,) + x.shape[1:])
                 for x in inputs)
    trk = eng.tracker(S, **TI.PARAMS)
    big = _np(trk.step(_dec(*wide), TI.N, want_cov=True, want_rates=True))
    st = trk.state().cpu().numpy()
    trk.close()
    for k in KEYS:
        got = big[k].reshape((TI.N, S) + big[k].shape[1:])
        want = out[k].reshape((TI.N, 3) + out[k].shape[1:])[:, src]
        assert np.array_equal(_bits(got), _bits(want)), k
    assert np.array_equal(_bits(st), _bits(state[src]))


def test_anchor_on_the_device(eng, golden):
    """G3. Configured like the reference's position filter, the position is within 16 float32 ulps of the fixture
    rounded to float32."""
    g = golden('kalman_pos.npz')
    trk = eng.tracker(1, **TI.ANCHOR)
    q = np.tile(np.float32([1, 0, 0, 0]), (40, 1))
    out = _np(trk.step(_dec(q, g['pos_in'].astype(np.float32), None, None), 40))
    trk.close()
    want = g['pos_out'].astype(np.float32)
    ulp = np.spacing(np.abs(want))
    err = np.abs(out['pos'].astype(np.float64) - want) / ulp
    print(f'largest position difference: {err.max():.2f} ulps')
    assert not out['track_status'].any()
    assert err.max() <= 16


def test_argument_and_state_errors(eng, inputs):
    """G4. Every SPEF_ERR_ARG case with nothing written; the optional pointers may each be NULL; reset(stream)
    clears that stream alone."""
    from spef_amd.engine import _ptr, _stream
    lib, st = eng.lib, _stream(eng.device)

    def params(**kw):
        p = dict(q=[1.0] * 4, p0=[1.0] * 4, r=[100.0] * 2, cov_scale=1.0, gate_chi2=0.0, max_coast=0)
        p.update(kw)
        return L.TrackParams((C.c_double * 4)(*p['q']), (C.c_double * 4)(*p['p0']), (C.c_double * 2)(*p['r']),
                             p['cov_scale'], p['gate_chi2'], p['max_coast'])

    h = C.c_void_p()
    good = params()
    for ctx, n, prm, out in ((None, 1, good, h), (eng.ctx, 0, good, h), (eng.ctx, 65537, good, h),
                             (eng.ctx, 1, None, h), (eng.ctx, 1, good, None)):
        assert lib.spef_track_create(ctx, n, C.byref(prm) if prm is not None else None,
                                     C.byref(out) if out is not None else None) == L.ERR_ARG
    for kw in (dict(q=[1, 1, -1, 1]), dict(p0=[float('nan'), 1, 1, 1]), dict(r=[1, float('inf')]), dict(cov_scale=-1.0),
               dict(gate_chi2=float('nan')), dict(max_coast=-1)):
        assert lib.spef_track_create(eng.ctx, 1, C.byref(params(**kw)), C.byref(h)) == L.ERR_ARG, kw
    assert not h.value

    trk = eng.tracker(3, **TI.PARAMS)
    d = _dec(*inputs, rows=slice(0, 6))
    qo, po = torch.full((6, 4), 7.0, device='cuda'), torch.full((6, 3), 7.0, device='cuda')
    ts = torch.full((6,), 77, dtype=torch.int32, device='cuda')
    buf = torch.full((3, L.TRACK_STATE_DOUBLES), 5.0, dtype=torch.float64, device='cuda')

    def step(tr=trk.handle, q=d['ori'], p=d['pos'], T=2, S=3, qo=qo, po=po, ts=ts, cov=d['cov'], status=d['status']):
        return lib.spef_track_step(tr, _ptr(q), _ptr(p), _ptr(cov), _ptr(status), T, S, _ptr(qo), _ptr(po), None, None,
                                   None, _ptr(ts), st)
    for kw in (dict(tr=None), dict(q=None), dict(p=None), dict(qo=None), dict(po=None), dict(ts=None), dict(S=2),
               dict(S=4), dict(T=0), dict(T=-1)):
        assert step(**kw) == L.ERR_ARG, kw
    for fn in (lib.spef_track_get_state, lib.spef_track_set_state):
        for first, n in ((-1, 1), (3, 1), (2, 2), (0, 0), (0, 4)):
            assert fn(trk.handle, first, n, _ptr(buf), st) == L.ERR_ARG, (first, n)
        assert fn(trk.handle, 0, 1, None, st) == L.ERR_ARG and fn(None, 0, 1, _ptr(buf), st) == L.ERR_ARG
    for stream in (-2, 3):
        assert lib.spef_track_reset(trk.handle, stream, st) == L.ERR_ARG
    assert lib.spef_track_reset(None, 0, st) == L.ERR_ARG
    torch.cuda.synchronize()
    assert (qo == 7).all().item() and (po == 7).all().item() and (ts == 77).all().item() and (buf == 5).all().item()
    assert not trk.state().any().item()                      # nothing ran: no stream has a track

    # cov, status (and d2, cov_out, rates_out above) may each be NULL
    assert step(cov=None) == L.OK
    torch.cuda.synchronize()
    assert (ts == 0).all().item() and trk.state()[:, 0].eq(1).all().item()
    assert step(status=None) == L.OK
    trk.reset(1)
    s3 = trk.state().cpu().numpy()
    assert not s3[1].any() and s3[0, 0] == 1 and s3[2, 0] == 1
    fresh = eng.tracker(3, **TI.PARAMS)
    fresh.set_state(s3[2:3], first=1)                        # state -> set_state, another stream
    assert np.array_equal(_bits(fresh.state(1, 1).cpu().numpy()), _bits(s3[2:3]))
    assert not fresh.state(0, 1).any().item()
    trk.reset()
    assert not trk.state().any().item()
    fresh.close()
    trk.close()


def test_track_step_graph_capture(eng, inputs, whole):
    """A step captured on a stream and replayed continues the sequence like eager steps, bit for bit."""
    out, _ = whole
    trk = eng.tracker(3, **TI.PARAMS)
    d = _dec(*inputs, rows=slice(0, 3))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        o = trk.step(d, 1)
    for f in range(3):
        for k, x in zip(('ori', 'pos', 'cov', 'status'), inputs):
            d[k].copy_(torch.from_numpy(np.ascontiguousarray(x[3 * f:3 * f + 3])))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(o['ori'].cpu().numpy()), _bits(out['ori'][3 * f:3 * f + 3])), f
        assert np.array_equal(_bits(o['pos'].cpu().numpy()), _bits(out['pos'][3 * f:3 * f + 3])), f
    del g
    trk.close()


# ---------------------------------------------------------------------------------------- end to end
def _kp_model(golden):
    """The planted keypoint head of test_pipeline_matches_single_engine (tests/test_gpu_refine.py), fp16x2."""
    g = golden('keypoints.npz')
    i = int(np.argmin(np.abs(g['t'][:, 2] - np.median(g['t'][:, 2]))))
    arch = mobilenet_v2('keypoints')
    sd = plant_keypoint_head(synthetic_state_dict(arch, seed=1001, head_std=2e-4), g['kp2d'][i])
    return g, Bl.pack(sd, arch, dtype='fp16x2')


def _kp_utils(g):
    from spef_amd.spe.keypoints import KeyPoints
    from spef_amd.spe.spe_utils import SPEUtils

    class Cam:
        K, nu, nv = g['K'], float(g['nu']), float(g['nv'])
    return SPEUtils(Cam, 'keypoints', pos_mode='keypoints', keypoints_path=KeyPoints(Cam, g['kp3d']))


def _u8_frames(count, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(rng.integers(0, 256, (count, 240, 384, 3), dtype=np.uint8))


def test_keypoint_mode_end_to_end(golden):
    """G5. predict_tracked (T = 3, S = 2, refinement on) equals forward -> decode_keypoints(want_cov) -> tracker.step
    at engine level bit for bit; a row whose raw output is NaN is reported with bit 1 and coasted, its neighbours are
    as before and nothing raises; decode_keypoints without want_cov returns today's keys."""
    from spef_amd.spe_mi355x import SPEMi355x
    g, blob = _kp_model(golden)
    p = dict(gate_chi2=TI.GATE, max_coast=3)
    spe = SPEMi355x(blob, 'cuda:0', _kp_utils(g), keypoint_refine=(50, 4.0))
    try:
        x = _u8_frames(6, 41)
        still, tracked, lat = spe.predict_tracked(x, n_streams=2, **p)
        assert lat > 0 and set(tracked) == {'ori', 'pos', 'mahalanobis', 'track_status'}
        assert set(still) == {'keypoints', 'ori', 'pos', 'ori_epnp', 'pos_epnp', 'reproj_rms'}
        assert spe.tracker(2, **p) is spe.tracker(2, **p)                    # cached like video_filter
        eng = spe.engine
        raw, _ = eng.forward(x.cuda())
        dec = eng.decode_keypoints(raw, want_cov=True)
        assert set(dec) == {'keypoints', 'ori', 'pos', 'status', 'ori_epnp', 'pos_epnp', 'fit', 'refine_iters', 'cov'}
        assert set(eng.decode_keypoints(raw)) == set(dec) - {'cov'}
        assert np.isfinite(dec['cov'].cpu().numpy()).all()
        trk = eng.tracker(2, **p)
        want = _np(trk.step(dec, 3))
        for k in tracked:
            assert np.array_equal(_bits(tracked[k]), _bits(want[k])), k
        assert np.array_equal(_bits(still['ori']), _bits(dec['ori'].cpu().numpy()))
        assert not tracked['track_status'].any()

        # row 3 (step 1 of stream 1) loses its raw output
        trk.reset()
        bad = raw.clone()
        bad[3] = float('nan')
        dec2 = eng.decode_keypoints(bad, want_cov=True)
        got = _np(trk.step(dec2, 3))
        print('decode status of the rows:', dec2['status'].cpu().numpy().tolist())
        assert got['track_status'].tolist() == [0, 0, 0, 1, 0, 0] and np.isnan(got['mahalanobis'][3])
        assert np.isfinite(got['ori']).all() and np.isfinite(got['pos']).all()
        for k in ('ori', 'pos', 'mahalanobis'):                             # stream 0 and the rows before: as before
            assert np.array_equal(_bits(got[k][[0, 1, 2, 4]]), _bits(want[k][[0, 1, 2, 4]])), k
        assert np.array_equal(_bits(got['pos'][3]), _bits(want['pos'][1]))   # coasted with zero velocity
        trk.close()
    finally:
        spe.close()


def test_pipeline_ordering(golden):
    """G6. Four batches of B = 6 (T = 3, S = 2) through submit_keypoints(track=) at depth 3: every dec['track'] and the
    final state equal one engine stepping the batches in order on one stream, bit for bit. With score= as well, track
    1 logs the tracked poses and a coasted row is not flagged FLAG_STATUS."""
    from spef_amd.pipeline import StreamPipeline
    from spef_amd.score import FLAG_STATUS
    g, blob = _kp_model(golden)
    p = dict(gate_chi2=TI.GATE, max_coast=3)
    batches = [_u8_frames(6, 50 + k).cuda() for k in range(4)]
    pipe = StreamPipeline(blob, 'cuda:0', depth=3)
    try:
        pipe.set_keypoints(g['kp3d'], g['K'], float(g['nu']), float(g['nv']))
        pipe.set_keypoint_refine(50, 4.0)
        trk = pipe.engine.tracker(2, **p)
        outs = [pipe.submit_keypoints(x, track=trk) for x in batches]
        pipe.synchronize()
        state = trk.state().cpu().numpy()
        ref, one = pipe.engines[0], pipe.engine.tracker(2, **p)
        for x, o in zip(batches, outs):
            want = _np(one.step(ref.decode_keypoints(ref.forward(x)[0], want_cov=True), 3))
            assert set(o['track']) == {'ori', 'pos', 'mahalanobis', 'track_status'} and 'cov' in o
            for k in want:
                assert np.array_equal(_bits(o['track'][k].cpu().numpy()), _bits(want[k])), k
        assert np.array_equal(_bits(one.state().cpu().numpy()), _bits(state))
        assert state[:, 0].tolist() == [1, 1]

        # scoring: with the tracked poses of a batch as its targets, track 1 (the tracked poses) has error zero
        one.reset()
        trk.reset()
        want = _np(one.step(ref.decode_keypoints(ref.forward(batches[0])[0], want_cov=True), 3))
        scorer = pipe.engine.scorer(2, 2, 16)
        try:
            pipe.submit_keypoints(batches[0], track=trk, score=(scorer, {'ori': want['ori'], 'pos': want['pos']}))
            res = scorer.result()
        finally:
            scorer.close()
        assert (res['pos_error'][:, 1] == 0.0).all() and not (res['flags'][:, 1].astype(np.int64) & FLAG_STATUS).any()
        assert (res['n'] == 3).all() and np.isfinite(res['pos_error'][:, 0]).all()    # track 0: the still poses
        one.close()
        trk.close()
    finally:
        pipe.close()


@pytest.mark.parametrize('graphs', (False, True))
def test_pipeline_submit_with_classification_heads(graphs):
    """StreamPipeline.submit(track=) behind classification heads, eager and with recorded graphs (the step stays
    outside the graph): three batches of T = 2, S = 2 at depth 2 equal one engine stepping them in order, bit for bit."""
    from spef_amd.pipeline import StreamPipeline
    from spef_amd.spe.spe_utils import SPEUtils
    su = SPEUtils(None, 'classification', 12, 3, False, 'classification')
    sd = synthetic_state_dict(mobilenet_v2('ursonet', su.orientation.n_bins, su.position.n_bins), seed=1001)
    rng = np.random.Generator(np.random.PCG64(71))
    batches = [torch.from_numpy(rng.random((4, 3, 64, 64), dtype=np.float32)).cuda() for _ in range(3)]
    pipe = StreamPipeline(Bl.pack(sd, dtype='fp16'), 'cuda:0', depth=2, ori_bins=su.orientation.histogram,
                          pos_grid=su.position.histogram)
    try:
        pipe.use_graphs(graphs)
        trk, one = pipe.engine.tracker(2), pipe.engine.tracker(2)
        outs = [pipe.submit(x, L.CLASSIFICATION, L.CLASSIFICATION, track=trk) for x in batches]
        pipe.synchronize()
        ref = pipe.engines[0]
        for x, o in zip(batches, outs):
            want = _np(one.step(ref.decode(L.CLASSIFICATION, L.CLASSIFICATION, *ref.forward(x)), 2))
            for k in want:
                assert np.array_equal(_bits(o['track'][k].cpu().numpy()), _bits(want[k])), k
        assert np.array_equal(_bits(trk.state().cpu().numpy()), _bits(one.state().cpu().numpy()))
        assert not outs[-1]['track']['track_status'].any().item()
        one.close()
        trk.close()
    finally:
        pipe.close()


def test_coasted_rows_are_not_flagged_by_the_scorer(eng, inputs):
    """G6, the scorer's view: a coasted row (track status 1) scores as a good row; only a row that passed through
    without a track (bit 8) carries FLAG_STATUS."""
    from spef_amd.pipeline import StreamPipeline
    from spef_amd.score import FLAG_STATUS
    q, t, c, s = (x.reshape((TI.N, 3) + x.shape[1:])[:, 1] for x in inputs)       # H4: dropouts at frames 20..25
    s = s.copy()
    s[0] = 8                                                                       # and no track on frame 0
    trk = eng.tracker(1, **TI.PARAMS)
    out = trk.step(_dec(q, t, c, s), TI.N)
    scorer = eng.scorer(1, 2, TI.N)
    try:
        scorer.step(1, StreamPipeline._tracked_for_score(torch.cuda.current_stream(), {'track': out}),
                    (out['ori'], out['pos']), TI.N)
        _, flags = scorer.log(1, 0, 0, TI.N)
    finally:
        scorer.close()
        trk.close()
    ts = out['track_status'].cpu().numpy()
    assert ts[0] == 9 and (ts[20:26] == 1).all()
    assert flags[0] & FLAG_STATUS and not (flags[1:] & FLAG_STATUS).any()


@pytest.mark.parametrize('head', ('classification', 'keypoints'))
def test_inference_tracker(golden, head):
    """G7. predict_sequence(x, 'Tracker') over 7 frames, seven predict calls and a 2 + 1 + 4 mix each continue one
    track: the forward runs at another batch size in each, so their still poses differ in the last float32 bits (bounds
    of test_predict_sequence_equals_predict_loop_on_gpu), and each run's tracked poses are held against the twin on
    that run's own still poses at 16 float32 ulps. pose_video carries 'keypoints' (the reprojection of the tracked
    pose) and 'bbox'; reset() clears the device state; 'Kalman' still raises."""
    from spef_amd.inference import Inference
    from spef_amd.spe.spe_utils import SPEUtils
    if head == 'keypoints':
        g, model = _kp_model(golden)
        su = _kp_utils(g)
        x = _u8_frames(7, 61)
    else:
        from spef_amd.spe.keypoints import KeyPoints
        g = golden('keypoints.npz')

        class Cam:
            K, nu, nv = g['K'], float(g['nu']), float(g['nv'])
        su = SPEUtils(Cam, 'classification', 12, 3, False, 'classification', keypoints_path=KeyPoints(Cam, g['kp3d']))
        model = synthetic_state_dict(mobilenet_v2('ursonet', su.orientation.n_bins, su.position.n_bins), seed=1001)
        x = torch.from_numpy(np.random.Generator(np.random.PCG64(31)).random((7, 3, 64, 64), dtype=np.float32))
    seq = Inference(model, 'gpu_mi355x', su)
    try:
        whole = seq.predict_sequence(x, 'Tracker')
        state = seq.inference_engine.tracker(1).state().cpu().numpy()
        assert state[0, 0] == 1
        seq.reset()
        assert not seq.inference_engine.tracker(1).state().any().item()
        loop = [seq.predict(x[t:t + 1], 'Tracker') for t in range(7)]
        seq.reset()
        mix = seq.predict_sequence(x[:2], 'Tracker') + [seq.predict(x[2:3], 'Tracker')] + \
            seq.predict_sequence(x[3:], 'Tracker')
        for run in (whole, loop, mix):
            assert len(run) == 7
            # the tracked poses continue one track however the video was cut: the twin on this run's own still poses
            # (the forward ran at other batch sizes, so the runs' still poses differ in their last bits)
            twin = TK.PoseTrackerHost(1).step(np.stack([r[0]['ori'] for r in run]), np.stack([r[0]['pos'] for r in run]))
            mag = np.abs(twin['pos']).max()
            for t, ((s1, lat, v1), (s2, _, _)) in enumerate(zip(run, whole)):
                assert lat > 0 and set(s1) == set(s2) and ('keypoints' in s1 and 'bbox' in s1)
                assert set(v1) == {'ori', 'pos', 'mahalanobis', 'track_status', 'keypoints', 'bbox'}
                assert v1['track_status'] == 0
                assert abs(float(np.dot(s1['ori'], s2['ori']))) == pytest.approx(1.0, abs=1e-6)
                assert abs(float(np.dot(v1['ori'].astype(np.float64), twin['ori'][t]))) >= 1 - 1e-6
                assert np.abs(v1['pos'] - twin['pos'][t]).max() <= ULP16 * mag
                assert v1['mahalanobis'] == pytest.approx(twin['mahalanobis'][t], rel=1e-4, abs=1e-9)
                kp = su.keypoints.create_keypoints2d(v1['ori'], v1['pos'])
                np.testing.assert_array_equal(v1['keypoints'], kp)
            assert all(np.dot(a[2]['ori'], b[2]['ori']) > 0 for a, b in zip(run[1:], run[:-1]))
        assert whole[0][2]['mahalanobis'] == 0 and all(w[2]['mahalanobis'] > 0 for w in whole[1:])
        with pytest.raises(ValueError):
            seq.predict(x[:1], 'Kalman')
        with pytest.raises(ValueError):
            seq.predict_sequence(x[:2], 'Kalman')
    finally:
        seq.close()
