"""Scoring on the GPU (csrc/k_score.hip, spef_score_* in include/spef.h, Engine.scorer, StreamPipeline.submit(score=...),
SPEMi355x.predict_video(targets=, scorer=), tools.evaluation.evaluation_device) against the host twin
(spef_amd/score.py), which states the kernels' arithmetic in NumPy, and against the host evaluation() loop.

Rows and statistics are compared with the twin for equality (NaN == NaN): the kernels follow the twin's arithmetic
operation by operation. The one allowance is the one k_video states: an fp64 acos / atan2 within 1e-16 of a float32
rounding boundary may round the other way on the device; a row that trips it is reported by the assertion, not
tolerated."""
import ctypes as C

import numpy as np
import pytest
import torch

from spef_amd import score as SC

pytestmark = pytest.mark.gpu

TILE = SC.LDS_ROWS                       # rows the statistics kernel sorts in LDS
N_MAX = 2 * TILE + 116                   # above twice the tile: three global merge strides


# ---------------------------------------------------------------------------------------- shared, read-only
@pytest.fixture(scope='module')
def eng():
    from spef_amd.engine import Engine
    e = Engine(None, 'cuda:0')           # scoring needs neither weights nor decode tables
    yield e
    e.close()


@pytest.fixture(scope='module')
def poses():
    """N_MAX predicted / true poses, every 97th with a nonzero decode status, and the twin's rows and flags."""
    rng = np.random.Generator(np.random.PCG64(2024))
    n = N_MAX
    qt = rng.normal(size=(n, 4))
    qt = (qt / np.linalg.norm(qt, axis=1, keepdims=True)).astype(np.float32)
    tt = (rng.normal(size=(n, 3)) * [0.3, 0.3, 3.0] + [0, 0, 10]).astype(np.float32)
    qp = qt + (rng.normal(size=(n, 4)) * rng.uniform(0.001, 0.2, (n, 1))).astype(np.float32)
    qp = (qp / np.linalg.norm(qp, axis=1, keepdims=True)).astype(np.float32)
    qp[::3] *= -1
    tp = (tt + rng.normal(size=(n, 3)) * 0.1).astype(np.float32)
    status = np.zeros(n, np.int32)
    status[96::97] = 2
    rows, flags = SC.score_rows(qp, tp, qt, tt, status)
    for a in (qp, tp, qt, tt, status, rows, flags):
        a.setflags(write=False)
    return {'qp': qp, 'tp': tp, 'qt': qt, 'tt': tt, 'status': status, 'rows': rows, 'flags': flags}


def _dec(p, sl):
    return {'ori': torch.tensor(p['qp'][sl]).cuda(), 'pos': torch.tensor(p['tp'][sl]).cuda(),
            'status': torch.tensor(p['status'][sl]).cuda()}


def _tg(p, sl):
    return {'ori': p['qt'][sl], 'pos': p['tt'][sl]}


def _stats_equal(res, g, t, want, what=''):
    for k in SC.STAT_FIELDS:
        got = res[k][g, t]
        assert got == want[k] or (np.isnan(got) and np.isnan(want[k])), (what, k, float(got), want[k])


def _flag_cases():
    q = np.array([0.5, 0.5, 0.5, 0.5], np.float32)
    t = np.array([0.1, -0.2, 8.0], np.float32)
    qp = np.stack([-q, q * np.float32(1.02), q * np.float32(1.004), q, q, q])
    tp = np.stack([t, t, t, [0.1, np.nan, 8.0], t, t]).astype(np.float32)
    qt = np.stack([q] * 6)
    tt = np.stack([t, t, t, t, [0, 0, 0], t]).astype(np.float32)
    status = np.array([0, 0, 0, 0, 0, 4], np.int32)
    return qp, tp, qt, tt, status, np.array([0, 1, 0, 2, 4, 8], np.int32)


# ---------------------------------------------------------------------------------------- 1. rows
def test_rows_match_twin(golden, eng):
    g = golden('score.npz')
    fq, ft, fqt, ftt, fs, want_flags = _flag_cases()
    qp, tp = np.concatenate([g['q_pred'], fq]), np.concatenate([g['t_pred'], ft])
    qt, tt = np.concatenate([g['q_true'], fqt]), np.concatenate([g['t_true'], ftt])
    status = np.concatenate([np.zeros(64, np.int32), fs])
    rows, flags = SC.score_rows(qp, tp, qt, tt, status)
    np.testing.assert_array_equal(flags[64:], want_flags)
    n = 70
    sc = eng.scorer(1, 1, 128)
    out = sc.step(0, {'ori': torch.from_numpy(qp).cuda(), 'pos': torch.from_numpy(tp).cuda(),
                      'status': torch.from_numpy(status).cuda()}, {'ori': qt, 'pos': tt}, want_rows=True)
    got = out.cpu().numpy()
    log_rows, log_flags = sc.log(0, 0, 0, n)
    bad = np.nonzero(~((got == rows) | (np.isnan(got) & np.isnan(rows))).all(1))[0]
    assert bad.size == 0, [(int(i), got[i].tolist(), rows[i].tolist()) for i in bad]
    np.testing.assert_array_equal(log_rows, rows)
    np.testing.assert_array_equal(log_flags, flags)
    res = sc.result()
    _stats_equal(res, 0, 0, SC.score_stats(rows, flags))
    assert res['n'][0, 0] == 66 and res['n_bad'][0, 0] == 4 and res['flags'][0, 0] == 15
    # the fixture's own figures, at the host test's bounds
    only = eng.scorer(1, 1, 64)
    only.step(0, (torch.from_numpy(g['q_pred']).cuda(), torch.from_numpy(g['t_pred']).cuda()),
              (g['q_true'], g['t_true']))
    r = only.result()
    for k, tol in (('ori_score', 1e-5), ('ori_error', 1e-5), ('esa_score', 1e-5), ('pos_score', 1e-6),
                   ('pos_error', 1e-6)):
        assert abs(r[k][0, 0] / float(g[k]) - 1) < tol, k
    only.close()
    sc.close()


# ---------------------------------------------------------------------------------------- 2. statistics
@pytest.mark.parametrize('n,capacity', [(1, 1), (2, 2), (3, 3), (64, 64), (1800, 1800), (1800, 3 * TILE), (TILE, TILE),
                                        (TILE + 1, TILE + 1), (N_MAX, N_MAX)])
def test_statistics_match_twin(eng, poses, n, capacity):
    sl = slice(0, n)
    sc = eng.scorer(1, 1, capacity)
    sc.step(0, _dec(poses, sl), _tg(poses, sl))
    res = sc.result()
    want = SC.score_stats(poses['rows'][sl], poses['flags'][sl])
    print(n, {k: float(res[k][0, 0]) for k in ('n', 'n_bad', 'ori_median', 'ori_mad', 'pos_median', 'pos_max')})
    _stats_equal(res, 0, 0, want, f'n={n}')
    assert res['n'][0, 0] + res['n_bad'][0, 0] == n and res['n_bad'][0, 0] == n // 97
    again = sc.result()                                   # the log is only read: the same figures twice
    _stats_equal(again, 0, 0, want, f'n={n} again')
    sc.close()


def test_statistics_at_the_largest_capacity(eng):
    """2^20 rows in one group, the largest log there is: every merge stride of the global-memory sort, and slot
    offsets at their largest."""
    n = SC.MAX_CAPACITY
    rng = np.random.Generator(np.random.PCG64(77))
    qt = rng.normal(size=(n, 4)).astype(np.float32)
    qt /= np.linalg.norm(qt, axis=1, keepdims=True)
    qp = qt + rng.normal(size=(n, 4)).astype(np.float32) * np.float32(0.05)
    qp /= np.linalg.norm(qp, axis=1, keepdims=True)
    tt = (rng.normal(size=(n, 3)) + [0, 0, 10]).astype(np.float32)
    tp = tt + rng.normal(size=(n, 3)).astype(np.float32) * np.float32(0.1)
    tt[12345] = 0                                         # one flagged row
    rows, flags = SC.score_rows(qp, tp, qt, tt)
    sc = eng.scorer(1, 1, n)
    half = n // 2 + 3
    for sl in (slice(0, half), slice(half, n)):
        sc.step(0, (torch.from_numpy(qp[sl]).cuda(), torch.from_numpy(tp[sl]).cuda()), (qt[sl], tt[sl]))
    res = sc.result()
    _stats_equal(res, 0, 0, SC.score_stats(rows, flags), 'n=2^20')
    assert res['n'][0, 0] == n - 1 and res['n_bad'][0, 0] == 1 and res['flags'][0, 0] == SC.FLAG_ZERO_TARGET
    sc.close()


def test_empty_log_is_nan(eng):
    sc = eng.scorer(2, 1, 8)
    res = sc.result()
    for k in SC.STAT_FIELDS:
        if k in ('n', 'n_bad', 'n_dropped', 'flags'):
            assert (res[k] == 0).all(), k
        else:
            assert np.isnan(res[k]).all(), k
    sc.close()


# ---------------------------------------------------------------------------------------- 3. cutting and grouping
def test_cutting_into_steps_changes_nothing(eng, poses):
    n = 1800
    one = eng.scorer(1, 1, n)
    one.step(0, _dec(poses, slice(0, n)), _tg(poses, slice(0, n)))
    want = one.result()
    cut = eng.scorer(1, 1, n)
    a = 0
    for m in (7, 64, 1, n - 72):
        cut.step(0, _dec(poses, slice(a, a + m)), _tg(poses, slice(a, a + m)))
        a += m
    got = cut.result()
    for k in SC.STAT_FIELDS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    np.testing.assert_array_equal(cut.log(0, 0, 0, n)[0], one.log(0, 0, 0, n)[0])
    _stats_equal(got, 0, 0, SC.score_stats(poses['rows'][:n], poses['flags'][:n]))
    one.close()
    cut.close()


def test_groups_tracks_and_reset(eng, poses):
    S, T = 3, 5
    sl = slice(190, 190 + T * S)                          # row t * S + s belongs to group s; row 193 has a status
    sl2 = slice(400, 400 + T * S)
    both = eng.scorer(S, 2, 16)
    both.step(0, _dec(poses, sl), _tg(poses, sl), T)
    both.step(1, _dec(poses, sl2), _tg(poses, sl2), T)    # the second track gets other rows
    res = both.result()
    for s in range(S):
        idx = np.arange(T) * S + s
        single = eng.scorer(1, 1, 16)
        part = {k: poses[k][sl][idx] for k in ('qp', 'tp', 'qt', 'tt', 'status')}
        single.step(0, _dec(part, slice(None)), _tg(part, slice(None)))
        r1 = single.result()
        single.close()
        for k in SC.STAT_FIELDS:
            assert r1[k][0, 0] == res[k][s, 0] or np.isnan(r1[k][0, 0]) and np.isnan(res[k][s, 0]), (s, k)
        _stats_equal(res, s, 0, SC.score_stats(poses['rows'][sl][idx], poses['flags'][sl][idx]), f'group {s}')
        _stats_equal(res, s, 1, SC.score_stats(poses['rows'][sl2][idx], poses['flags'][sl2][idx]), f'track 1 {s}')
    both.reset(1)                                         # one group only, both of its tracks
    res2 = both.result()
    for k in SC.STAT_FIELDS:
        for s in (0, 2):
            np.testing.assert_array_equal(res2[k][s], res[k][s], err_msg=k)
    assert (res2['n'][1] == 0).all() and np.isnan(res2['ori_median'][1]).all()
    both.step(0, _dec(poses, sl), _tg(poses, sl), T)      # group 1 starts over, the others go on
    res3 = both.result()
    assert res3['n'][1, 0] + res3['n_bad'][1, 0] == T and res3['n'][0, 0] + res3['n_bad'][0, 0] == 2 * T
    _stats_equal(res3, 1, 0, SC.score_stats(poses['rows'][sl][np.arange(T) * S + 1],
                                            poses['flags'][sl][np.arange(T) * S + 1]))
    both.reset()
    assert (both.result()['n'] == 0).all()
    both.close()


# ---------------------------------------------------------------------------------------- 4. capacity
def test_capacity_drops_and_counts(eng, poses):
    sc = eng.scorer(1, 1, 100)
    for a, b in ((0, 60), (60, 130)):                     # the second step crosses the capacity
        sc.step(0, _dec(poses, slice(a, b)), _tg(poses, slice(a, b)))
    res = sc.result()
    assert res['n'][0, 0] + res['n_bad'][0, 0] == 100 and res['n_dropped'][0, 0] == 30
    _stats_equal(res, 0, 0, SC.score_stats(poses['rows'][:100], poses['flags'][:100], n_dropped=30))
    sc.step(0, _dec(poses, slice(130, 140)), _tg(poses, slice(130, 140)))      # a full log: every row dropped
    res = sc.result()
    assert res['n_dropped'][0, 0] == 40
    _stats_equal(res, 0, 0, SC.score_stats(poses['rows'][:100], poses['flags'][:100], n_dropped=40))
    sc.close()


# ---------------------------------------------------------------------------------------- 5. argument errors
def test_argument_errors_enqueue_nothing(eng, poses):
    from spef_amd import _lib as L
    lib = eng.lib
    h = C.c_void_p()
    for g, t, cap in ((0, 1, 8), (1, 0, 8), (1, 1, 0), (-1, 1, 8), (1, 1, (1 << 20) + 1)):
        assert lib.spef_score_create(eng.ctx, g, t, cap, C.byref(h)) == L.ERR_ARG
    assert h.value is None
    sc = eng.scorer(2, 2, 16)
    sl = slice(0, 4)
    sc.step(0, _dec(poses, sl), _tg(poses, sl))
    before = sc.result()
    d, (qt, pt) = _dec(poses, sl), sc.targets(_tg(poses, sl))
    rows = torch.full((4, 5), -7.0, device='cuda:0')
    torch.cuda.synchronize()
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())

    def call(track, T, S, quat=d['ori']):
        return lib.spef_score_step(sc.handle, track, p(quat), p(d['pos']), p(d['status']), p(qt), p(pt), T, S,
                                   p(rows), None)
    assert call(0, 2, 3) == L.ERR_ARG                     # S != n_groups
    assert call(0, 4, 1) == L.ERR_ARG
    assert call(0, 0, 2) == L.ERR_ARG                     # T < 1
    assert call(0, -1, 2) == L.ERR_ARG
    assert call(2, 2, 2) == L.ERR_ARG                     # track out of range
    assert call(-1, 2, 2) == L.ERR_ARG
    assert call(0, 2, 2, None) == L.ERR_ARG               # null input
    assert lib.spef_score_reset(sc.handle, 2, None) == L.ERR_ARG
    assert lib.spef_score_finalize(sc.handle, None, None) == L.ERR_ARG
    with pytest.raises(AssertionError):
        sc.step(0, _dec(poses, slice(0, 3)), _tg(poses, slice(0, 3)))          # 3 rows, 2 groups
    torch.cuda.synchronize()
    assert bool((rows == -7).all())                       # nothing ran
    after = sc.result()
    for k in SC.STAT_FIELDS:
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)
    sc.close()


def test_step_graph_capture(eng, poses):
    """A step captured on a stream and replayed three times logs the same rows as three eager steps: the slot
    indices come from device memory."""
    n = 50
    sl = slice(0, n)
    d, tg = _dec(poses, sl), None
    sc = eng.scorer(1, 1, 4 * n)
    tg = sc.targets(_tg(poses, sl))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        sc.step(0, d, tg)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    res = sc.result()
    want = SC.score_stats(np.tile(poses['rows'][sl], (3, 1)), np.tile(poses['flags'][sl], 3))
    _stats_equal(res, 0, 0, want)
    del g
    sc.close()


# ---------------------------------------------------------------------------------------- 6. end to end
@pytest.fixture(scope='module')
def model():
    from spef_amd import blob as Bl
    from spef_amd.arch import mobilenet_v2
    from spef_amd.spe.spe_utils import SPEUtils
    from spef_amd.weights import synthetic_state_dict
    su = SPEUtils(None, 'classification', 12, 3, False, 'classification')
    sd = synthetic_state_dict(mobilenet_v2('ursonet', su.orientation.n_bins, su.position.n_bins), seed=1001)
    return su, Bl.pack(sd, dtype='fp16')


def _frames(count, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(rng.random((count, 3, 64, 64), dtype=np.float32))


def _targets(count, first=0):
    from spef_amd.data.synthetic import synth_poses
    ori, pos = synth_poses(count, first)
    return {'ori': ori, 'pos': pos}


@pytest.mark.parametrize('graphs', [False, True])
def test_pipeline_scores_what_it_returns(model, graphs):
    from spef_amd import _lib as L
    from spef_amd.pipeline import StreamPipeline
    su, blob = model
    B, K = 4, 6
    x = _frames(B * K, 41)
    tg = _targets(B * K)
    pipe = StreamPipeline(blob, 'cuda:0', depth=3, ori_bins=su.orientation.histogram, pos_grid=su.position.histogram)
    pipe.use_graphs(graphs)
    sc = pipe.engine.scorer(1, 1, B * K)
    xs = [x[k * B:(k + 1) * B].cuda() for k in range(K)]
    outs = []
    for k, f in enumerate(xs):
        t = {n: v[k * B:(k + 1) * B] for n, v in tg.items()}
        d = pipe.submit(f, L.CLASSIFICATION, L.CLASSIFICATION, score=(sc, t))
        d['event'].synchronize()                         # with graphs a slot's outputs are overwritten three submits on
        outs.append({n: d[n].cpu().numpy() for n in ('ori', 'pos', 'status')})
    res = sc.result()
    rows, flags = SC.score_rows(np.concatenate([o['ori'] for o in outs]), np.concatenate([o['pos'] for o in outs]),
                                tg['ori'], tg['pos'], np.concatenate([o['status'] for o in outs]))
    assert not flags.any()
    _stats_equal(res, 0, 0, SC.score_stats(rows, flags))
    np.testing.assert_array_equal(sc.log(0, 0, 0, B * K)[0], rows)
    sc.close()
    pipe.close()


def test_pipeline_scoring_does_not_wait_per_batch(model):
    """The same submits without a synchronisation in between (the way evaluation_device drives them) give the same
    figures: the steps are ordered by events, not by the host."""
    from spef_amd import _lib as L
    from spef_amd.pipeline import StreamPipeline
    su, blob = model
    B, K = 4, 6
    x = _frames(B * K, 41)
    tg = _targets(B * K)
    pipe = StreamPipeline(blob, 'cuda:0', depth=3, ori_bins=su.orientation.histogram, pos_grid=su.position.histogram)
    sc = pipe.engine.scorer(1, 1, B * K)
    xs = [x[k * B:(k + 1) * B].cuda() for k in range(K)]
    outs = [pipe.submit(f, L.CLASSIFICATION, L.CLASSIFICATION,
                        score=(sc, {n: v[k * B:(k + 1) * B] for n, v in tg.items()})) for k, f in enumerate(xs)]
    res = sc.result()
    pipe.synchronize()
    rows, flags = SC.score_rows(np.concatenate([o['ori'].cpu().numpy() for o in outs]),
                                np.concatenate([o['pos'].cpu().numpy() for o in outs]), tg['ori'], tg['pos'])
    _stats_equal(res, 0, 0, SC.score_stats(rows, flags))
    sc.close()
    pipe.close()


def test_predict_video_scores_both_tracks(model):
    from spef_amd.spe_mi355x import SPEMi355x
    su, blob = model
    S, T = 2, 3
    x = _frames(T * S, 42)
    tg = _targets(T * S)
    spe = SPEMi355x(blob, 'cuda:0', su)
    sc = spe.engine.scorer(S, 2, 8)
    still, video, _ = spe.predict_video(x, n_streams=S, targets=tg, scorer=sc)
    res = sc.result()
    for track, pose in ((0, still), (1, video)):
        rows, flags = SC.score_rows(pose['ori'], pose['pos'], tg['ori'], tg['pos'])
        for s in range(S):
            idx = np.arange(T) * S + s
            _stats_equal(res, s, track, SC.score_stats(rows[idx], flags[idx]), f'track {track} stream {s}')
    assert (res['n'] == T).all()
    with pytest.raises(AssertionError):
        spe.predict_video(x, n_streams=S, targets=tg, scorer=spe.engine.scorer(S, 1, 8))   # one track only
    sc.close()
    spe.close()


def test_evaluation_device_matches_evaluation(model):
    """A five-batch loader with a last batch of 1. Tolerances: scores and errors rtol 1e-6 -- evaluation()'s side: its
    per-batch float32 means (get_score on float32 arrays) weighted by batch size carry ~1e-7 each, the bound
    test_evaluation_loop_matches_get_score uses; std 1e-6 -- evaluation()'s side again: np.std of a float32 list is
    taken in float32 (~1e-7), the device's is fp64. Median absolute deviation: both sides take exact order statistics,
    so they differ only through the float32 rows. If no row differs by more than d, the median moves by at most d,
    every |x - median| by at most 2 d and so does their median: the bound is 2 d, with d from the number formats --
    the dot product (four float32 products summed in float32 on the host, in fp64 on the device) is off by at most
    8 * 2^-24 on either side, which acos turns into 2 * 8 * 2^-24 / sqrt(1 - dot^2) rad, plus 4 float32 roundings of
    the angle; the position error (three squares, a sum, a square root) by at most 8 * 2^-24 relative."""
    from spef_amd.spe_mi355x import SPEMi355x
    from spef_amd.tools.evaluation import evaluation, evaluation_device
    su, blob = model
    B = 4
    x = _frames(4 * B + 1, 43)
    tg = _targets(4 * B + 1)
    batches = [({'torch': x[a:a + B]}, {k: torch.from_numpy(v[a:a + B]) for k, v in tg.items()})
               for a in range(0, 4 * B + 1, B)]
    assert len(batches) == 5 and batches[-1][0]['torch'].shape[0] == 1
    spe = SPEMi355x(blob, 'cuda:0', su)
    s_host, e_host = evaluation(spe, {'valid': batches}, su, ('valid',))
    s_dev, e_dev = evaluation_device(spe, {'valid': batches}, su, ('valid',))
    assert set(s_dev['valid']) == set(s_host['valid']) and set(e_dev['valid']) == set(e_host['valid'])
    for k in ('ori', 'pos', 'esa'):
        print('score', k, s_dev['valid'][k][0], s_host['valid'][k][0])
        assert s_dev['valid'][k][0] == pytest.approx(s_host['valid'][k][0], rel=1e-6)
    for k in ('ori', 'pos', 'ori_std', 'pos_std'):
        print('error', k, e_dev['valid'][k][0], e_host['valid'][k][0])
        assert e_dev['valid'][k][0] == pytest.approx(e_host['valid'][k][0], rel=1e-6)
    pred = [spe.predict(b[0]['torch'])[0] for b in batches]            # the poses evaluation() scored
    q = np.concatenate([p['ori'] for p in pred]).astype(np.float64)
    t = np.concatenate([p['pos'] for p in pred]).astype(np.float64)
    dot = np.minimum(np.abs(np.sum(q * tg['ori'], axis=1)), 1.0)
    eps = 8 * 2.0 ** -24
    d_ori = float(np.max(np.rad2deg(2 * eps / np.sqrt(1 - dot * dot)) + 4 * 2.0 ** -24 * 180.0))
    d_pos = eps * float(np.linalg.norm(t - tg['pos'], axis=1).max())
    for k, d in (('ori_mad', d_ori), ('pos_mad', d_pos)):
        print('error', k, e_dev['valid'][k][0], e_host['valid'][k][0], 'bound', 2 * d)
        assert abs(e_dev['valid'][k][0] - e_host['valid'][k][0]) <= 2 * d
    spe.close()


def test_deploy_tool_device_eval(tmp_path):
    """deploy_mi355x --device-eval writes the same records through evaluation_device."""
    import json
    import os
    from spef_amd.tools.build_mi355x import main as build
    from spef_amd.tools.deploy_mi355x import main as deploy
    out = str(tmp_path / 'b')
    assert build(['--synthetic', '--out', out]) == 0
    assert deploy(['--build', out, '--synthetic', '2', '--num-predict', '2', '--device-eval']) == 0
    sc = json.load(open(os.path.join(out, 'on_board', 'score.json')))
    assert set(sc['score']['synthetic']) == {'ori', 'pos', 'esa'}
    assert set(sc['error']['synthetic']) == {'ori', 'pos', 'ori_std', 'pos_std', 'ori_mad', 'pos_mad'}
    for rec in (sc['score']['synthetic'], sc['error']['synthetic']):
        assert all(len(v) == 1 and np.isfinite(v[0]) and v[0] > 0 for v in rec.values()), rec
    assert sc['score']['synthetic']['esa'][0] == sc['score']['synthetic']['ori'][0] + sc['score']['synthetic']['pos'][0]
