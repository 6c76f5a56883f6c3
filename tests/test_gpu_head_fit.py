"""GPU: the head-fit path (csrc/k_headfit.hip, ``spef_headfit_*``, ``spef_features``, ``spef_encode_targets``) against its
NumPy twin (spef_amd/solver/head_fit.py), stage by stage: every stage is checked on the device's own output of the stage
before, so each tolerance is the rounding of that stage alone (eps = float32 machine epsilon, 2^-23):

  logits    the standard dot-product bound (K + 4) eps (|X| |W|^T + |b|) against the float64 product
  G         4 eps (p + t) scale / B against the twin at the device's logits (a regression head: 4 eps |G|)
  loss      4 eps |loss| + 4 eps mean_b sum_i t |log p| per head
  grad_out  (B + 4) eps |G|^T |X| against the float64 product of the device's G and X (or the dropout copy)
  update    8 eps (|w| + |update|) against the twin's float32 optimizer fed the device's grad_out; the state likewise

Shapes: K in {16, 48, 1280} (its minimum, a partial 64-column wave, several 256-column workgroups), heads (37, 3), (37, 27),
(5, 8) -- 16-row tiles that hold both heads and padding rows -- and (1728, 1000); B in {1, 5, 17, 65} (not multiples of the
MFMA's 4, more than one 16-image group of the forward).

Trajectory yardstick (30 SGD steps; the distances printed by test_trajectory, MI355X): see DESIGN.md section 3."""
import numpy as np
import pytest
import torch

from oracle import decode_ref as D
from spef_amd import _lib as L
from spef_amd import blob as Bl
from spef_amd.arch import mobilenet_v2
from spef_amd.data.synthetic import synth_frames, synth_poses
from spef_amd.solver import head_fit as HF
from spef_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
TINY = 2.0 ** -149          # the float32 subnormal spacing: no float32 result is closer to its exact value than half of it
OPTS = {'sgd': dict(momentum=0.9, weight_decay=1e-4, lr=0.05), 'adam': dict(weight_decay=1e-4, lr=0.01)}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _h(t):
    return t.cpu().numpy()


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope='module')
def engine():
    from spef_amd.engine import Engine
    e = Engine(None, 'cuda:0')
    yield e
    e.close()


def _soft(rng, B, n):
    t = rng.random((B, n)) ** 4
    t[:, ::5] = 0.0
    if n <= 5:
        t[:, 1] += 0.1
    return (t / t.sum(axis=1, keepdims=True)).astype(np.float32)


def _data(K, n_ori, n_pos, B, seed, pos_mode='classification'):
    rng = np.random.Generator(np.random.PCG64([seed, K, n_ori, n_pos, B]))
    # |x|^2 about 1 whatever K, so that the same learning rates are stable at every shape (a diverging fit drives G into
    # float32 subnormals, where no relative bound holds); logits of order 1
    X = (rng.standard_normal((B, K)) / np.sqrt(K)).astype(np.float32)
    W = (rng.standard_normal((n_ori + n_pos, K)) * 0.7).astype(np.float32)
    b = (rng.standard_normal(n_ori + n_pos) * 0.1).astype(np.float32)
    to = _soft(rng, B, n_ori)
    tp = (rng.standard_normal((B, 3)) * 2).astype(np.float32) if pos_mode == 'regression' else _soft(rng, B, n_pos)
    return X, W, b, to, tp


def _check_step(tr, X, Xo, to, tp, W0, b0, st0, out, opt, prm, step, pos_mode, beta, norm):
    """One step's stages. Xo = what the orientation rows contracted with. -> the new (W, b, state) on the host."""
    B, K = X.shape
    n_ori, n = tr.n_ori, tr.n_ori + tr.n_pos
    z = _h(out['logits'])
    # --- logits
    ref = np.concatenate([HF.forward(Xo, W0[:n_ori], b0[:n_ori]), HF.forward(X, W0[n_ori:], b0[n_ori:])], axis=1)
    bound = np.concatenate([np.abs(Xo).astype(np.float64) @ np.abs(W0[:n_ori]).astype(np.float64).T,
                            np.abs(X).astype(np.float64) @ np.abs(W0[n_ori:]).astype(np.float64).T], axis=1) + np.abs(b0)
    r = np.max(np.abs(z - ref) / ((K + 4) * EPS * bound))
    print(f'step {step}: logits {r:.3f} of the dot bound')
    assert r <= 1.0
    # --- G and loss at the device's logits
    (tot, lo, lp), G64 = HF.loss_and_g(z[:, :n_ori], to, z[:, n_ori:], tp, beta, pos_mode, norm)
    G = _h(tr.last_g(B))
    if pos_mode == 'regression':
        p, logp = HF.log_softmax_parts(z[:, :n_ori])
        gb = np.concatenate([(p + to) * (beta / B), np.abs(G64[:, n_ori:])], axis=1)
        lb = 4 * EPS * (abs(tot) + beta * float(np.mean(np.sum(to * np.abs(logp), axis=1))))
    else:
        gb = HF.g_bound(z[:, :n_ori], to, z[:, n_ori:], tp, beta)
        logp = [HF.log_softmax_parts(z[:, :n_ori])[1], HF.log_softmax_parts(z[:, n_ori:])[1]]
        lb = 4 * EPS * (abs(tot) + beta * float(np.mean(np.sum(to * np.abs(logp[0]), axis=1))) +
                        float(np.mean(np.sum(tp * np.abs(logp[1]), axis=1))))
    r = np.max(np.abs(G - G64) / np.maximum(4 * EPS * gb, 1e-300))
    loss = _h(out['loss']).astype(np.float64)
    print(f'step {step}: G {r:.3f} of 4 eps (p + t) scale / B; loss {loss[0]:.6f} off by {abs(loss[0] - tot):.2e} '
          f'(bound {lb:.2e})')
    assert r <= 1.0
    assert abs(loss[0] - tot) <= lb and abs(loss[1] - lo) <= lb and abs(loss[2] - lp) <= lb
    # --- gradients from the device's G
    gw, gbias = _h(out['grad_w']), _h(out['grad_b'])
    dW, db = HF.gradients(G, Xo, X, n_ori)
    aG = np.abs(G).astype(np.float64)
    bw = np.concatenate([aG[:, :n_ori].T @ np.abs(Xo).astype(np.float64), aG[:, n_ori:].T @ np.abs(X).astype(np.float64)])
    r = np.max(np.abs(gw[:n] - dW) / np.maximum((B + 4) * EPS * bw, TINY))
    rb = np.max(np.abs(gbias[:n] - db) / np.maximum((B + 4) * EPS * aG.sum(axis=0), TINY))
    print(f'step {step}: grad_w {r:.3f}, grad_b {rb:.3f} of the dot bound')
    assert r <= 1.0 and rb <= 1.0
    assert not gw[n:].any() and not gbias[n:].any()          # padding rows: exactly zero
    # --- optimizer from the device's gradient
    f32 = np.float32
    if opt == 'sgd':
        Wt, s0 = HF.sgd_step(W0, st0[0], gw[:n], f32(prm['lr']), prm['momentum'], prm['weight_decay'])
        bt, s1 = HF.sgd_step(b0, st0[1], gbias[:n], f32(prm['lr']), prm['momentum'], prm['weight_decay'])
        st_t = (s0, s1)
    else:
        Wt, s0, s2 = HF.adam_step(W0, st0[0], st0[2], gw[:n], f32(prm['lr']), step, weight_decay=prm['weight_decay'])
        bt, s1, s3 = HF.adam_step(b0, st0[1], st0[3], gbias[:n], f32(prm['lr']), step, weight_decay=prm['weight_decay'])
        st_t = (s0, s1, s2, s3)
    W1, b1 = (_h(t) for t in tr.weights())
    st1 = tuple(_h(t) for t in tr.state())
    for got, want, old, what in [(W1, Wt, W0, 'W'), (b1, bt, b0, 'bias')] + \
            [(g, w, o, f'state {i}') for i, (g, w, o) in enumerate(zip(st1, st_t, st0))]:
        tol = 8 * EPS * (np.abs(want) + np.abs(want - old))
        bad = np.abs(got.astype(np.float64) - want) > tol
        print(f'step {step}: {what} differs from the float32 twin in {int(np.count_nonzero(got != want))} of {got.size}')
        assert not bad.any(), what
    return W1, b1, st1


SHAPES = [(K, h, B) for K in (16, 48, 1280) for h in ((37, 3), (37, 27), (5, 8), (1728, 1000)) for B in (1, 5, 17, 65)]


@pytest.mark.parametrize('opt', ['sgd', 'adam'])
@pytest.mark.parametrize('K,heads,B', SHAPES, ids=[f'K{K}-{h[0]}+{h[1]}-B{B}' for K, h, B in SHAPES])
def test_step_stages(engine, K, heads, B, opt):
    n_ori, n_pos = heads
    pos_mode = 'regression' if n_pos == 3 else 'classification'
    beta, norm = (0.5, opt == 'sgd') if n_pos == 3 else (1.0, False)
    X, W, b, to, tp = _data(K, n_ori, n_pos, B, 1, pos_mode)
    prm = OPTS[opt]
    tr = engine.head_trainer(K, n_ori, n_pos, optimizer=opt, pos_mode=pos_mode, beta=beta, norm_distance=norm,
                             Bmax=max(B, 8), **prm)
    try:
        tr.set_weights(W, b)
        Xd, tod, tpd = _d(X), _d(to), _d(tp)
        st = tuple(np.zeros_like(W if i % 2 == 0 else b) for i in range(4 if opt == 'adam' else 2))
        for step in (1, 2, 3):
            out = tr.step(Xd, tod, tpd, want_logits=True, want_grad=True)
            W, b, st = _check_step(tr, X, X, to, tp, W, b, st, out, opt, prm, step, pos_mode, beta, norm)
        _check_padding(tr, opt, W, b)
    finally:
        tr.close()


def _check_padding(tr, opt, W, b):
    """After the steps (weight decay on): the padding rows of W, bias and every state tensor are zero bit for bit, and the
    rows before them are what ``weights`` returns."""
    n = tr.n_ori + tr.n_pos
    Np = (n + 15) // 16 * 16
    for which in ('W', 'bias', 'W_s1', 'bias_s1') + (('W_s2', 'bias_s2') if opt == 'adam' else ()):
        a = _h(tr.raw(which))
        assert a.shape[0] == Np
        assert not _bits(a[n:]).any(), which
    assert np.array_equal(_bits(_h(tr.raw('W'))[:n]), _bits(W)) and np.array_equal(_bits(_h(tr.raw('bias'))[:n]), _bits(b))
    if opt == 'sgd':
        with pytest.raises(AssertionError):
            tr.raw('W_s2')
    with pytest.raises(AssertionError):
        tr.raw('Xd')                                                   # dropout is off


@pytest.mark.parametrize('p,opt,n_ori', [(0.2, 'sgd', 37), (0.5, 'adam', 37), (0.2, 'adam', 32), (0.5, 'sgd', 32)])
def test_dropout(engine, p, opt, n_ori):
    """Dropout on the orientation rows only: with a 16-row tile that holds both heads (37 % 16 != 0) and with the heads
    split at a tile boundary (32). The device's dropout copy of X is read back: it is the twin's bit for bit, and its
    realised keep rate over B * K = 4352 elements is within 5 binomial standard deviations of 1 - p."""
    K, n_pos, B, seed = 256, 27, 17, 12345
    X, W, b, to, tp = _data(K, n_ori, n_pos, B, 2)
    assert np.all(X != 0)
    prm = OPTS[opt]
    tr = engine.head_trainer(K, n_ori, n_pos, optimizer=opt, dropout_p=p, seed=seed, Bmax=B + 3, **prm)
    plain = engine.head_trainer(K, n_ori, n_pos, optimizer=opt, Bmax=B, **prm)
    try:
        Xd, tod, tpd = _d(X), _d(to), _d(tp)
        st = tuple(np.zeros_like(W if i % 2 == 0 else b) for i in range(4 if opt == 'adam' else 2))
        tr.set_weights(W, b)
        for step in (1, 2, 3):
            plain.set_weights(W, b)
            ev = _h(tr.evaluate(Xd, tod, tpd, want_logits=True)['logits'])     # train = 0 ignores dropout
            assert np.array_equal(_bits(ev), _bits(_h(plain.evaluate(Xd, tod, tpd, want_logits=True)['logits'])))
            out = tr.step(Xd, tod, tpd, want_logits=True, want_grad=True)
            Xo = _h(tr.raw('Xd'))[:B]
            kept = Xo != 0
            rate = kept.mean()
            print(f'step {step}: kept {rate:.4f} of {kept.size}, expected {1 - p}')
            assert abs(rate - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / kept.size)
            keep = HF.dropout_keep(seed, step - 1, B, K, p)
            assert np.array_equal(kept, keep)
            assert np.array_equal(_bits(Xo), _bits(HF.dropout_apply(X, keep, p)))
            z = _h(out['logits'])
            assert np.array_equal(_bits(z[:, n_ori:]), _bits(ev[:, n_ori:]))     # the position rows read X itself
            assert not np.array_equal(z[:, :n_ori], ev[:, :n_ori])
            W, b, st = _check_step(tr, X, Xo, to, tp, W, b, st, out, opt, prm, step, 'classification', 1.0, False)
    finally:
        tr.close()
        plain.close()


def test_deterministic_and_graph_replay(engine):
    """The same 10 steps twice and once as 10 replays of one captured step: bit-identical weights (Adam and dropout on, so
    the device-side step counter drives both the bias corrections and the mask)."""
    K, n_ori, n_pos, B = 48, 37, 27, 17
    X, W, b, to, tp = _data(K, n_ori, n_pos, B, 3)
    tr = engine.head_trainer(K, n_ori, n_pos, optimizer='adam', dropout_p=0.2, seed=7, Bmax=B, weight_decay=1e-4, lr=0.01)
    try:
        Xd, tod, tpd = _d(X), _d(to), _d(tp)
        runs = []
        for _ in range(2):
            tr.set_weights(W, b)
            tr.reset_state()
            for _ in range(10):
                tr.step(Xd, tod, tpd)
            runs.append(_h(tr.weights()[0]))
        assert np.array_equal(_bits(runs[0]), _bits(runs[1]))
        assert not np.array_equal(runs[0], W)
        tr.set_weights(W, b)
        tr.reset_state()
        loss = torch.empty(3, dtype=torch.float32, device='cuda')
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            tr.step(Xd, tod, tpd, loss=loss)
        tr.set_weights(W, b)      # whatever the capture did or did not run, start again
        tr.reset_state()
        for _ in range(10):
            graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(_h(tr.weights()[0])), _bits(runs[0]))
        del graph
    finally:
        tr.close()


def test_regression_at_the_target_is_zero_not_nan(engine):
    K, n_ori, B = 16, 5, 5
    X, W, b, to, _ = _data(K, n_ori, 3, B, 4, 'regression')
    W[n_ori:] = 0.0
    b[n_ori:] = [1.5, -2.0, 12.0]
    tp = np.tile(b[n_ori:], (B, 1)).astype(np.float32)
    for norm in (False, True):
        tr = engine.head_trainer(K, n_ori, 3, optimizer='sgd', pos_mode='regression', norm_distance=norm, Bmax=B,
                                 momentum=0.9, lr=0.05)
        try:
            tr.set_weights(W, b)
            out = tr.step(_d(X), _d(to), _d(tp), want_grad=True)
            loss, gw, gb = _h(out['loss']), _h(out['grad_w']), _h(out['grad_b'])
            assert loss[2] == 0.0 and np.isfinite(loss).all() and loss[0] == np.float32(loss[1])
            assert not gw[n_ori:].any() and not gb[n_ori:].any() and np.isfinite(gw).all()
            W1, b1 = (_h(t) for t in tr.weights())
            assert np.array_equal(W1[n_ori:], W[n_ori:]) and np.array_equal(b1[n_ori:], b[n_ori:])
        finally:
            tr.close()


def test_argument_checks(engine):
    with pytest.raises(AssertionError):
        engine.head_trainer(24, 5, 8)                                  # K % 16
    with pytest.raises(AssertionError):
        engine.head_trainer(16, 5, 8, ori_mode='regression')           # out of scope
    with pytest.raises(AssertionError):
        engine.head_trainer(16, 5, 8, pos_mode='regression')           # regression has 3 outputs
    tr = engine.head_trainer(16, 5, 8, Bmax=4)
    try:
        X, W, b, to, tp = _data(16, 5, 8, 5, 5)
        with pytest.raises(AssertionError):
            tr.step(_d(X), _d(to), _d(tp))                             # B > Bmax
        with pytest.raises(L.SpefError):
            tr.load_model()                                            # no model in this engine: SPEF_ERR_STATE
    finally:
        tr.close()


# ------------------------------------------------------------------------------------------------------ trajectory
def _torch_run(X, W, b, to, tp, n_ori, steps, lr, momentum, wd):
    x, t_o, t_p = (torch.from_numpy(a) for a in (X, to, tp))
    lin = torch.nn.Linear(X.shape[1], W.shape[0])
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(W))
        lin.bias.copy_(torch.from_numpy(b))
    opt = torch.optim.SGD(lin.parameters(), lr=lr, momentum=momentum, weight_decay=wd)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        z = lin(x)
        po, pp = torch.softmax(z[:, :n_ori], dim=1), torch.softmax(z[:, n_ori:], dim=1)
        loss = torch.mean(torch.sum(-(t_o * torch.log(po)), dim=1)) + torch.mean(torch.sum(-(t_p * torch.log(pp)), dim=1))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return np.array(losses), lin.weight.detach().numpy().copy()


@pytest.mark.parametrize('K,n_ori,n_pos,B', [(48, 37, 27, 5), (1280, 1728, 1000, 64)])
def test_trajectory(engine, K, n_ori, n_pos, B):
    """30 SGD steps against the float64 twin; the yardstick is a float32 torch CPU run of the same steps (the reference's
    own path), and the device may be 8 times as far from the twin as torch is."""
    steps, lr, momentum, wd = 30, 0.5, 0.9, 1e-4
    X, W, b, to, tp = _data(K, n_ori, n_pos, B, 6)
    tw = HF.HeadFitTwin(K, n_ori, n_pos, optimizer='sgd', momentum=momentum, weight_decay=wd)
    tw.set_weights(W, b)
    l64 = np.array([tw.step(X, to, tp, lr)[0] for _ in range(steps)])
    lt, Wt = _torch_run(X, W, b, to, tp, n_ori, steps, lr, momentum, wd)
    tr = engine.head_trainer(K, n_ori, n_pos, optimizer='sgd', momentum=momentum, weight_decay=wd, lr=lr, Bmax=B)
    try:
        tr.set_weights(W, b)
        Xd, tod, tpd = _d(X), _d(to), _d(tp)
        losses = torch.empty((steps, 3), dtype=torch.float32, device='cuda')
        for s in range(steps):
            tr.step(Xd, tod, tpd, loss=losses[s])
        ld, Wd = _h(losses)[:, 0].astype(np.float64), _h(tr.weights()[0])
    finally:
        tr.close()
    dl_t, dl_d = np.max(np.abs(lt - l64)), np.max(np.abs(ld - l64))
    dw_t, dw_d = np.max(np.abs(Wt - tw.W)), np.max(np.abs(Wd - tw.W))
    print(f'K {K}, {n_ori} + {n_pos}, B {B}: loss {l64[0]:.4f} -> {l64[-1]:.4f}; max |d loss| torch {dl_t:.3e} device '
          f'{dl_d:.3e}; max |d W| torch {dw_t:.3e} device {dw_d:.3e}')
    assert l64[-1] < l64[0]
    assert dl_d <= 8 * dl_t and dw_d <= 8 * dw_t


# ------------------------------------------------------------------------------------------------------ encode
@pytest.fixture(scope='module')
def tables(golden):
    def quats(n):
        h = np.random.Generator(np.random.PCG64(n)).standard_normal((n, 4))
        return h / np.linalg.norm(h, axis=1, keepdims=True)
    return {1728: golden('decode_ori.npz')['hist'], 1232: D.orientation_histogram(12, True)[0], 257: quats(257),
            5: quats(5), 1000: golden('decode_pos.npz')['grid'], 8: D.position_histogram(2)}


def test_encode_matches_reference(golden, tables):
    from spef_amd.engine import Engine
    g, gp, red = golden('encode.npz'), golden('decode_pos.npz'), golden('decode_ori.npz')['redundant']
    e = Engine(None, 'cuda:0')
    try:
        e.set_decode_tables(tables[1728], tables[1000])
        assert g['q'].shape[0] == 16 and gp['enc_t'].shape[0] == 32
        o = e.encode_targets(quat=g['q'], mask=red)
        np.testing.assert_allclose(_h(o['ori_soft']), g['enc'], rtol=1e-6, atol=1e-9)
        t = e.encode_targets(pos=gp['enc_t'])
        np.testing.assert_allclose(_h(t['pos_soft']), gp['enc'], rtol=1e-6, atol=1e-9)
        assert not _h(o['status']).any() and not _h(t['status']).any()
    finally:
        e.close()


@pytest.mark.parametrize('B', [1, 3, 65])
@pytest.mark.parametrize('n_ori,n_pos', [(1232, 1000), (257, 8), (5, 8)])
def test_encode_matches_twin(tables, n_ori, n_pos, B):
    from spef_amd.engine import Engine
    rng = np.random.Generator(np.random.PCG64([n_ori, B]))
    q = rng.standard_normal((B, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = rng.uniform(-1, 1, (B, 3)) * np.array([10.0, 8.0, 15.0]) + np.array([0.0, 0.0, 19.0])
    # a variance wide enough for the sparse random tables to see every pose (the 5-bin table would underflow to 0 / 0)
    ov, pv = (HF.soft_variance(3, 12) if n_ori > 1000 else 0.05), HF.soft_variance(100, 10)
    e = Engine(None, 'cuda:0')
    try:
        e.set_decode_tables(tables[n_ori], tables[n_pos])
        o = e.encode_targets(q, t, ori_var=ov, pos_var=pv)
        np.testing.assert_allclose(_h(o['ori_soft']), HF.encode_orientation(q, tables[n_ori], ov), rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(_h(o['pos_soft']), HF.encode_position(t, tables[n_pos], pv), rtol=1e-6, atol=1e-9)
        assert not _h(o['status']).any()
    finally:
        e.close()


def test_encode_flags_a_nan_row_and_spares_its_neighbours(tables):
    from spef_amd.engine import Engine
    q = np.array([[1.0, 0, 0, 0], [np.nan, 0, 0, 0], [0, 0.6, 0.8, 0]])
    t = np.array([[0.0, 0, 10], [1.0, 1, 12], [np.inf, 0, 10]])
    e = Engine(None, 'cuda:0')
    try:
        e.set_decode_tables(tables[1232], tables[1000])
        o = e.encode_targets(q, t)
        os_, ps, st = _h(o['ori_soft']), _h(o['pos_soft']), _h(o['status'])
        assert st.tolist() == [[0, 0], [1, 0], [0, 1]]
        assert np.isnan(os_[1]).all() and np.isnan(ps[2]).all()
        ref_o = HF.encode_orientation(q, tables[1232], HF.soft_variance(3, 12))
        ref_p = HF.encode_position(t, tables[1000], HF.soft_variance(100, 10))
        np.testing.assert_allclose(os_[[0, 2]], ref_o[[0, 2]], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(ps[[0, 1]], ref_p[[0, 1]], rtol=1e-6, atol=1e-9)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------ with a model
FEATURE_REL_MAX = {'fp32': 1e-5, 'fp16': 4e-3}      # tests/test_gpu_c2_precision.py BOUNDS: max |delta| / the map's max


@pytest.mark.parametrize('dtype', ['fp32', 'fp16'])
def test_features_and_loaded_head(golden, dtype):
    """``Engine.features`` against the fixture's pooled features (the mean of a map is no further off than the map), and a
    trainer loaded from the model evaluates to ``Engine.forward``'s logits bit for bit."""
    from spef_amd.engine import Engine
    g = golden('fwd_64x64_b2.npz')
    sd = synthetic_state_dict(mobilenet_v2('ursonet', 1728, 3), seed=1001)
    e = Engine(Bl.pack(sd, dtype=dtype), 'cuda:0')
    try:
        x = _d(g['frames'])
        f = e.features(x)
        err = np.abs(_h(f) - g['pooled']).max() / np.abs(g['pooled']).max()
        print(f'{dtype}: pooled features off by {err:.3e} of their max')
        assert err < FEATURE_REL_MAX[dtype]
        ori, pos = e.forward(x)
        tr = e.head_trainer(pos_mode='regression', Bmax=4)
        try:
            B = f.shape[0]
            to = torch.full((B, 1728), 1.0 / 1728, device='cuda')
            out = tr.evaluate(f, to, torch.zeros((B, 3), device='cuda'), want_logits=True)
            z = _h(out['logits'])
            assert np.array_equal(_bits(z[:, :1728]), _bits(_h(ori))) and np.array_equal(_bits(z[:, 1728:]), _bits(_h(pos)))
        finally:
            tr.close()
        wrong = e.head_trainer(1280, 1728, 8)
        try:
            with pytest.raises(AssertionError):
                wrong.load_model()                                     # widths differ from the blob's
            with pytest.raises(AssertionError):
                wrong.commit()
        finally:
            wrong.close()
    finally:
        e.close()


def test_features_refuses_a_keypoint_blob():
    from spef_amd import _lib as L
    from spef_amd.engine import Engine
    arch = mobilenet_v2('keypoints')
    e = Engine(Bl.pack(synthetic_state_dict(arch, seed=5, head_std=0.002), arch, dtype='fp16'), 'cuda:0')
    try:
        with pytest.raises(L.SpefError) as ei:
            e.features(_d(synth_frames(1, 240, 384, 0)))
        assert ei.value.code == L.ERR_STATE
    finally:
        e.close()


def test_int8_blob_is_refused():
    """An int8 blob's pooled buffer holds codes and its head is int8: no features, no head to load or to commit to."""
    from spef_amd.blob_q8 import pack_int8
    from spef_amd.engine import Engine
    from spef_amd.quant import calibrate
    sd = synthetic_state_dict(mobilenet_v2(), seed=1001)
    e = Engine(pack_int8(sd, calibrate(sd, synth_frames(2, 64, 64, 900))), 'cuda:0')
    try:
        with pytest.raises(L.SpefError) as ei:
            e.features(_d(synth_frames(1, 64, 64, 0)))
        assert ei.value.code == L.ERR_STATE
        tr = e.head_trainer(1280, e.n_out0, e.n_out1, pos_mode='regression' if e.n_out1 == 3 else 'classification')
        try:
            for call in (tr.load_model, tr.commit):
                with pytest.raises(L.SpefError) as ei:
                    call()
                assert ei.value.code == L.ERR_STATE
        finally:
            tr.close()
    finally:
        e.close()


def test_end_to_end_fit_commit_export(golden):
    """A synthetic fp32 model, 16 frames of 64 x 64, 1728 + 1000 bins: 40 Adam steps on the cached features towards the
    encoded poses, commit, and the committed engine decodes closer to the poses than before; a fresh engine on the
    exported blob gives the same logits bit for bit."""
    from spef_amd import _lib as L
    from spef_amd.engine import Engine
    n, n_ori, n_pos = 16, 1728, 1000
    hist, red = golden('decode_ori.npz')['hist'], golden('decode_ori.npz')['redundant']
    grid = golden('decode_pos.npz')['grid']
    blob0 = Bl.pack(synthetic_state_dict(mobilenet_v2('ursonet', n_ori, n_pos), seed=77), dtype='fp32')
    frames = _d(synth_frames(n, 64, 64, 0))
    q_true, t_true = synth_poses(n, 0)
    e = Engine(blob0, 'cuda:0')
    try:
        e.set_decode_tables(hist, grid)
        tg = e.encode_targets(q_true.astype(np.float64), t_true.astype(np.float64), mask=red)
        assert not _h(tg['status']).any()
        X = e.features(frames)

        def errors():
            dec = e.decode(L.CLASSIFICATION, L.CLASSIFICATION, *e.forward(frames))
            ang = D.angle_deg_stable(_h(dec['ori']).astype(np.float64), q_true.astype(np.float64))
            return float(np.mean(ang)), float(np.mean(np.linalg.norm(_h(dec['pos']) - t_true, axis=1)))
        before = errors()
        tr = e.head_trainer(optimizer='adam', lr=2e-3, Bmax=n)
        try:
            losses = torch.empty((40, 3), dtype=torch.float32, device='cuda')
            for s in range(40):
                tr.step(X, tg['ori_soft'], tg['pos_soft'], loss=losses[s])
            ls = _h(losses)
            tr.commit()
            W, b = (_h(t) for t in tr.weights())
        finally:
            tr.close()
        after = errors()
        print(f'loss {ls[0, 0]:.4f} -> {ls[-1, 0]:.4f}; mean angle {before[0]:.2f} -> {after[0]:.2f} deg; mean position '
              f'error {before[1]:.3f} -> {after[1]:.3f} m')
        assert np.isfinite(ls).all() and ls[-1, 0] < ls[0, 0]
        assert after[0] < before[0] and after[1] < before[1]
        ori, pos = e.forward(frames)
        fresh = Engine(Bl.replace_head(blob0, W[:n_ori], b[:n_ori], W[n_ori:], b[n_ori:]), 'cuda:0')
        try:
            o2, p2 = fresh.forward(frames)
            assert np.array_equal(_bits(_h(o2)), _bits(_h(ori))) and np.array_equal(_bits(_h(p2)), _bits(_h(pos)))
        finally:
            fresh.close()
    finally:
        e.close()


def test_finetune_tool_synthetic(tmp_path):
    """The fine-tune tool end to end on the synthetic loader (a 1728 + 3 build: position regression): feature pass,
    device-side targets, two epochs, the exported blob and finetune.json. The validation loss it reports for the head it
    kept is the reference's training loss, SPELoss(beta = 1, norm_distance = True) (train.py:83): it is held to the
    float64 twin evaluated on that head and the validation frames' features. Tolerance: the float32 logits are within
    dz = (K + 4) eps (|X| |W|^T + |b|) of the float64 ones; log-softmax moves by at most 2 max |dz| and the normalised
    Frobenius norm by at most |dz_pos|_F / |target|_F; plus 4 eps for the rounding of the loss itself and 1 eps for the
    soft labels (the device's and the twin's are float32 roundings of the same fp64 value: at most one ulp apart)."""
    import json
    import os
    from spef_amd.config import load_config, to_spe_utils
    from spef_amd.data.synthetic import speed_like_loader
    from spef_amd.engine import Engine
    from spef_amd.spe.camera import CAMERAS
    from spef_amd.tools.build_mi355x import main as build
    from spef_amd.tools.finetune_mi355x import main as finetune
    out = str(tmp_path / 'b')
    assert build(['--synthetic', '--out', out]) == 0
    assert finetune(['--build', out, '--synthetic', '128', '--epochs', '2', '--batch', '32', '--optim', 'adam', '--lr',
                     '1e-3']) == 0
    rec = json.load(open(os.path.join(out, 'finetune', 'finetune.json')))
    assert rec['frames'] == 128 and rec['valid_frames'] == 16 and rec['epochs'] == 2 and rec['steps_per_epoch'] == 4
    for k in ('train_loss', 'valid_loss', 'ori_error', 'pos_error', 'esa_score'):
        assert len(rec[k]) == 2 and np.isfinite(rec[k]).all(), k
    assert rec['train_loss'][1] < rec['train_loss'][0]
    b0 = open(os.path.join(out, 'model.spef'), 'rb').read()
    b1 = open(os.path.join(out, 'finetune', 'model.spef'), 'rb').read()
    assert len(b1) == len(b0) and b1 != b0 and Bl.describe(b1)['ops'][:-1] == Bl.describe(b0)['ops'][:-1]
    # the reported loss of the kept head against the twin
    cfg = load_config(os.path.join(out, 'config.yaml'))
    assert cfg.MODEL.HEAD.POS == 'regression'
    su = to_spe_utils(cfg, CAMERAS['speed'])
    FB, size = cfg.MI355X.BATCH_SIZE, tuple(cfg.DATA.IMG_SIZE)
    assert 128 % FB == 0 and FB >= 16
    im, tg = list(speed_like_loader(128 // FB, FB, size))[-1]          # the batch that holds the last 16 frames
    e = Engine(b0, 'cuda:0')
    try:
        X = _h(e.features(im['torch'].cuda().contiguous()))[-16:]
    finally:
        e.close()
    q, t = np.asarray(tg['ori'], np.float64)[-16:], np.asarray(tg['pos'], np.float64)[-16:]
    to = HF.encode_orientation(q, su.orientation.histogram, HF.soft_variance(cfg.DATA.ORI_SMOOTH_FACTOR, cfg.MODEL.HEAD.N_ORI_BINS_PER_DIM),
                               None if cfg.MODEL.HEAD.ORI_DELETE_UNUSED_BINS else su.orientation.redundant_flags)
    tp = t.astype(np.float32)
    info = Bl.describe(b1)
    fc = [o for o in info['ops'] if o[0] == Bl.OP_FC][0]
    n_ori, n, K = info['n_out0'], info['n_out0'] + info['n_out1'], fc[1]
    W = np.frombuffer(b1, np.float32, n * K, info['data_off'] + fc[8]).reshape(n, K)
    b = np.frombuffer(b1, np.float32, n, info['data_off'] + fc[9])
    tw = HF.HeadFitTwin(K, n_ori, 3, pos_mode='regression', beta=1.0, norm_distance=True)
    tw.set_weights(W, b)
    want = tw.evaluate(X, to, tp)[0]
    dz = (K + 4) * EPS * (np.abs(X).astype(np.float64) @ np.abs(W).astype(np.float64).T + np.abs(b))
    tol = 2 * dz[:, :n_ori].max() + np.sqrt(np.sum(dz[:, n_ori:] ** 2)) / np.sqrt(np.sum(tp.astype(np.float64) ** 2)) + \
        5 * EPS * abs(want)
    off = HF.HeadFitTwin(K, n_ori, 3, pos_mode='regression', beta=1.0, norm_distance=False)
    off.set_weights(W, b)
    print(f"best valid loss {rec['best_valid_loss']:.6f}, twin {want:.6f} (tolerance {tol:.2e}); without norm_distance "
          f"{off.evaluate(X, to, tp)[0]:.3f}")
    assert abs(rec['best_valid_loss'] - want) <= tol
    assert rec['best_valid_loss'] == min(rec['valid_loss'])
