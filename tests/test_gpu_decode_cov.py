"""GPU: the pose covariance of the soft-classification decode (csrc/k_cov.hip, ``spef_decode_cov``) against its NumPy
twin (spef_amd/spe/decode_cov.py), evaluated on the device's own PDFs and poses, and its way up through Engine,
StreamPipeline and the pose tracker.

Shapes: B in {1, 3, 65} (one row, a few, more workgroups than one wave of rows), orientation tables of 1728 and 1232
bins (the reference's), 257 (one bin past a full 256-thread stride) and 5 (most threads idle), position grids of 1000
and 8 bins, and once the largest tables spef_set_decode_tables takes in practice (8192 bins, a 21^3 = 9261-bin grid). Tolerances: a block is float64 arithmetic rounded once to float32, so 2^-22 of its largest entry (float32
rounding with a 4x margin); ``ori_hinv`` adds the inverse's sensitivity 1e-12 cond(a) to a sum taken in another order
(the bound of tests/test_decode_cov_host.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import decode_ref as D
from spef_amd import _lib as L
from spef_amd import blob as Bl
from spef_amd.arch import mobilenet_v2
from spef_amd.spe import decode_cov as DC
from spef_amd.spe import track as TK
from spef_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

BLOCK_TOL = 2.0 ** -22
ULP16 = 16 * 2.0 ** -23             # tests/test_gpu_track.py
CLS, REG = L.CLASSIFICATION, L.REGRESSION
GATE = dict(q=1e-4, p0=1.0, gate_chi2=16.81)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items() if isinstance(v, torch.Tensor)}


def _rand_quats(n):
    h = np.random.Generator(np.random.PCG64(n)).standard_normal((n, 4))
    return h / np.linalg.norm(h, axis=1, keepdims=True)


@pytest.fixture(scope='module')
def tables(golden):
    return {1728: golden('decode_ori.npz')['hist'], 1232: D.orientation_histogram(12, True)[0],
            257: _rand_quats(257), 5: _rand_quats(5), 8192: _rand_quats(8192),
            1000: golden('decode_pos.npz')['grid'], 8: D.position_histogram(2), 9261: D.position_histogram(21)}


@pytest.fixture(scope='module')
def engines(tables):
    from spef_amd.engine import Engine
    made = {}

    def get(n_ori, n_pos):
        if (n_ori, n_pos) not in made:
            e = Engine(None, 'cuda:0')
            e.set_decode_tables(None if n_ori is None else tables[n_ori], None if n_pos is None else tables[n_pos])
            made[(n_ori, n_pos)] = e
        return made[(n_ori, n_pos)]
    yield get
    for e in made.values():
        e.close()


def logits(tables, n_ori, n_pos, B, seed):
    """Bumps of three widths around a random bin-space direction per row (orientation) and around a random grid point
    (position), float32."""
    rng = np.random.Generator(np.random.PCG64(seed))
    h, g = tables[n_ori], tables[n_pos]
    q0 = rng.standard_normal((B, 4))
    q0 /= np.linalg.norm(q0, axis=1, keepdims=True)
    kappas = (4.0, 30.0, 200.0) if len(h) > 100 else (1.0, 4.0, 12.0)     # a few bins: keep more than one in play
    kappa = np.array([kappas[b % 3] for b in range(B)])
    lo = kappa[:, None] * (q0 @ h.T) ** 2
    t0 = g[rng.integers(0, len(g), B)] + rng.normal(0, 1.0, (B, 3))
    lp = -((t0[:, None, :] - g[None]) ** 2).sum(-1) / np.array([(2.0, 20.0, 200.0)[b % 3] for b in range(B)])[:, None]
    return torch.from_numpy(lo.astype(np.float32)).cuda(), torch.from_numpy(lp.astype(np.float32)).cuda()


def assert_matches_twin(dev, ori_bins, pos_grid, tag, fixed_var=(100.0, 100.0), floor_var=(0.0, 0.0), skip=()):
    """``dev``: the device's dict as NumPy. The twin runs on the device's own PDFs and poses. ``skip``: rows whose
    blocks are not compared by value (their status and NaN pattern still are)."""
    twin = DC.decode_cov_host(dev.get('ori_soft') if ori_bins is not None else None,
                              dev.get('pos_soft') if pos_grid is not None else None, dev['ori'], dev['pos'], ori_bins,
                              pos_grid, fixed_var, floor_var, dtype=np.float64)
    assert np.array_equal(dev['cov_status'], twin['cov_status']), tag
    worst = [0.0, 0.0]
    for b in range(dev['cov'].shape[0]):
        assert not dev['cov'][b, :3, 3:].any() and not dev['cov'][b, 3:, :3].any(), (tag, b)
        for sl in (slice(0, 3), slice(3, 6)):
            want, got = twin['cov'][b, sl, sl], dev['cov'][b, sl, sl].astype(np.float64)
            assert np.array_equal(np.isnan(got), np.isnan(want)), (tag, b)
            if np.isnan(want).any() or b in skip:
                continue
            if not want.any():
                assert not got.any(), (tag, b)
                continue
            err = np.abs(got - want).max() / np.abs(want).max()
            worst[0] = max(worst[0], err)
            assert err <= BLOCK_TOL, (tag, b, err)
            assert np.array_equal(got, got.T), (tag, b)
        if 'ori_hinv' in dev:
            want, got = twin['ori_hinv'][b], dev['ori_hinv'][b].astype(np.float64)
            assert np.array_equal(np.isnan(got), np.isnan(want)), (tag, b)
            if np.isnan(want).any():
                continue
            tol = (2.0 ** -22 + 1e-12 * np.linalg.cond(DC.markley_matrix(dev['ori_soft'][b], ori_bins))) * np.abs(want).max()
            err = np.abs(got - want).max()
            worst[1] = max(worst[1], err / tol)
            assert err <= tol, (tag, b, err, tol)
    print(f'{tag}: largest block error {worst[0]:.2e} of its block (bound {BLOCK_TOL:.2e}); largest ori_hinv error '
          f'{worst[1]:.3f} of its bound')
    return twin


@pytest.fixture(scope='module')
def big(engines, tables):
    """B = 65 at 1728 / 1000 bins, decoded once: (engine, the decode dict with its covariance)."""
    eng = engines(1728, 1000)
    dec = eng.decode(CLS, CLS, *logits(tables, 1728, 1000, 65, 65), want_cov=True, want_hinv=True)
    torch.cuda.synchronize()
    return eng, dec


# ---------------------------------------------------------------------------------------- kernel against twin
def test_b65_matches_twin(big, tables):
    _, dec = big
    dev = _np(dec)
    assert not dev['status'].any() and not dev['cov_status'].any()
    assert_matches_twin(dev, tables[1728], tables[1000], '1728/1000 B=65')


@pytest.mark.parametrize('n_ori,n_pos,B', [(1232, 8, 3), (257, 1000, 1), (5, 8, 3), (257, 8, 65), (8192, 9261, 1)])
def test_table_sizes_match_twin(engines, tables, n_ori, n_pos, B):
    eng = engines(n_ori, n_pos)
    dec = eng.decode(CLS, CLS, *logits(tables, n_ori, n_pos, B, 1000 * n_ori + B), want_cov=True, want_hinv=True)
    dev = _np(dec)
    assert dev['cov'].shape == (B, 6, 6) and dev['ori_hinv'].shape == (B, 4, 4) and dev['cov_status'].shape == (B,)
    assert not dev['status'].any()
    assert_matches_twin(dev, tables[n_ori], tables[n_pos], f'{n_ori}/{n_pos} B={B}')


def test_batch_independence(big):
    """A row's result does not depend on the batch it is in: B = 65 equals its slices 5 + 60, bit for bit."""
    eng, dec = big
    whole = _np(dec)
    parts = []
    for sl in (slice(0, 5), slice(5, 65)):
        part = {k: dec[k][sl].contiguous() for k in ('ori', 'pos', 'ori_soft', 'pos_soft')}
        parts.append(_np(eng.decode_cov(part, CLS, CLS, want_hinv=True)))
    for k in ('cov', 'ori_hinv', 'cov_status'):
        assert np.array_equal(_bits(np.concatenate([p[k] for p in parts])), _bits(whole[k])), k


def test_bad_rows(engines, tables):
    """Rows: 0 good, 1 NaN orientation logit, 2 one-hot orientation, 3 orientation PDF zeroed, 4 NaN position logit,
    5 position PDF zeroed. cov_status carries exactly the documented bits, the NaN blocks are where they belong, and
    the decode status is what the decode left."""
    eng = engines(1728, 1000)
    lo, lp = logits(tables, 1728, 1000, 6, 6)
    lo[1, 100] = float('nan')
    lo[2] = -1e4
    lo[2, 777] = 0.0
    lp[4, 3] = float('nan')
    dec = eng.decode(CLS, CLS, lo, lp)
    dec['ori_soft'][3] = 0.0
    dec['pos_soft'][5] = 0.0
    status = dec['status'].cpu().numpy().copy()
    assert status.tolist() == [0, 1, 0, 0, 4, 0]
    eng.decode_cov(dec, CLS, CLS, want_hinv=True)
    dev = _np(dec)
    assert np.array_equal(dev['status'], status)
    assert dev['cov_status'].tolist() == [0, DC.ORI | DC.HINV, DC.HINV, DC.ORI | DC.HINV, DC.POS, DC.POS]
    assert dev['ori_soft'][2].max() == 1.0 and dev['ori_soft'][2].sum() == 1.0
    nan_theta, nan_t, nan_h = [1, 3], [4, 5], [1, 2, 3]
    for b in range(6):
        assert np.isnan(dev['cov'][b, :3, :3]).all() == (b in nan_theta), b
        assert np.isfinite(dev['cov'][b, :3, :3]).all() == (b not in nan_theta), b
        assert np.isnan(dev['cov'][b, 3:, 3:]).all() == (b in nan_t), b
        assert np.isfinite(dev['cov'][b, 3:, 3:]).all() == (b not in nan_t), b
        assert np.isnan(dev['ori_hinv'][b]).all() == (b in nan_h) and np.isfinite(dev['ori_hinv'][b]).all() == (b not in nan_h)
    assert np.abs(dev['cov'][2, :3, :3]).max() < 1e-12            # one-hot: the bin is its own decode
    # (row 2's theta block is the square of a float32 rounding residue, ~1e-15 rad^2: all cancellation, no value)
    assert_matches_twin(dev, tables[1728], tables[1000], 'bad rows', skip=(2,))
    # the tracker takes a row with a NaN block as a row without a covariance: the fixed r
    trk, ref = eng.tracker(6), eng.tracker(6)
    good = dict(dec, status=torch.zeros_like(dec['status']), ori=dec['ori'].nan_to_num(1.0), pos=dec['pos'].nan_to_num(1.0))
    for t in (trk, ref):
        t.step(dict(good, cov=None), 1)
    a = _np(trk.step(good, 1))
    b = _np(ref.step(dict(good, cov=torch.where(torch.isnan(good['cov']).flatten(1).any(1)[:, None, None],
                                                torch.diag(torch.full((6,), 100.0, device='cuda')), good['cov'])), 1))
    assert np.array_equal(_bits(a['mahalanobis']), _bits(b['mahalanobis'])) and np.isfinite(a['mahalanobis']).all()
    trk.close()
    ref.close()


def test_modes_and_floors(engines, tables, big):
    """A regression head's block is fixed_var I whatever else is set; floor_var lands on the diagonal of a
    classification head's block and nowhere else."""
    eng, dec = big
    base = _np(dec)
    part = {k: dec[k][:3].contiguous() for k in ('ori', 'pos', 'ori_soft', 'pos_soft')}
    fl = _np(eng.decode_cov(dict(part), CLS, CLS, fixed_var=(3.0, 7.0), floor_var=(0.25, 4.0)))
    assert 'ori_hinv' not in fl
    assert_matches_twin(fl, tables[1728], tables[1000], 'floors', (3.0, 7.0), (0.25, 4.0))
    off = ~np.eye(6, dtype=bool)
    assert np.array_equal(_bits(fl['cov'][:, off]), _bits(base['cov'][:3][:, off]))
    assert (fl['cov'][:, ~off] > base['cov'][:3][:, ~off]).all()

    e_or = engines(None, 1000)                                     # orientation regression, position classification
    mixed = _np(e_or.decode_cov(dict(part, ori_soft=None), REG, CLS, fixed_var=(3.0, 7.0), floor_var=(0.25, 4.0)))
    assert np.array_equal(mixed['cov'][:, :3, :3], np.tile(3.0 * np.eye(3, dtype=np.float32), (3, 1, 1)))
    assert np.array_equal(_bits(mixed['cov'][:, 3:, 3:]), _bits(fl['cov'][:, 3:, 3:])) and not mixed['cov_status'].any()
    e_rr = engines(None, None)                                     # both in regression mode: no table is needed
    reg = _np(e_rr.decode_cov({'ori': part['ori'], 'pos': part['pos']}, REG, REG, fixed_var=(3.0, 7.0),
                              floor_var=(0.25, 4.0)))
    assert np.array_equal(reg['cov'], np.tile(np.diag([3.0] * 3 + [7.0] * 3).astype(np.float32), (3, 1, 1)))
    assert not reg['cov_status'].any()
    mixed = _np(engines(1728, None).decode_cov(dict(part, pos_soft=None), CLS, REG, fixed_var=(3.0, 7.0)))
    assert np.array_equal(mixed['cov'][:, 3:, 3:], np.tile(7.0 * np.eye(3, dtype=np.float32), (3, 1, 1)))
    assert np.array_equal(_bits(mixed['cov'][:, :3, :3]), _bits(base['cov'][:3, :3, :3]))
    with pytest.raises(AssertionError):
        e_or.decode_cov(dict(part, ori_soft=None), REG, CLS, want_hinv=True)


def test_filtered_pdfs(engines, tables):
    """The video filter's outputs are a PDF + pose pair too: T = 4, S = 2."""
    eng = engines(1728, 1000)
    vf = eng.video_filter(2)
    try:
        vid = vf.step(eng.decode(CLS, CLS, *logits(tables, 1728, 1000, 8, 42)), 4)
        dev = _np(eng.decode_cov(vid, CLS, CLS, want_hinv=True))
    finally:
        vf.close()
    assert not dev['status'].any() and not dev['cov_status'].any()
    assert_matches_twin(dev, tables[1728], tables[1000], 'filtered T=4 S=2')


def test_off_switch_and_capture(engines, tables, big):
    """Without want_cov the decode returns the keys and the bits it always did; with it, the same bits plus the new
    keys; a captured decode_cov replays to the same bits."""
    eng, dec = big
    lo, lp = logits(tables, 1728, 1000, 65, 65)
    plain = eng.decode(CLS, CLS, lo, lp)
    assert set(plain) == {'ori', 'pos', 'ori_soft', 'pos_soft', 'status'}
    assert set(dec) == set(plain) | {'cov', 'cov_status', 'ori_hinv'}
    assert set(eng.decode(CLS, CLS, lo, lp, want_soft=False, want_cov=True)) == set(plain) | {'cov', 'cov_status'}
    for k in plain:
        assert np.array_equal(_bits(plain[k].cpu().numpy()), _bits(dec[k].cpu().numpy())), k
    with pytest.raises(AssertionError):
        eng.decode(CLS, CLS, lo, lp, floor_var=(1.0, 1.0))
    torch.cuda.synchronize()
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cap = eng.decode_cov(dict(plain), CLS, CLS, want_hinv=True)
    g.replay()
    torch.cuda.synchronize()
    for k in ('cov', 'ori_hinv', 'cov_status'):
        assert np.array_equal(_bits(cap[k].cpu().numpy()), _bits(dec[k].cpu().numpy())), k
    del g


def test_abi_errors(engines, tables, big):
    """Wrong widths, a NULL PDF or pose of a classification head, a bad variance, B < 1, NULL outputs and ori_hinv
    behind a regression head: SPEF_ERR_ARG with nothing enqueued; a missing table: SPEF_ERR_STATE."""
    from spef_amd.engine import _ptr, _stream
    eng, dec = big
    lib, st = eng.lib, _stream(eng.device)
    cov = torch.full((65, 36), 7.0, device='cuda')
    hinv = torch.full((65, 16), 7.0, device='cuda')
    cs = torch.full((65,), 77, dtype=torch.int32, device='cuda')

    def prm(fixed=(100.0, 100.0), floor=(0.0, 0.0)):
        return L.CovParams((C.c_double * 2)(*fixed), (C.c_double * 2)(*floor))

    def call(ctx=eng.ctx, om=CLS, pm=CLS, op=dec['ori_soft'], no=1728, pp=dec['pos_soft'], npos=1000, q=dec['ori'],
             t=dec['pos'], B=65, p=prm(), cov=cov, hinv=hinv, cs=cs):
        return lib.spef_decode_cov(ctx, om, pm, _ptr(op), no, _ptr(pp), npos, _ptr(q), _ptr(t), B,
                                   C.byref(p) if p is not None else None, _ptr(cov), _ptr(hinv), _ptr(cs), st)
    nan, inf = float('nan'), float('inf')
    for kw in (dict(ctx=None), dict(no=1727), dict(no=1232), dict(npos=999), dict(npos=0), dict(op=None), dict(pp=None),
               dict(q=None), dict(t=None), dict(B=0), dict(B=-1), dict(p=None), dict(cov=None), dict(cs=None),
               dict(om=2), dict(pm=3), dict(om=REG), dict(p=prm(fixed=(-1.0, 1.0))), dict(p=prm(fixed=(1.0, nan))),
               dict(p=prm(floor=(inf, 0.0))), dict(p=prm(floor=(0.0, -1e-300)))):
        assert call(**kw) == L.ERR_ARG, kw
    bare = engines(None, None)
    assert call(ctx=bare.ctx) == L.ERR_STATE and call(ctx=bare.ctx, om=REG, hinv=None) == L.ERR_STATE
    assert call(ctx=engines(1728, None).ctx) == L.ERR_STATE
    torch.cuda.synchronize()
    assert (cov == 7).all().item() and (hinv == 7).all().item() and (cs == 77).all().item()
    assert call(hinv=None) == L.OK                                  # ori_hinv is optional
    torch.cuda.synchronize()
    assert np.array_equal(_bits(cov.cpu().numpy().reshape(65, 6, 6)), _bits(dec['cov'].cpu().numpy()))
    assert (hinv == 7).all().item() and not cs.any().item()


# ---------------------------------------------------------------------------------------- into the tracker
def test_gating_at_engine_level(engines, golden):
    """decode of planted logits -> decode_cov -> tracker.step: a still track of one planted T = 0.2 pose whose frame 5
    is the planted pose farthest from it. With the fixed r = 100 nothing is gated; with the PDFs' covariance frame 5
    is, and the device agrees with the host tracker fed the twin's covariance."""
    eng = engines(1728, None)
    g = golden('decode_ori.npz')
    lg = g['planted_logits'][2, :4]
    q4 = D.decode_orientation_batch(D.softmax_f32(lg), g['hist']).astype(np.float64)
    ang = 2 * np.arccos(np.minimum(1.0, np.abs(q4[1:] @ q4[0])))
    assert ang.max() > 1.0                                          # the scenario's own precondition
    rows = [0] * 8
    rows[5] = 1 + int(np.argmax(ang))
    lo = torch.from_numpy(np.ascontiguousarray(lg[rows])).cuda()
    lp = torch.from_numpy(np.tile(np.float32([0.1, -0.2, 9.0]), (8, 1))).cuda()
    fixed, pdf = eng.tracker(1, **GATE), eng.tracker(1, **GATE)
    try:
        plain = eng.decode(CLS, REG, lo, lp)
        a = _np(fixed.step(plain, 8))
        dec = eng.decode(CLS, REG, lo, lp, want_cov=True, fixed_var=pdf.params['r'])
        b = _np(pdf.step(dec, 8))
    finally:
        fixed.close()
        pdf.close()
    dev = _np(dec)
    twin = assert_matches_twin(dev, g['hist'], None, 'planted T=0.2')
    host = TK.PoseTrackerHost(1, **GATE).step(dev['ori'], dev['pos'], twin['cov'].astype(np.float32), dev['status'])
    print(f'outlier {np.degrees(ang.max()):.1f} deg off; d2 with r = 100: {a["mahalanobis"][5]:.3f}, with the PDF '
          f'covariance: {b["mahalanobis"][5]:.1f}')
    assert not a['track_status'].any()
    assert b['track_status'][5] & TK.GATED and not b['track_status'][:5].any()
    assert np.array_equal(b['track_status'], host['track_status'])
    np.testing.assert_allclose(b['mahalanobis'], host['mahalanobis'], rtol=1e-4, atol=1e-9)


@pytest.mark.parametrize('graphs', (False, True))
def test_pipeline_feeds_the_tracker(golden, graphs):
    """StreamPipeline.submit(want_cov=True, track=) on 64 x 64 frames, T = 8, S = 1, behind a head whose orientation
    bias is a planted T = 0.2 PDF: dec['cov'] is the kernel's, the step stays outside the recorded graph, and the
    tracked poses equal the host tracker fed the twin's covariance at the tolerances of
    tests/test_gpu_track.py::test_inference_tracker. Without want_cov the dict has no 'cov'."""
    from spef_amd.pipeline import StreamPipeline
    g = golden('decode_ori.npz')
    arch = mobilenet_v2('ursonet', 1728, 3)
    sd = synthetic_state_dict(arch, seed=1001, head_std=2e-4, pos_bias=(0.3, -0.2, 12.0))
    sd['head.ori.1.bias'] = g['planted_logits'][2, 0].astype(np.float32)
    rng = np.random.Generator(np.random.PCG64(64))
    x = torch.from_numpy(rng.random((8, 3, 64, 64), dtype=np.float32)).cuda()
    prm = dict(GATE, r=(50.0, 25.0))
    pipe = StreamPipeline(Bl.pack(sd, arch, dtype='fp16'), 'cuda:0', depth=2, ori_bins=g['hist'])
    try:
        pipe.use_graphs(graphs)
        trk = pipe.engine.tracker(1, **prm)
        assert 'cov' not in pipe.submit(x, CLS, REG)
        outs = [pipe.submit(x, CLS, REG, want_cov=True, track=trk) for _ in range(2)]   # both slots; 16 frames
        pipe.synchronize()
        host = TK.PoseTrackerHost(1, **prm)
        for o in outs:
            dev = _np(o)
            assert not dev['status'].any() and not dev['cov_status'].any() and 'ori_hinv' not in o
            twin = assert_matches_twin(dev, g['hist'], None, f'pipeline graphs={graphs}', fixed_var=(50.0, 25.0))
            assert np.array_equal(dev['cov'][:, 3:, 3:], np.tile(25.0 * np.eye(3, dtype=np.float32), (8, 1, 1)))
            want = host.step(dev['ori'], dev['pos'], twin['cov'].astype(np.float32), dev['status'])
            got = _np(o['track'])
            mag = np.abs(want['pos']).max()
            assert np.array_equal(got['track_status'], want['track_status']) and not got['track_status'].any()
            assert (np.abs((got['ori'].astype(np.float64) * want['ori']).sum(1)) >= 1 - 1e-6).all()
            assert np.abs(got['pos'] - want['pos']).max() <= ULP16 * mag
            np.testing.assert_allclose(got['mahalanobis'], want['mahalanobis'], rtol=1e-4, atol=1e-9)
        sig = np.degrees(np.sqrt(np.trace(_np(outs[0])['cov'][0, :3, :3])))
        print(f'planted head: sigma {sig:.1f} deg')
        assert sig < 30.0                                           # the planted PDF, not a flat one (2.2 rad)
        trk.close()
    finally:
        pipe.close()


def test_predict_and_predict_tracked(golden):
    """SPEMi355x.predict(want_cov=True) adds 'cov', 'cov_status' and 'ori_hinv'; predict_tracked(pdf_cov=True) equals
    decode(want_cov, fixed_var = r) -> tracker.step at engine level bit for bit; both off by default."""
    from spef_amd.spe.spe_utils import SPEUtils
    from spef_amd.spe_mi355x import SPEMi355x
    su = SPEUtils(None, 'classification', 12, 3, False, 'classification')
    sd = synthetic_state_dict(mobilenet_v2('ursonet', su.orientation.n_bins, su.position.n_bins), seed=1001)
    x = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).random((4, 3, 64, 64), dtype=np.float32))
    spe = SPEMi355x(Bl.pack(sd, dtype='fp16'), 'cuda:0', su)
    try:
        plain, _ = spe.predict(x)
        pose, _ = spe.predict(x, want_cov=True)
        assert set(plain) == {'ori', 'pos', 'ori_soft', 'pos_soft'} and set(pose) == set(plain) | {'cov', 'cov_status', 'ori_hinv'}
        for k in plain:
            assert np.array_equal(_bits(plain[k]), _bits(pose[k])), k
        assert pose['cov'].shape == (4, 6, 6) and pose['ori_hinv'].shape == (4, 4, 4) and not pose['cov_status'].any()
        assert_matches_twin(dict(pose), su.orientation.histogram, su.position.histogram, 'predict')
        p = dict(gate_chi2=16.81, r=(9.0, 4.0))
        still, tracked, lat = spe.predict_tracked(x, n_streams=2, pdf_cov=True, floor_var=(1e-4, 1e-2), **p)
        assert lat > 0 and set(still) == set(plain)
        eng = spe.engine
        dec = eng.decode(CLS, CLS, *eng.forward(x.cuda()), want_cov=True, fixed_var=(9.0, 4.0), floor_var=(1e-4, 1e-2))
        trk = eng.tracker(2, **p)
        want = _np(trk.step(dec, 2))
        trk.close()
        for k in tracked:
            assert np.array_equal(_bits(tracked[k]), _bits(want[k])), k
    finally:
        spe.close()
