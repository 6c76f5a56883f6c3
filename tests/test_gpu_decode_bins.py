"""GPU: the decode, the video filter and the head at bin counts other than the 12^3 = 1728 (1232) grid every other
test uses: the kernel variants that only run above 2048 bins (decode_ori_kernel<32, false / true>,
video_scan_kernel<32, METRIC> for all six metrics, the mixed case of one head above 2048 and the other far below),
the width edges of the ones below (n = 1, n < 256, exact multiples of 256, 2048 / 2049, 8191 / 8192 / 8193), the
position decode at 27 .. 9261 bins, normalize_ori_kernel over more than one workgroup, and head widths whose out0 /
out1 boundary falls inside one lane's 4-row group of fc_kernel (n0 % 4 != 0).

References: oracle/decode_ref.py (softmax_f32, decode_orientation, decode_position_batch, l2_normalise_f32,
angle_deg_stable), oracle/model_ref.py and the host twin spef_amd.temporal.filter_sequences. Tolerances are the ones
the project uses for the same quantities: soft outputs rtol 1e-5 / atol 1e-9 and orientation < 1e-3 degrees, position
< 1e-4 (tests/test_gpu_parity.py), video PDFs and distances tests/test_gpu_video.py's _rtol, head outputs 1e-3.

The angle comparisons need a well-conditioned eigenvector: every row compared by angle has a reference eigenvalue
gap l1 - l2 >= 0.1 of a = sum_i p_i q_i q_i^T, asserted on the host before the GPU runs (the smallest over all the
peaked rows here is printed by each case). Flat, near-flat and exactly degenerate rows are checked by the property
the decode must satisfy instead (tests/test_gpu_parity.py::test_decode_orientation_flat_softmax): a unit quaternion
whose Rayleigh quotient is the top eigenvalue."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import decode_ref as D
from oracle import model_ref as M
from spef_amd import _lib as L
from spef_amd import temporal as TP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_video import ORI, POS, _moving, _rtol, _step  # noqa: E402

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-3                    # tests/test_gpu_parity.py
MIN_GAP = 0.1                       # smallest reference eigenvalue gap of a row that is compared by angle
KAPPAS = (8.0, 50.0, 400.0)
CUBIC = {2197: 13, 4096: 16, 8000: 20}
RANDOM_N = (1, 2, 255, 256, 257, 2047, 2048, 2049, 4096, 8191, 8192)
ORI_TABLES = [f'cubic{n}' for n in CUBIC] + [f'rand{n}' for n in RANDOM_N]
WIDE = (2049, 4096, 8192)           # decode_ori_kernel<32>: just above the switch, mid, the limit


# ---------------------------------------------------------------------------------------- shared, read-only
def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def table(name):
    """'cubicN': orientation_histogram(k) with k^3 = N bins; 'randN': N unit quaternions, PCG64(N) normal values
    normalised in float64; 'oriN' / 'posN': the N-bin orientation / position grid of the video tests."""
    if name.startswith('cubic'):
        return _frozen(D.orientation_histogram(CUBIC[int(name[5:])], False)[0])
    if name.startswith('rand'):
        n = int(name[4:])
        h = np.random.Generator(np.random.PCG64(n)).standard_normal((n, 4))
        return _frozen(h / np.linalg.norm(h, axis=1, keepdims=True))
    if name == 'ori27':
        return _frozen(D.orientation_histogram(3, False)[0])
    if name.startswith('ori'):
        return table({2197: 'cubic2197', 8192: 'rand8192'}[int(name[3:])])
    assert name.startswith('pos')
    return _frozen(D.position_histogram({27: 3, 2197: 13, 9261: 21}[int(name[3:])]))


@pytest.fixture(scope='module')
def engines():
    """Weightless contexts with decode tables: (orientation table name or None, position table name or None)."""
    from spef_amd.engine import Engine
    made = {}

    def get(ori, pos):
        if (ori, pos) not in made:
            e = Engine(None, 'cuda:0')
            e.set_decode_tables(None if ori is None else table(ori), None if pos is None else table(pos))
            made[(ori, pos)] = e
        return made[(ori, pos)]
    yield get
    for e in made.values():
        e.close()


def peaked_logits(h, rows, seed):
    """float32 logits kappa * (h . q0)^2 [rows, n]: a Bingham-like bump around a random unit quaternion q0 per row,
    the concentrations of KAPPAS in turn (rows = 24: 8 rows per concentration)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    q0 = rng.standard_normal((rows, 4))
    q0 /= np.linalg.norm(q0, axis=1, keepdims=True)
    kappa = np.array([KAPPAS[r % len(KAPPAS)] for r in range(rows)])
    return (kappa[:, None] * (q0 @ np.asarray(h, np.float64).T) ** 2).astype(np.float32)


def moments(p, h):
    """a = sum_i p_i q_i q_i^T in float64 for every row of p -> [rows, 4, 4]."""
    hb = np.asarray(h, np.float64)
    return np.einsum('bi,ij,ik->bjk', np.asarray(p, np.float64), hb, hb)


@functools.lru_cache(maxsize=None)
def peaked_case(name, rows=24):
    """-> (logits, reference softmax, reference quaternions, eigenvalue gaps) of one table, computed once."""
    h = table(name)
    lg = peaked_logits(h, rows, 100000 + h.shape[0])
    p = D.softmax_f32(lg)
    lam = np.linalg.eigvalsh(moments(p, h))
    return _frozen(lg), _frozen(p), _frozen(D.decode_orientation_batch(p, h)), _frozen(lam[:, -1] - lam[:, -2])


def assert_rayleigh(q, p, h, tag):
    """test_decode_orientation_flat_softmax's assertion: q's Rayleigh quotient is the top eigenvalue of a."""
    q = np.asarray(q, np.float64)
    assert np.isfinite(q).all(), tag
    np.testing.assert_allclose(np.linalg.norm(q, axis=1), 1.0, atol=1e-6)
    for b, a in enumerate(moments(p, h)):
        lam = np.linalg.eigvalsh(a)
        assert q[b] @ a @ q[b] >= lam[-1] - 1e-6 * (lam[-1] - lam[0] + 1e-12) - 1e-7, (tag, b)


def decode_ori(eng, lg):
    out = eng.decode(L.CLASSIFICATION, L.REGRESSION, torch.from_numpy(np.array(lg, np.float32)).cuda(),
                     torch.zeros((lg.shape[0], 3), device='cuda'))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def assert_peaked(eng, lg, p, rq, gap, tag):
    assert gap.min() >= MIN_GAP, (tag, gap.min())            # the reference alone, before anything runs on the GPU
    out = decode_ori(eng, lg)
    soft_err = np.abs(out['ori_soft'] - p).max()
    ang = D.angle_deg_stable(out['ori'], rq)
    nrm = np.abs(np.linalg.norm(out['ori'].astype(np.float64), axis=1) - 1).max()
    print(f'{tag}: min gap {gap.min():.3f}, max |d soft| {soft_err:.3e}, max rel '
          f'{np.abs(out["ori_soft"] / np.where(p > 1e-30, p, 1) - 1)[p > 1e-30].max():.3e}, max angle {ang.max():.3e} deg, '
          f'max |norm - 1| {nrm:.3e}')
    np.testing.assert_allclose(out['ori_soft'], p, rtol=1e-5, atol=1e-9)
    assert ang.max() < 1e-3, (tag, ang.max())
    assert nrm <= 1e-6, (tag, nrm)
    assert not out['status'].any(), tag


# ---------------------------------------------------------------------------------------- 1. orientation decode
@pytest.mark.parametrize('name', ORI_TABLES)
def test_decode_orientation_every_width(engines, name):
    lg, p, rq, gap = peaked_case(name)
    assert_peaked(engines(name, None), lg, p, rq, gap, name)


@pytest.mark.parametrize('B', [1, 67])
def test_decode_orientation_batch_sizes(engines, B):
    h = table('cubic2197')
    lg = peaked_logits(h, B, 200000 + B)
    p = D.softmax_f32(lg)
    lam = np.linalg.eigvalsh(moments(p, h))
    assert_peaked(engines('cubic2197', None), lg, p, D.decode_orientation_batch(p, h), lam[:, -1] - lam[:, -2],
                  f'cubic2197 B={B}')


@pytest.mark.parametrize('n', WIDE)
def test_decode_orientation_flat_softmax_wide(engines, n):
    """The rows of test_decode_orientation_flat_softmax through decode_ori_kernel<32>."""
    h = table(f'rand{n}')
    rng = np.random.Generator(np.random.PCG64(11))
    for scale in (0.0, 1e-4, 1e-2):
        lg = (scale * rng.standard_normal((8, n))).astype(np.float32)
        out = decode_ori(engines(f'rand{n}', None), lg)
        assert not out['status'].any()
        assert_rayleigh(out['ori'], D.softmax_f32(lg), h, (n, scale))


@pytest.mark.parametrize('n', WIDE)
def test_decode_orientation_degenerate_pair(n):
    """Two mutually orthogonal bins share all the mass (logit 0, every other bin -1e4: their exp is 0): the top
    eigenvalue 1/2 is exactly double and the repeated squaring never reaches rank one, so it runs out its steps. Any
    unit vector of the plane is right: the Rayleigh property only. The two bins lie in different threads, one of
    them in the last (partly filled) register slot."""
    from spef_amd.engine import Engine
    h = table(f'rand{n}').copy()
    i0, i1 = 5, n - 1
    h[i0], h[i1] = (1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0)
    lg = np.full((1, n), -1e4, np.float32)
    lg[0, [i0, i1]] = 0.0
    p = D.softmax_f32(lg)
    assert p[0, i0] == 0.5 and p[0, i1] == 0.5 and p.sum() == 1.0
    eng = Engine(None, 'cuda:0')
    try:
        eng.set_decode_tables(h, None)
        out = decode_ori(eng, lg)
    finally:
        eng.close()
    print(f'degenerate pair n={n}: q = {out["ori"][0]}')
    np.testing.assert_array_equal(out['ori_soft'], p)
    assert not out['status'].any()
    assert_rayleigh(out['ori'], p, h, n)
    assert np.abs(out['ori'][0, 2:]).max() <= 1e-6            # in the plane of the two bins


@pytest.mark.parametrize('n', [2049, 8192])
def test_decode_orientation_bad_rows_wide(engines, n):
    """A row with one NaN and an all -inf row set status bit 1 (their quaternion is NaN); the good rows around them
    are what they are in a batch without bad rows, bit for bit."""
    name = f'rand{n}'
    lg, p, rq, gap = peaked_case(name)
    bad = np.ascontiguousarray(lg[:5]).copy()
    bad[1, n - 3] = np.nan
    bad[3] = -np.inf
    out, clean = decode_ori(engines(name, None), bad), decode_ori(engines(name, None), lg[:5])
    assert list(out['status']) == [0, 1, 0, 1, 0]
    assert np.isnan(out['ori'][[1, 3]]).all()
    good = [0, 2, 4]
    for k in ('ori', 'ori_soft'):
        np.testing.assert_array_equal(out[k][good], clean[k][good], err_msg=k)
    assert D.angle_deg_stable(out['ori'][good], rq[good]).max() < 1e-3
    np.testing.assert_allclose(out['ori_soft'][good], p[good], rtol=1e-5, atol=1e-9)


def test_set_decode_tables_rejects_8193_orientation_bins():
    from spef_amd.engine import Engine
    h = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (8193, 1))
    eng = Engine(None, 'cuda:0')
    try:
        with pytest.raises(AssertionError, match='8192'):
            eng.set_decode_tables(h, None)
        eng.set_decode_tables(h[:8192], None)                 # the limit itself is accepted
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------- 2. position decode
def check_position_decode(eng, grid, tag):
    lg = (3 * np.random.Generator(np.random.PCG64(grid.shape[0])).standard_normal((5, grid.shape[0]))).astype(np.float32)
    out = eng.decode(L.REGRESSION, L.CLASSIFICATION, torch.ones((5, 4), device='cuda'), torch.from_numpy(lg).cuda())
    torch.cuda.synchronize()
    soft, pos = out['pos_soft'].cpu().numpy(), out['pos'].cpu().numpy()
    p = D.softmax_f32(lg)
    dpos = np.abs(pos - D.decode_position_batch(p, grid)).max()
    print(f'{tag}: max rel d soft {np.abs(soft / p - 1).max():.3e}, max |d pos| {dpos:.3e}')
    np.testing.assert_allclose(soft, p, rtol=1e-5, atol=1e-9)
    assert dpos < 1e-4, (tag, dpos)
    assert not out['status'].cpu().numpy().any()


@pytest.mark.parametrize('n', [27, 2197, 9261])
def test_decode_position_grids(engines, n):
    check_position_decode(engines(None, f'pos{n}'), table(f'pos{n}'), f'pos{n}')


def _raw_decode(eng, ori_mode, pos_mode, ori_raw, pos_raw, bufs):
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    L.check(eng.lib.spef_decode(eng.ctx, ori_mode, pos_mode, p(ori_raw), ori_raw.shape[1], p(pos_raw), pos_raw.shape[1],
                                ori_raw.shape[0], p(bufs.get('ori_soft')), p(bufs['quat']), p(bufs.get('pos_soft')),
                                p(bufs['pos']), p(bufs['status']), None))
    torch.cuda.synchronize()


def test_decode_writes_every_output_word(engines):
    """spef_decode owns its outputs: with the status words and every output pre-filled with -7, a classification /
    classification decode leaves every status word 0 and no -7 anywhere."""
    eng = engines('cubic2197', 'pos2197')
    B, dev = 5, 'cuda:0'
    lg = torch.from_numpy(np.array(peaked_case('cubic2197')[0][:B])).cuda()
    pl = torch.from_numpy((3 * np.random.Generator(np.random.PCG64(7)).standard_normal((B, 2197))).astype(np.float32)).cuda()
    bufs = {k: torch.full(shape, -7.0, device=dev) for k, shape in
            (('ori_soft', (B, 2197)), ('pos_soft', (B, 2197)), ('quat', (B, 4)), ('pos', (B, 3)))}
    bufs['status'] = torch.full((B,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    _raw_decode(eng, L.CLASSIFICATION, L.CLASSIFICATION, lg, pl, bufs)
    assert not bool(bufs['status'].any())
    for k, v in bufs.items():
        assert not bool((v == -7).any()), k
    np.testing.assert_allclose(bufs['ori_soft'].sum(1).cpu().numpy(), 1.0, rtol=1e-5)
    np.testing.assert_allclose(bufs['pos_soft'].sum(1).cpu().numpy(), 1.0, rtol=1e-5)


def test_decode_regression_more_than_one_workgroup(engines):
    """Regression / regression at B = 257 (normalize_ori_kernel's second workgroup holds one row): L2 normalisation
    against the oracle, status zeroed, and pos = pos_raw bit for bit, into a separate buffer and in place."""
    eng = engines(None, None)
    B, dev = 257, 'cuda:0'
    rng = np.random.Generator(np.random.PCG64(257))
    raw = (4 * rng.standard_normal((B, 4))).astype(np.float32)
    praw = (10 * rng.standard_normal((B, 3))).astype(np.float32)
    d_raw, d_praw = torch.from_numpy(raw).cuda(), torch.from_numpy(praw).cuda()
    bufs = {'quat': torch.full((B, 4), -7.0, device=dev), 'pos': torch.full((B, 3), -7.0, device=dev),
            'status': torch.full((B,), -7, dtype=torch.int32, device=dev)}
    torch.cuda.synchronize()
    _raw_decode(eng, L.REGRESSION, L.REGRESSION, d_raw, d_praw, bufs)
    want = D.l2_normalise_f32(raw)
    print(f'normalize_ori B={B}: max |d q| {np.abs(bufs["quat"].cpu().numpy() - want).max():.3e}')
    np.testing.assert_allclose(bufs['quat'].cpu().numpy(), want, rtol=0, atol=1e-6)
    assert not bool(bufs['status'].any())
    np.testing.assert_array_equal(bufs['pos'].cpu().numpy().view(np.uint32), praw.view(np.uint32))
    # in place: pos is pos_raw itself
    bufs2 = {'quat': torch.full((B, 4), -7.0, device=dev), 'pos': d_praw,
             'status': torch.full((B,), -7, dtype=torch.int32, device=dev)}
    torch.cuda.synchronize()
    _raw_decode(eng, L.REGRESSION, L.REGRESSION, d_raw, d_praw, bufs2)
    np.testing.assert_array_equal(d_praw.cpu().numpy().view(np.uint32), praw.view(np.uint32))
    np.testing.assert_array_equal(bufs2['quat'].cpu().numpy(), bufs['quat'].cpu().numpy())
    assert not bool(bufs2['status'].any())


# ---------------------------------------------------------------------------------------- 3. video filter
VIDEO_PAIRS = [(2197, 2197), (8192, 27), (27, 2197)]     # both heads <32>; ori <32> per 32 + pos per 1; per 1 + per 9


@functools.lru_cache(maxsize=None)
def moving(T, S, n, head, metric):
    """test_gpu_video._moving (with its assertion that every blend weight lies in [0.2, 0.9]), computed once (the tests only read it)."""
    return _moving(T, S, n, ORI if head == 'ori' else POS, metric)


def video_engine(engines, n_ori, n_pos):
    return engines(f'ori{n_ori}', f'pos{n_pos}')


@pytest.mark.parametrize('metric', TP.METRICS)
@pytest.mark.parametrize('n_ori,n_pos', VIDEO_PAIRS)
def test_video_filter_matches_host_twin_wide(engines, metric, n_ori, n_pos):
    """The body of test_gpu_video.py::test_video_filter_matches_host_twin above 2048 bins; for l2 with the orientation
    head above 2048 also the decode of the filtered PDFs (decode_ori_kernel<32, true>)."""
    T, S = 5, 3
    xo, xp = moving(T, S, n_ori, 'ori', metric), moving(T, S, n_pos, 'pos', metric)
    wo, do, _ = TP.filter_sequences(xo, ORI['n'], ORI['alpha'], metric)
    wp, dp, _ = TP.filter_sequences(xp, POS['n'], POS['alpha'], metric)
    w = np.concatenate([np.exp(-np.float32(ORI['alpha']) * do[1:]).ravel(), np.exp(-np.float32(POS['alpha']) * dp[1:]).ravel()])
    print(f'{metric} n={n_ori}/{n_pos}: blend weights {w.min():.3f} .. {w.max():.3f}')
    eng = video_engine(engines, n_ori, n_pos)
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
    if metric == 'l2' and n_ori > 2048:
        rq = D.decode_orientation_batch(out['ori_soft'], table(f'ori{n_ori}'))
        ang = D.angle_deg_stable(out['ori'], rq).max()
        dpos = np.abs(out['pos'] - D.decode_position_batch(out['pos_soft'], table(f'pos{n_pos}'))).max()
        print(f'l2 n={n_ori}/{n_pos} filtered poses: max angle {ang:.3e} deg, max |d pos| {dpos:.3e}')
        assert ang < 1e-3 and dpos < 1e-4, (ang, dpos)


def test_video_status_bits_wide(engines):
    """The bad-frame block of test_gpu_video.py::test_video_decode_and_status_bits at 2197 / 2197 bins."""
    T, S = 5, 3
    xo, xp = moving(T, S, 2197, 'ori', 'l2'), moving(T, S, 2197, 'pos', 'l2')
    bo, bp = xo.copy(), xp.copy()
    bp[1, 0] = 0.0
    bo[2, 1, 5] = np.nan
    bp[2, 1, 5] = np.nan
    bo[3, 2] = 0.0
    vf = video_engine(engines, 2197, 2197).video_filter(S)
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


def test_video_split_equals_one_shot_wasserstein_wide(engines):
    """T = 6 in one call equals 2 + 4 in two, bit for bit, at 2197 / 2197 bins: the fp64 prefix scan over threads
    that own 9 bins each, and the state written and read back between the calls."""
    T, S = 6, 3
    xo, xp = moving(T, S, 2197, 'ori', 'wasserstein'), moving(T, S, 2197, 'pos', 'wasserstein')
    vf = video_engine(engines, 2197, 2197).video_filter(S, 'wasserstein')
    one = _step(vf, xo, xp)
    vf.reset()
    a, b = _step(vf, xo[:2], xp[:2]), _step(vf, xo[2:], xp[2:])
    vf.close()
    assert (one['ori_distance'][S:] > 0).all() and (one['pos_distance'][S:] > 0).all()
    for k in ('ori_soft', 'pos_soft', 'ori_distance', 'pos_distance', 'ori', 'pos', 'status'):
        np.testing.assert_array_equal(np.concatenate([a[k], b[k]]), one[k], err_msg=k)


def test_video_set_state_continues_a_sequence_wide(engines):
    """test_gpu_video.py::test_video_set_state_continues_a_sequence at 8192 / 27 bins (video_set_state_kernel with 32
    bins and with one bin per thread)."""
    T, S = 4, 2
    xo, xp = moving(T, S, 8192, 'ori', 'l2'), moving(T, S, 27, 'pos', 'l2')
    eng = video_engine(engines, 8192, 27)
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


def test_video_create_rejects_more_than_8192_bins(engines):
    """A 21^3 = 9261-bin position grid is fine for the still-frame decode, but the video scan holds at most 32 bins
    per thread: spef_video_create refuses it (it used to succeed, and every step then failed with a bare HIP
    'invalid value'), names the limit and the count, leaves the handle null and the context usable."""
    eng = engines('ori27', 'pos9261')
    h = C.c_void_p()
    assert eng.lib.spef_video_create(eng.ctx, 2, 0, 0.8, 16.49, 0.5, 48.64, C.byref(h)) == L.ERR_ARG
    assert h.value is None
    msg = eng.lib.spef_last_error().decode()
    assert '8192' in msg and '9261' in msg and 'position' in msg, msg
    with pytest.raises(AssertionError, match='8192'):
        eng.video_filter(2)
    check_position_decode(eng, table('pos9261'), 'pos9261 after the refused create')
    vf = engines('ori8192', 'pos27').video_filter(2)            # 8192 itself is accepted
    vf.close()


# ---------------------------------------------------------------------------------------- 4. head widths
@pytest.mark.parametrize('n_ori,n_pos,batches', [(27, 27, (3,)), (2197, 125, (3, 17))], ids=['27+27', '2197+125'])
def test_head_width_splits_a_lane_group(n_ori, n_pos, batches):
    """fc_kernel with n0 % 4 != 0: one lane's four rows go partly to out0 and partly to out1 (27 = 6 * 4 + 3,
    2197 = 549 * 4 + 1), and the last tile is partly padding (54 and 2322 are no multiples of 16). B = 17 adds a second
    image group with 15 masked rows. Sentinels: every element of both outputs is written."""
    from spef_amd import blob as Bl
    from spef_amd.arch import mobilenet_v2
    from spef_amd.engine import Engine
    from spef_amd.weights import synthetic_state_dict
    sd = synthetic_state_dict(mobilenet_v2('ursonet', n_ori, n_pos), seed=1001)
    eng = Engine(Bl.pack(sd, dtype='fp16'), 'cuda:0')
    try:
        assert (eng.n_out0, eng.n_out1) == (n_ori, n_pos)
        for B in batches:
            x = torch.from_numpy(np.random.Generator(np.random.PCG64(40 + B)).random((B, 3, 64, 96), dtype=np.float32))
            ro, rp = M.forward(x, sd)
            sentinel = 12345.0
            out0 = torch.full((B, n_ori), sentinel, device='cuda:0')
            out1 = torch.full((B, n_pos), sentinel, device='cuda:0')
            torch.cuda.synchronize()
            eng.forward(x.cuda(), out0, out1)
            torch.cuda.synchronize()
            o, p = out0.cpu().numpy(), out1.cpu().numpy()
            assert not (o == sentinel).any() and not (p == sentinel).any()
            d0, d1 = np.abs(o - ro.numpy()).max(), np.abs(p - rp.numpy()).max()
            print(f'head {n_ori}+{n_pos} B={B}: max |d ori| {d0:.3e}, max |d pos| {d1:.3e}')
            assert d0 < LOGIT_TOL and d1 < LOGIT_TOL, (B, d0, d1)
    finally:
        eng.close()
