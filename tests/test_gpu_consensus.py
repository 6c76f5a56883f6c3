"""GPU: the 3-point consensus between EPnP and the refinement (csrc/k_consensus.hip) against its NumPy twin
(spef_amd/spe/consensus.py) and against facts that need no twin, and its way up through Engine, StreamPipeline and
SPEMi355x."""
import os
import sys

import numpy as np
import pytest
import torch

from spef_amd import _lib as L
from spef_amd import blob as Bl
from spef_amd.arch import mobilenet_v2
from spef_amd.quaternion import angle_deg
from spef_amd.spe import consensus as CS
from spef_amd.spe import refine as RF
from spef_amd.weights import plant_keypoint_head, synthetic_state_dict

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epnp_inputs as I  # noqa: E402
from consensus_inputs import FIXTURES, MIN_INLIERS, TAU, cam, planted  # noqa: E402

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 5)
ANG_MED, ANG_MAX, POS_MED, POS_MAX = 1e-4, 0.1, 1e-5, 1e-3      # kernel against twin: tests/test_gpu_refine.py
COST_REL = 1e-5                                                  # test_gpu_refine.py's bound on 'fit'
SAMPLE_PX = 1e-6
# The cost of a pose rounded to float32 against the cost of the pose itself, measured with the twin on the ten planted
# inputs (k = 1..5, both fixtures; CS.pose_cost of its float32 'ori' / 'pos' against its 'cost'): at most 1.80e-6
# relative (1.9e-4 px^2 absolute). Ten times that:
F32_POSE_COST_REL = 1.8e-5
KEYS_OFF = {'keypoints', 'ori', 'pos', 'status'}
KEYS_REFINE = KEYS_OFF | {'ori_epnp', 'pos_epnp', 'fit', 'refine_iters'}
KEYS_ON = KEYS_REFINE | {'inliers', 'n_inliers', 'ori_consensus', 'pos_consensus'}


@pytest.fixture(scope='module')
def eng():
    from spef_amd.engine import Engine
    arch = mobilenet_v2('keypoints')
    e = Engine(Bl.pack(synthetic_state_dict(arch, seed=1001, head_std=0.002), arch, dtype='fp32'), 'cuda:0')
    assert e._kp_consensus is None and e._kp_refine is None      # off unless asked for
    yield e
    e.close()


def _configure(eng, c):
    eng.set_keypoint_refine(None)
    eng.set_keypoint_consensus(None)
    eng.set_keypoints(c['kp3d'], c['K'], c['nu'], c['nv'], c['dist'])


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items() if isinstance(v, torch.Tensor)}


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype == bool else a.view(np.uint64 if a.itemsize == 8 else np.uint32)


def _consensus(eng, kp, q, t, weights=None, **kw):
    kw.setdefault('inlier_px', TAU)
    kw.setdefault('min_inliers', MIN_INLIERS)
    return _np(eng.consensus_keypoints(_dev(kp), _dev(q), _dev(t), weights=_dev(weights), want_pose64=True, **kw))


def _epnp(eng, kp):
    e = _np(eng.decode_keypoints(_dev(kp), apply_sigmoid=False))
    assert set(e) == KEYS_OFF
    return e


def _host_errors(R, t, kp, c):
    """Squared reprojection errors [B x n] (px^2) and depths of the poses R, t in plain NumPy fp64, on the observations
    of the refinement (spe.refine.observations): nothing of the consensus twin."""
    uv = RF.observations(kp, c['K'], c['nu'], c['nv'], c['dist'])
    K = np.asarray(c['K'], np.float64).reshape(3, 3)
    Xc = np.einsum('bij,nj->bni', R, c['kp3d'].astype(np.float64)) + t[:, None, :]
    u = K[0, 0] * Xc[..., 0] / Xc[..., 2] + K[0, 2]
    v = K[1, 1] * Xc[..., 1] / Xc[..., 2] + K[1, 2]
    return (u - uv[..., 0]) ** 2 + (v - uv[..., 1]) ** 2, Xc[..., 2]


@pytest.fixture(scope='module')
def cases(eng, golden):
    """(fixture, k) -> the planted inputs, the GPU's own EPnP pose on them, the kernel's consensus from that pose and
    the twin's from the same pose; computed once."""
    cache = {}

    def get(name, k):
        if (name, k) not in cache:
            g = golden(name)
            c = cam(g)
            _configure(eng, c)
            kp, bad = planted(g, k, FIXTURES[name])
            e = _epnp(eng, kp)
            dev = _consensus(eng, kp, e['ori'], e['pos'])
            twin = CS.consensus_host(kp, inlier_px=TAU, min_inliers=MIN_INLIERS, quat=e['ori'], pos=e['pos'], **c)
            cache[(name, k)] = (g, c, kp, bad, e, dev, twin)
        return cache[(name, k)]
    return get


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('name', list(FIXTURES))
def test_kernel_equals_twin(cases, name, k):
    """Mask, inlier count and status on every row; the planted mask with them."""
    g, c, kp, bad, e, dev, twin = cases(name, k)
    assert np.array_equal(dev['inliers'], twin['inliers']) and np.array_equal(dev['inliers'], ~bad)
    assert np.array_equal(dev['n_inliers'], twin['n_inliers']) and np.array_equal(dev['status'], twin['status'])
    assert not dev['status'].any()
    assert np.array_equal(_bits(dev['weights']), _bits(twin['weights']))
    same = dev['triple'] == twin['triple']
    ang = angle_deg(dev['ori'], twin['ori'])
    dp = np.linalg.norm(dev['pos'].astype(np.float64) - twin['pos'], axis=1)
    print(f'{name} k = {k}: same triple on {same.sum()} / {len(same)} rows, same root on '
          f'{(dev["root"] == twin["root"])[same].sum()}; there angle max {ang[same].max():.2e} deg, position max '
          f'{dp[same].max():.2e} m; hypotheses scored kernel {dev["scored"].min()}..{dev["scored"].max()}, differing '
          f'from the twin on {(dev["scored"] != twin["scored"]).sum()} rows')
    assert np.median(ang[same]) < ANG_MED and ang[same].max() < ANG_MAX
    assert np.median(dp[same]) < POS_MED and dp[same].max() < POS_MAX
    assert np.abs(np.linalg.norm(dev['ori'].astype(np.float64), axis=1) - 1).max() < 2e-7
    assert np.all(np.sum(dev['ori'] * e['ori'], axis=1) >= 0)              # the start's hemisphere


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('name', list(FIXTURES))
def test_cost(cases, name, k):
    """The kernel's cost is the twin's lowest cost of the kernel's winning triple, and the twin's global minimum, both to
    a relative 1e-5: the triple may differ from the twin's only where the two tie to that bound.

    Measured on the MI355X over the ten inputs: the largest relative difference is 5.8e-8, which is the float32 of the
    output alone (the kernel's cost is bit for bit the float32 of the twin's on every row), and the kernel's triple and
    root are the twin's on 800 of 800 rows."""
    g, c, kp, bad, e, dev, twin = cases(name, k)
    own = CS.triple_cost(kp, triple=dev['triple'], inlier_px=TAU, **c)
    got = dev['cost'].astype(np.float64)
    r_own = np.abs(got - own) / own
    r_min = np.abs(got - twin['cost']) / twin['cost']
    exact = np.abs(got - own.astype(np.float32).astype(np.float64)) / own
    differ = dev['triple'] != twin['triple']
    print(f'{name} k = {k}: cost against the twin on the same triple rel max {r_own.max():.2e} (against its float32 '
          f'{exact.max():.2e}), against the twin\'s minimum {r_min.max():.2e}; other triple on {differ.sum()} rows')
    assert r_own.max() < COST_REL and r_min.max() < COST_REL


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('name', list(FIXTURES))
def test_twin_independent_facts(cases, name, k):
    """The winning hypothesis (float64, as scored) is a rotation, puts every point in front, and reprojects its own
    three sample points to 1e-6 px; the cost recomputed here from the float32 pose agrees to what that rounding
    allows (F32_POSE_COST_REL, above)."""
    g, c, kp, bad, e, dev, twin = cases(name, k)
    B, n = bad.shape
    R, t = dev['R'], dev['t']
    assert R.dtype == np.float64 and np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12
    assert np.abs(np.linalg.det(R) - 1).max() < 1e-12
    e2, z = _host_errors(R, t, kp, c)
    assert np.all(z > 0)
    tr = CS.triples(n)[dev['triple']]
    own = np.sqrt(np.take_along_axis(e2, tr, axis=1))
    cost64 = np.minimum(e2, TAU * TAU).sum(1)
    r64 = np.abs(cost64 - dev['cost']) / cost64
    q = dev['ori'].astype(np.float64)
    e2f, zf = _host_errors(RF.quat2dcm(q / np.linalg.norm(q, axis=1, keepdims=True)), dev['pos'].astype(np.float64),
                           kp, c)
    cost32 = np.minimum(e2f, TAU * TAU).sum(1)
    r32 = np.abs(cost32 - dev['cost']) / cost32
    print(f'{name} k = {k}: own sample points reproject to {own.max():.2e} px at worst; cost recomputed from the '
          f'float64 pose rel max {r64.max():.2e}, from the float32 pose {r32.max():.2e}')
    assert own.max() < SAMPLE_PX
    assert np.array_equal(e2 < TAU * TAU, dev['inliers'])
    assert r64.max() < 2.0 ** -22 and np.all(zf > 0)          # the float32 of the cost itself, and room for the sum
    assert r32.max() < F32_POSE_COST_REL
    assert np.array_equal(_bits(dev['pos']), _bits(t.astype(np.float32)))


@pytest.mark.parametrize('name', list(FIXTURES))
def test_full_path(eng, cases, name):
    """decode_keypoints with the consensus (8 px) and the refinement (50 trials, Huber 4 px) on, k = 4: the kernel chain
    against the twin chain at the kernel-against-twin bounds of test_gpu_refine.py, and the largest orientation error
    under a tenth of the same engine's with the consensus off."""
    g, c, kp, bad, e, dev, twin = cases(name, 4)
    B = len(kp)
    _configure(eng, c)
    try:
        eng.set_keypoint_refine(50, 4.0)
        off = _np(eng.decode_keypoints(_dev(kp), apply_sigmoid=False))
        eng.set_keypoint_consensus(TAU)                       # min_inliers: the default, 6 of 11
        on = _np(eng.decode_keypoints(_dev(kp), apply_sigmoid=False, want_cov=True))
    finally:
        _configure(eng, c)
    assert set(off) == KEYS_REFINE and set(on) == KEYS_ON | {'cov'}
    for key in ('keypoints', 'ori_epnp', 'pos_epnp'):
        assert np.array_equal(_bits(on[key]), _bits(off[key])), key
    assert np.array_equal(_bits(on['ori_epnp']), _bits(e['ori']))
    for key, ref in (('inliers', 'inliers'), ('n_inliers', 'n_inliers'), ('ori_consensus', 'ori'),
                     ('pos_consensus', 'pos')):
        assert np.array_equal(_bits(on[key]), _bits(dev[ref])), key      # the stage alone, bit for bit
    ref = RF.refine_pose_host(kp, twin['ori'], twin['pos'], weights=twin['weights'], max_iters=50, huber_px=4.0,
                              status=twin['status'], **c)
    ang = angle_deg(on['ori'], ref['ori'])
    dp = np.linalg.norm(on['pos'].astype(np.float64) - ref['pos'], axis=1)
    err_on, err_off = angle_deg(on['ori'], g['q'][:B]), angle_deg(off['ori'], g['q'][:B])
    print(f'{name}: chain against twin chain, angle median {np.median(ang):.2e} max {ang.max():.2e} deg, position '
          f'median {np.median(dp):.2e} max {dp.max():.2e} m; orientation error with the consensus median '
          f'{np.median(err_on):.3f} p90 {np.percentile(err_on, 90):.3f} max {err_on.max():.3f} deg, without '
          f'{np.median(err_off):.3f} / {np.percentile(err_off, 90):.3f} / {err_off.max():.3f} deg')
    assert not (on['status'] & ~32).any() and np.array_equal(on['status'] & ~32, ref['status'] & ~32)
    assert np.median(ang) < ANG_MED and ang.max() < ANG_MAX
    assert np.median(dp) < POS_MED and dp.max() < POS_MAX
    assert err_on.max() < err_off.max() / 10
    cov = on['cov'].astype(np.float64)
    assert np.all(np.isfinite(cov)) and np.all(np.diagonal(cov, axis1=1, axis2=2) > 0)


def test_no_consensus(eng, golden):
    """Eight of eleven points moved (32 rows, seed 19): bit 64 on every row, the stage leaves pose and weights as they
    came, and the decode returns exactly what it returns with the consensus off."""
    g = golden('keypoints.npz')
    c = cam(g)
    _configure(eng, c)
    kp, bad = planted(g, 8, 32, seed=19)
    e = _epnp(eng, kp)
    st = np.zeros(32, np.int32)
    st[3] = 8
    o = _consensus(eng, kp, e['ori'], e['pos'], status=_dev(st))
    twin = CS.consensus_host(kp, inlier_px=TAU, min_inliers=MIN_INLIERS, quat=e['ori'], pos=e['pos'], status=st, **c)
    assert np.array_equal(o['status'], st | 64) and np.array_equal(o['status'], twin['status'])
    assert np.array_equal(_bits(o['ori']), _bits(e['ori'])) and np.array_equal(_bits(o['pos']), _bits(e['pos']))
    assert np.all(o['weights'] == 1) and not o['inliers'].any() and not o['n_inliers'].any()
    assert np.all(np.isnan(o['cost'])) and np.all(o['triple'] == -1) and np.all(o['root'] == -1)
    assert np.all(o['scored'] > 0) and np.all(np.isnan(o['R'])) and np.all(np.isnan(o['t']))
    try:
        eng.set_keypoint_refine(50, 4.0)
        off = _np(eng.decode_keypoints(_dev(kp), apply_sigmoid=False, want_cov=True))
        eng.set_keypoint_consensus(TAU, MIN_INLIERS)
        on = _np(eng.decode_keypoints(_dev(kp), apply_sigmoid=False, want_cov=True))
    finally:
        _configure(eng, c)
    assert np.array_equal(on['status'], off['status'] | 64)
    for key in ('keypoints', 'ori', 'pos', 'ori_epnp', 'pos_epnp', 'fit', 'refine_iters', 'cov'):
        assert np.array_equal(_bits(on[key]), _bits(off[key])), key
    assert np.array_equal(_bits(on['ori_consensus']), _bits(on['ori_epnp'])) and not on['inliers'].any()


def test_status_rows_and_unscored_points(eng, cases):
    """Rows that cannot be solved get bit 64 and keep pose and weights bit for bit, their neighbours are solved as in a
    batch without them; points with weight zero are neither sampled nor inliers. All as the twin says."""
    g, c, kp, bad, e, dev, twin = cases('keypoints.npz', 3)
    _configure(eng, c)
    kp, q0, t0, bad = kp[:16].copy(), e['ori'][:16].copy(), e['pos'][:16].copy(), bad[:16]
    rng = np.random.default_rng(3)
    w = rng.uniform(0.25, 1.0, (16, 11)).astype(np.float32)
    off = np.zeros((16, 11), bool)
    for i in range(8, 16):                  # rows 8..15: two good points switched off
        off[i, rng.choice(np.nonzero(~bad[i])[0], 2, replace=False)] = True
    w[off] = 0
    kp[1, 6] = np.nan                       # a non-finite keypoint
    w[2, 3] = -1.0                          # a negative weight
    w[3, 0] = np.inf
    w[4, 2:] = 0                            # two candidates
    w[5, 6:] = 0                            # five candidates: fewer than min_inliers
    q0[6] = 0                               # no start orientation: solved all the same
    o = _consensus(eng, kp, q0, t0, weights=w)
    ref = CS.consensus_host(kp, weights=w, inlier_px=TAU, min_inliers=MIN_INLIERS, quat=q0, pos=t0, **c)
    assert list(o['status']) == [0, 64, 64, 64, 64, 64] + [0] * 10 == list(ref['status'])
    for r in range(1, 6):
        assert np.array_equal(_bits(o['ori'][r]), _bits(q0[r])) and np.array_equal(_bits(o['pos'][r]), _bits(t0[r]))
        assert np.array_equal(_bits(o['weights'][r]), _bits(w[r])) and np.isnan(o['cost'][r])
        assert list(o[k][r] for k in ('n_inliers', 'triple', 'root')) == [0, -1, -1] and not o['inliers'][r].any()
    assert [int(o['scored'][r]) for r in (1, 2, 3, 4)] == [0, 0, 0, 0] and o['scored'][5] > 0
    live = [0] + list(range(6, 16))
    assert np.array_equal(o['inliers'][live], (~bad & ~off)[live]) and np.array_equal(o['inliers'], ref['inliers'])
    assert np.array_equal(_bits(o['weights']), _bits(ref['weights']))
    assert np.array_equal(o['weights'][live], np.where(~bad & ~off, w, 0)[live])
    tr = CS.triples(11)[o['triple'][8:]]
    assert not off[np.arange(8, 16)[:, None], tr].any()
    np.testing.assert_allclose(o['cost'][live], ref['cost'][live], rtol=COST_REL)
    assert abs(abs(np.sum(o['ori'][6].astype(np.float64) * ref['ori'][6])) - 1) < 1e-6


def test_argument_and_state_errors(eng, golden):
    """The error codes of the C entry point, with nothing written."""
    from spef_amd.engine import Engine, _ptr, _stream
    g = golden('keypoints.npz')
    _configure(eng, cam(g))
    kp = _dev(planted(g, 2, 4)[0])
    q, t = _dev(g['q'][:4].astype(np.float32)), _dev(g['t'][:4].astype(np.float32))
    st = torch.zeros(4, dtype=torch.int32, device='cuda')
    wo = torch.full((4, 11), -7.0, device='cuda')
    info = torch.full((4, 4), -7, dtype=torch.int32, device='cuda')
    cost = torch.full((4,), -7.0, device='cuda')
    q0, t0 = q.clone(), t.clone()

    def call(ctx=eng.ctx, kp=kp, B=4, tau=8.0, mi=6, q=q, t=t, wo=wo, info=info, cost=cost, st=st):
        return eng.lib.spef_consensus_keypoints(ctx, _ptr(kp), None, B, tau, mi, _ptr(q), _ptr(t), _ptr(wo), _ptr(info),
                                                _ptr(cost), _ptr(st), _stream(eng.device))
    for kw in (dict(kp=None), dict(q=None), dict(t=None), dict(wo=None), dict(st=None), dict(B=0), dict(B=-3),
               dict(tau=0.0), dict(tau=-1.0), dict(tau=float('nan')), dict(tau=float('inf')), dict(mi=3), dict(mi=12),
               dict(mi=0), dict(ctx=None)):
        assert call(**kw) == L.ERR_ARG, kw
    empty = Engine(None, 'cuda:0')
    try:
        assert call(ctx=empty.ctx) == L.ERR_STATE
    finally:
        empty.close()
    torch.cuda.synchronize()
    assert torch.equal(q, q0) and torch.equal(t, t0) and not st.any().item()
    assert (wo == -7).all().item() and (info == -7).all().item() and (cost == -7).all().item()
    assert call(info=None, cost=None) == L.OK          # info and cost may be NULL
    assert call(mi=4) == L.OK
    torch.cuda.synchronize()
    assert not torch.equal(q, q0) and not st.any().item() and (info[:, 0] == 9).all().item()
    assert call(mi=11) == L.OK                         # the upper end of 4..n: nine inliers are too few
    torch.cuda.synchronize()
    assert (st == 64).all().item() and (info[:, 0] == 0).all().item()


def test_slices_equal_the_whole_batch(eng, golden):
    """B = 257 in one launch against slices of 64 (the last holds one problem) and a slice of 3, bit for bit."""
    g = golden('keypoints.npz')
    c = cam(g)
    _configure(eng, c)
    kp, bad = planted(g, 3, 257)
    e = _epnp(eng, kp)
    rng = np.random.default_rng(1)
    w = rng.uniform(0.2, 1.0, (257, 11)).astype(np.float32)
    w[rng.uniform(size=w.shape) < 0.05] = 0
    whole = _consensus(eng, kp, e['ori'], e['pos'], weights=w)
    assert np.any(whole['ori'] != e['ori']) and (whole['status'] == 0).sum() > 200
    for a, b in [(i, min(i + 64, 257)) for i in range(0, 257, 64)] + [(100, 103)]:
        part = _consensus(eng, kp[a:b], e['ori'][a:b], e['pos'][a:b], weights=w[a:b])
        for k in ('ori', 'pos', 'inliers', 'weights', 'n_inliers', 'triple', 'root', 'scored', 'cost', 'status', 'R',
                  't'):
            assert np.array_equal(_bits(part[k]), _bits(whole[k][a:b])), (k, a, b)


def test_stream_capture(eng, cases):
    """The call records into a HIP graph (no allocation in the library, no host synchronisation) and the replay gives
    the bits of the plain launch."""
    g, c, kp, bad, e, dev, twin = cases('keypoints.npz', 3)
    _configure(eng, c)
    kpd, q, t = _dev(kp), _dev(e['ori']), _dev(e['pos'])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = eng.consensus_keypoints(kpd, q, t, inlier_px=TAU, min_inliers=MIN_INLIERS, want_pose64=True)
    graph.replay()
    torch.cuda.synchronize()
    out = _np(out)
    for k in ('ori', 'pos', 'inliers', 'weights', 'n_inliers', 'triple', 'root', 'scored', 'cost', 'status', 'R', 't'):
        assert np.array_equal(_bits(out[k]), _bits(dev[k])), k


@pytest.mark.parametrize('n', (4, 16))
def test_other_models(eng, golden, n):
    """The fewest and the most points a model may have: 4 triples in one wave, 560 triples strided over 256 threads.
    n = 4: the four spanning Tango points of tests/test_gpu_epnp_shapes.py, 1 px noise, all four must be inliers.
    n = 16: epnp_inputs.case(16) at 1 px with three points per row moved 100 px. Kernel against twin, B = 64 and the
    last row alone."""
    g = golden('keypoints.npz')
    camera = I.speed_camera(g)
    q, t = I.poses(g, 'speed')
    if n == 4:
        pts = np.ascontiguousarray(g['kp3d'][[0, 2, 5, 10]], np.float32)
        kp = I.add_noise(I.project(camera, pts, q, t), camera, 1.0, 4)
        bad = np.zeros((I.B, n), bool)
    else:
        cs = I.case(g, 16, 'speed', 1.0)
        pts, kp = cs['pts'], cs['kp'].copy()
        rng = np.random.default_rng(16)
        bad = np.zeros((I.B, n), bool)
        for i in range(I.B):
            w = rng.choice(n, 3, replace=False)
            bad[i, w] = True
            phi = rng.uniform(0, 2 * np.pi, 3)
            kp[i].reshape(n + 1, 2)[w + 1] += 100.0 * np.stack([np.cos(phi) / camera.nu, np.sin(phi) / camera.nv], -1)
    c = dict(kp3d=pts, K=camera.K, nu=camera.nu, nv=camera.nv, dist=None)
    q0, t0 = q.astype(np.float32), t.astype(np.float32)
    mi = CS.default_min_inliers(n)
    _configure(eng, c)
    try:
        dev = _consensus(eng, kp, q0, t0, min_inliers=None)
        lone = _consensus(eng, kp[63:], q0[63:], t0[63:], min_inliers=mi)
    finally:
        _configure(eng, cam(g))
    twin = CS.consensus_host(kp, inlier_px=TAU, quat=q0, pos=t0, **c)
    own = CS.triple_cost(kp, triple=np.maximum(dev['triple'], 0), inlier_px=TAU, **c)
    ok = dev['status'] == 0
    rel = np.abs(dev['cost'][ok] - own[ok]) / own[ok]
    print(f'n = {n}: consensus on {ok.sum()} / {I.B} rows, inliers {dev["n_inliers"].min()}..{dev["n_inliers"].max()}, '
          f'cost rel max {rel.max():.2e}, scored {dev["scored"].min()}..{dev["scored"].max()}')
    assert np.array_equal(dev['status'], twin['status']) and ok.sum() >= 60
    assert np.array_equal(dev['inliers'], twin['inliers']) and np.array_equal(dev['n_inliers'], twin['n_inliers'])
    assert np.array_equal(dev['inliers'][ok], ~bad[ok])
    assert rel.max() < COST_REL
    np.testing.assert_allclose(dev['cost'][ok], twin['cost'][ok], rtol=COST_REL)
    assert dev['triple'].max() < n * (n - 1) * (n - 2) // 6
    for k in ('ori', 'pos', 'inliers', 'weights', 'n_inliers', 'triple', 'root', 'scored', 'cost', 'status', 'R', 't'):
        assert np.array_equal(_bits(lone[k][0]), _bits(dev[k][63])), k


def test_wiring(golden):
    """StreamPipeline.submit_keypoints equals one engine's decode bit for bit with the consensus on, SPEMi355x.predict
    carries the new keys, predict_tracked runs with it on (the tracker then gets the refinement's covariance)."""
    from spef_amd.pipeline import StreamPipeline
    from spef_amd.spe.keypoints import KeyPoints
    from spef_amd.spe.spe_utils import SPEUtils
    from spef_amd.spe_mi355x import SPEMi355x
    g = golden('keypoints.npz')
    i = int(np.argmin(np.abs(g['t'][:, 2] - np.median(g['t'][:, 2]))))
    arch = mobilenet_v2('keypoints')
    blob = Bl.pack(plant_keypoint_head(synthetic_state_dict(arch, seed=1001, head_std=2e-4), g['kp2d'][i]), arch,
                   dtype='fp16x2')
    rng = np.random.Generator(np.random.PCG64(31))
    batches = [torch.from_numpy(rng.integers(0, 256, (3, 240, 384, 3), dtype=np.uint8)).cuda() for _ in range(3)]
    pipe = StreamPipeline(blob, 'cuda:0', depth=2)
    try:
        pipe.set_keypoints(g['kp3d'], g['K'], float(g['nu']), float(g['nv']))
        pipe.set_keypoint_consensus(TAU)
        outs = [pipe.submit_keypoints(x) for x in batches]
        pipe.synchronize()
        ref = pipe.engines[0]
        for x, o in zip(batches, outs):
            r = ref.decode_keypoints(ref.forward(x)[0])
            torch.cuda.synchronize()
            assert set(r) == KEYS_ON and set(o) == KEYS_ON | {'raw', 'event'}
            for k in r:
                np.testing.assert_array_equal(o[k].cpu().numpy(), r[k].cpu().numpy(), err_msg=k)
            # (the planted head on random frames: whether a row reaches consensus is the network's matter, not the wiring's)
            none = (o['status'] & 64) != 0
            assert torch.equal(none, o['n_inliers'] == 0) and (o['n_inliers'][~none] >= MIN_INLIERS).all().item()
            assert torch.equal(o['inliers'].sum(1).int(), o['n_inliers']) and not (o['status'] & 15).any().item()
            assert (o['refine_iters'] <= 20).all().item()          # 20 trials without set_keypoint_refine
    finally:
        pipe.close()

    class Cam:
        K, nu, nv = g['K'], float(g['nu']), float(g['nv'])
    su = SPEUtils(Cam, 'keypoints', pos_mode='keypoints', keypoints_path=KeyPoints(Cam, g['kp3d']))
    x = torch.from_numpy(rng.integers(0, 256, (4, 240, 384, 3), dtype=np.uint8))
    plain = SPEMi355x(blob, 'cuda:0', su)
    spe = SPEMi355x(blob, 'cuda:0', su, keypoint_refine=(50, 4.0), keypoint_consensus=(TAU, 0))
    try:
        assert plain.keypoint_consensus is None and plain.engine._kp_consensus is None
        base, _ = plain.predict(x)
        assert set(base) == {'keypoints', 'ori', 'pos'}
        pose, _ = spe.predict(x)
        assert spe.engine._kp_consensus == (TAU, None) and spe.engine._kp_refine == (50, 4.0)
        assert set(pose) == {'keypoints', 'ori', 'pos', 'ori_epnp', 'pos_epnp', 'reproj_rms', 'inliers', 'n_inliers',
                             'ori_consensus', 'pos_consensus'}
        assert pose['inliers'].shape == (4, 11) and pose['inliers'].dtype == bool
        assert np.array_equal(pose['inliers'].sum(1), pose['n_inliers'])
        assert np.all((pose['n_inliers'] >= MIN_INLIERS) | (pose['n_inliers'] == 0))
        assert np.array_equal(_bits(pose['ori_epnp']), _bits(base['ori']))
        still, tracked, lat = spe.predict_tracked(x, n_streams=2)
        assert lat > 0 and set(still) == set(pose) and set(tracked) == {'ori', 'pos', 'mahalanobis', 'track_status'}
        assert np.all(np.isfinite(tracked['ori'])) and not (tracked['track_status'] & 1).any()
    finally:
        spe.close()
        plain.close()
