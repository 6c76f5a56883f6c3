"""GPU: the pose refinement behind EPnP (csrc/k_refine.hip) against its NumPy twin (spef_amd/spe/refine.py), and its
way up through Engine, StreamPipeline and SPEMi355x."""
import os
import sys

import numpy as np
import pytest
import torch

from spef_amd import _lib as L
from spef_amd import blob as Bl
from spef_amd.arch import mobilenet_v2
from spef_amd.quaternion import angle_deg
from spef_amd.spe import refine as RF
from spef_amd.weights import plant_keypoint_head, synthetic_state_dict

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from refine_inputs import axis_case, noisy, one_outlier, pose_errors  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURES = ('keypoints.npz', 'keypoints_speedplus.npz')
KINDS = {'noisy': 0.0, 'outlier': 4.0}      # input kind -> Huber threshold (px)
# kernel against twin: the bounds of test_epnp_matches_oracle_on_noisy_keypoints (tests/test_gpu_keypoints.py)
ANG_MED, ANG_MAX, POS_MED, POS_MAX = 1e-4, 0.1, 1e-5, 1e-3
COV_TOL = 16 * 2.0 ** -23


@pytest.fixture(scope='module')
def eng():
    from spef_amd.engine import Engine
    arch = mobilenet_v2('keypoints')
    e = Engine(Bl.pack(synthetic_state_dict(arch, seed=1001, head_std=0.002), arch, dtype='fp32'), 'cuda:0')
    assert e._kp_refine is None             # off unless asked for
    yield e
    e.close()


def _cam(g):
    return dict(kp3d=g['kp3d'], K=g['K'], nu=float(g['nu']), nv=float(g['nv']),
                dist=g['dist'] if 'dist' in g.files else None)


def _configure(eng, c):
    eng.set_keypoint_refine(None)
    eng.set_keypoints(c['kp3d'], c['K'], c['nu'], c['nv'], c['dist'])


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items() if isinstance(v, torch.Tensor)}


def _refine(eng, kp, q, t, **kw):
    return _np(eng.refine_keypoints(torch.from_numpy(np.ascontiguousarray(kp)).cuda(), torch.from_numpy(q).cuda(),
                                    torch.from_numpy(t).cuda(), want_cov=True, **kw))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope='module')
def cases(eng, golden):
    """(fixture, kind) -> the inputs, the GPU's own EPnP pose on them, the kernel's refinement from that pose and the
    twin's from the same pose, 256 problems and 50 trials each; computed once."""
    cache = {}

    def get(name, kind):
        if (name, kind) not in cache:
            g = golden(name)
            c = _cam(g)
            _configure(eng, c)
            kp = noisy(g, 3, 3.0) if kind == 'noisy' else one_outlier(g)[0]
            e = _np(eng.decode_keypoints(torch.from_numpy(kp).cuda(), apply_sigmoid=False))
            assert set(e) == {'keypoints', 'ori', 'pos', 'status'} and not e['status'].any()
            dev = _refine(eng, kp, e['ori'], e['pos'], max_iters=50, huber_px=KINDS[kind])
            twin = RF.refine_pose_host(kp, e['ori'], e['pos'], max_iters=50, huber_px=KINDS[kind], **c)
            cache[(name, kind)] = (g, kp, e, dev, twin)
        return cache[(name, kind)]
    return get


@pytest.mark.parametrize('kind', list(KINDS))
@pytest.mark.parametrize('name', FIXTURES)
def test_kernel_matches_twin(cases, name, kind):
    """(a), (c): same start (the GPU's EPnP pose), 50 trials; the cost never rises."""
    g, kp, e, dev, twin = cases(name, kind)
    ang = angle_deg(dev['ori'], twin['ori'])
    dp = np.linalg.norm(dev['pos'].astype(np.float64) - twin['pos'], axis=1)
    rel = np.abs(dev['fit'].astype(np.float64) - twin['fit']) / np.abs(twin['fit'])
    print(f'{name} {kind}: angle median {np.median(ang):.2e} max {ang.max():.2e} deg, position median '
          f'{np.median(dp):.2e} max {dp.max():.2e} m, fit rel {rel.max():.2e}, trials kernel median '
          f'{np.median(dev["iters"]):.0f} max {dev["iters"].max()}, differing from the twin in '
          f'{int((dev["iters"] != twin["iters"]).sum())} rows')
    assert not dev['status'].any() and not twin['status'].any()
    assert np.median(ang) < ANG_MED and ang.max() < ANG_MAX
    assert np.median(dp) < POS_MED and dp.max() < POS_MAX
    assert rel.max() < 1e-5
    assert np.all(dev['fit'][:, 3] <= dev['fit'][:, 2])                    # (c) exact
    assert np.all(dev['iters'] >= 1) and np.all(dev['iters'] <= 50)
    assert np.all(np.sum(dev['ori'] * e['ori'], axis=1) >= 0)              # the start's hemisphere


@pytest.mark.parametrize('name', FIXTURES)
def test_outlier_recovery(cases, name):
    """(b): one keypoint per frame moved 60 px. Huber at 4 px brings the median errors to a third of EPnP's or less."""
    g, kp, e, dev, twin = cases(name, 'outlier')
    a0, r0 = pose_errors(e['ori'], e['pos'], g)
    a1, r1 = pose_errors(dev['ori'], dev['pos'], g)
    print(f'{name}: orientation median {np.median(a0):.3f} -> {np.median(a1):.3f} deg, relative position '
          f'{np.median(r0):.2e} -> {np.median(r1):.2e}')
    assert np.median(a1) <= np.median(a0) / 3
    assert np.median(r1) <= np.median(r0) / 3


@pytest.mark.parametrize('kind', list(KINDS))
@pytest.mark.parametrize('name', FIXTURES)
def test_covariance(cases, name, kind):
    """(h): symmetric, positive diagonal, and the twin's to a relative Frobenius distance of COV_TOL.

    Measured for this tolerance: the twin run from the exact start and from a start perturbed by 1e-9, on these four
    inputs, gives covariances at most 7.6e-8 apart (relative Frobenius norm of the float32 outputs; 3e-9 to 8e-9 on
    three of the four). Ten times that, 7.6e-7, is below the floor of 16 float32 ulps = 1.9e-6 for the output cast,
    so the floor is the tolerance."""
    g, kp, e, dev, twin = cases(name, kind)
    cov, ref = dev['cov'].astype(np.float64), twin['cov'].astype(np.float64)
    assert np.array_equal(_bits(dev['cov']), _bits(dev['cov'].transpose(0, 2, 1)))
    assert np.all(np.diagonal(cov, axis1=1, axis2=2) > 0)
    rel = np.linalg.norm((cov - ref).reshape(len(cov), -1), axis=1) / np.linalg.norm(ref.reshape(len(cov), -1), axis=1)
    print(f'{name} {kind}: covariance against the twin, relative Frobenius max {rel.max():.2e}')
    assert rel.max() <= COV_TOL


@pytest.mark.parametrize('name', FIXTURES)
def test_noise_free_kat_through_decode(eng, golden, name):
    """(d): all 1,800 poses through decode_keypoints with the refinement on."""
    g = golden(name)
    _configure(eng, _cam(g))
    eng.set_keypoint_refine(50, 4.0)
    try:
        o = _np(eng.decode_keypoints(torch.from_numpy(g['kp2d']).cuda(), apply_sigmoid=False))
    finally:
        eng.set_keypoint_refine(None)
    assert set(o) == {'keypoints', 'ori', 'pos', 'status', 'ori_epnp', 'pos_epnp', 'fit', 'refine_iters'}
    assert not o['status'].any()
    assert angle_deg(o['ori'], g['q']).max() < 5e-4
    assert np.linalg.norm(o['pos'] - g['t'], axis=1).max() < 2e-4
    assert angle_deg(o['ori_epnp'], g['q']).max() < 5e-4 and np.all(o['fit'][:, 3] <= o['fit'][:, 2])


def test_off_is_off(eng, golden):
    """(e): with the refinement never configured the decode is today's -- same keys, and the arrays of a direct
    spef_decode_keypoints call, bit for bit; predict returns the three keys it always did."""
    from spef_amd.engine import _ptr, _stream
    from spef_amd.spe.keypoints import KeyPoints
    from spef_amd.spe.spe_utils import SPEUtils
    from spef_amd.spe_mi355x import SPEMi355x
    g = golden('keypoints.npz')
    _configure(eng, _cam(g))
    kp = torch.from_numpy(noisy(g, 3, 3.0, 64)).cuda()
    o = eng.decode_keypoints(kp, apply_sigmoid=False)
    assert set(o) == {'keypoints', 'ori', 'pos', 'status'}
    kpo, q, t = torch.empty_like(kp), torch.empty(64, 4, device='cuda'), torch.empty(64, 3, device='cuda')
    st = torch.empty(64, dtype=torch.int32, device='cuda')
    L.check(eng.lib.spef_decode_keypoints(eng.ctx, _ptr(kp), 64, 0, _ptr(kpo), _ptr(q), _ptr(t), _ptr(st),
                                          _stream(eng.device)))
    for k, v in (('keypoints', kpo), ('ori', q), ('pos', t)):
        assert np.array_equal(_bits(o[k].cpu().numpy()), _bits(v.cpu().numpy())), k
    assert np.array_equal(o['status'].cpu().numpy(), st.cpu().numpy())

    class Cam:
        K, nu, nv = g['K'], float(g['nu']), float(g['nv'])
    su = SPEUtils(Cam, 'keypoints', pos_mode='keypoints', keypoints_path=KeyPoints(Cam, g['kp3d']))
    x = torch.from_numpy(np.random.Generator(np.random.PCG64(9)).random((2, 3, 240, 384), dtype=np.float32))
    pose, _ = SPEMi355x(eng, 'cuda:0', su).predict(x)
    assert set(pose) == {'keypoints', 'ori', 'pos'}
    try:   # one trial: every row stops at max_iters (bit 32), which predict must not raise on
        fine, _ = SPEMi355x(eng, 'cuda:0', su, keypoint_refine=(1, 4.0)).predict(x)
    finally:
        eng.set_keypoint_refine(None)
    assert set(fine) == {'keypoints', 'ori', 'pos', 'ori_epnp', 'pos_epnp', 'reproj_rms'}
    assert np.array_equal(_bits(fine['ori_epnp']), _bits(pose['ori'])) and fine['reproj_rms'].shape == (2, 2)
    assert np.array_equal(_bits(fine['keypoints']), _bits(pose['keypoints']))


def test_slices_equal_the_whole_batch(eng, golden):
    """(f): B = 257 in one launch against slices of 64 (the last holds one problem) and a slice of 3."""
    g = golden('keypoints.npz')
    _configure(eng, _cam(g))
    kp = noisy(g, 3, 3.0, 257)
    e = _np(eng.decode_keypoints(torch.from_numpy(kp).cuda(), apply_sigmoid=False))
    rng = np.random.default_rng(1)
    w = rng.uniform(0.2, 1.0, (257, 11)).astype(np.float32)
    whole = _refine(eng, kp, e['ori'], e['pos'], weights=torch.from_numpy(w), max_iters=50, huber_px=4.0)
    assert np.any(whole['ori'] != e['ori'])
    for a, b in [(i, min(i + 64, 257)) for i in range(0, 257, 64)] + [(100, 103)]:
        part = _refine(eng, kp[a:b], e['ori'][a:b], e['pos'][a:b], weights=torch.from_numpy(w[a:b]), max_iters=50,
                       huber_px=4.0)
        for k in ('ori', 'pos', 'fit', 'cov', 'iters', 'status'):
            assert np.array_equal(_bits(part[k]), _bits(whole[k][a:b])), (k, a, b)


def test_status_rows(eng, golden):
    """(g): rows that cannot be refined get bit 16 and keep their pose bit for bit, their neighbours are refined as in
    a batch without them; one trial on a noisy row sets bit 32."""
    g = golden('keypoints.npz')
    c = _cam(g)
    _configure(eng, c)
    kp = noisy(g, 5, 3.0, 8)
    q0, t0 = g['q'][:8].astype(np.float32), g['t'][:8].astype(np.float32)
    clean = _refine(eng, kp, q0, t0, max_iters=50, huber_px=4.0)
    kp[1, 6] = np.nan
    t0[2, 2] = -t0[2, 2]
    st = np.zeros(8, np.int32)
    st[3] = 8
    w = np.ones((8, 11), np.float32)
    w[4, 2:] = 0
    w[5, 0] = np.inf
    q0[6] = 0
    o = _refine(eng, kp, q0, t0, weights=torch.from_numpy(w), max_iters=50, huber_px=4.0,
                status=torch.from_numpy(st).cuda())
    twin = RF.refine_pose_host(kp, q0, t0, weights=w, max_iters=50, huber_px=4.0, status=st, **c)
    assert list(o['status']) == [0, 16, 16, 24, 16, 16, 16, 0] == list(twin['status'])
    for r in range(1, 7):
        assert np.array_equal(_bits(o['ori'][r]), _bits(q0[r])) and np.array_equal(_bits(o['pos'][r]), _bits(t0[r]))
        assert np.all(np.isnan(o['fit'][r])) and np.all(np.isnan(o['cov'][r])) and o['iters'][r] == 0
    for r in (0, 7):
        for k in ('ori', 'pos', 'fit', 'cov', 'iters'):
            assert np.array_equal(_bits(o[k][r]), _bits(clean[k][r])), (k, r)
        assert o['fit'][r, 3] < o['fit'][r, 2]
    one = _refine(eng, kp[:1], q0[:1], t0[:1], max_iters=1, huber_px=4.0)
    assert one['status'][0] == 32 and one['iters'][0] == 1


def test_argument_and_state_errors(eng, golden):
    """(g): the error codes of the C entry point, with nothing written."""
    from spef_amd.engine import Engine, _ptr, _stream
    g = golden('keypoints.npz')
    _configure(eng, _cam(g))
    kp = torch.from_numpy(noisy(g, 3, 3.0, 4)).cuda()
    q, t = torch.from_numpy(g['q'][:4].astype(np.float32)).cuda(), torch.from_numpy(g['t'][:4].astype(np.float32)).cuda()
    st = torch.zeros(4, dtype=torch.int32, device='cuda')
    q0, t0 = q.clone(), t.clone()

    def call(ctx=eng.ctx, kp=kp, B=4, it=50, hub=4.0, q=q, t=t, st=st):
        return eng.lib.spef_refine_keypoints(ctx, _ptr(kp), None, B, it, hub, _ptr(q), _ptr(t), None, None, None,
                                             _ptr(st), _stream(eng.device))
    for kw in (dict(kp=None), dict(q=None), dict(t=None), dict(st=None), dict(B=0), dict(B=-3), dict(it=0),
               dict(it=101), dict(hub=-1.0), dict(hub=float('nan')), dict(hub=float('inf')), dict(ctx=None)):
        assert call(**kw) == L.ERR_ARG, kw
    empty = Engine(None, 'cuda:0')
    try:
        assert call(ctx=empty.ctx) == L.ERR_STATE
    finally:
        empty.close()
    torch.cuda.synchronize()
    assert torch.equal(q, q0) and torch.equal(t, t0) and not st.any().item()
    assert call() == L.OK                   # fit, cov and iters may be NULL
    torch.cuda.synchronize()
    assert not torch.equal(q, q0) and not st.any().item()


def _synthetic_model(golden, n):
    """n = 4: four Tango points that span space; n = 16: the 11 Tango points and 5 seeded ones."""
    g = golden('keypoints.npz')
    if n == 4:
        pts = g['kp3d'][[0, 2, 5, 10]]
    else:
        pts = np.concatenate([g['kp3d'], np.random.default_rng(16).uniform(-0.5, 0.5, (n - 11, 3)).astype(np.float32)])
    assert np.linalg.svd(pts - pts.mean(0), compute_uv=False).min() > 0.05
    return g, np.ascontiguousarray(pts, np.float32)


@pytest.mark.parametrize('n', (4, 16))
def test_lane_bounds(eng, golden, n):
    """The fewest and the most points a problem may have (EPNP_MAXN = 16), projected by KeyPoints.project, 1 px noise,
    started from the true pose: kernel against twin at the bounds of (a), B = 64 and B = 1."""
    from spef_amd.spe.keypoints import KeyPoints
    g, pts = _synthetic_model(golden, n)

    class Cam:
        K, nu, nv = g['K'], float(g['nu']), float(g['nv'])
    kps = KeyPoints(Cam, pts)
    rng = np.random.default_rng(n)
    kp = np.stack([kps.create_keypoints2d(g['q'][i], g['t'][i]) for i in range(64)])
    kp = (kp + rng.normal(0, 1.0, kp.shape) / np.tile([Cam.nu, Cam.nv], n + 1)).astype(np.float32)
    q0, t0 = g['q'][:64].astype(np.float32), g['t'][:64].astype(np.float32)
    c = dict(kp3d=pts, K=g['K'], nu=Cam.nu, nv=Cam.nv, dist=None)
    _configure(eng, c)
    try:
        dev = _refine(eng, kp, q0, t0, max_iters=50, huber_px=4.0)
        lone = _refine(eng, kp[63:], q0[63:], t0[63:], max_iters=50, huber_px=4.0)
    finally:
        _configure(eng, _cam(g))
    twin = RF.refine_pose_host(kp, q0, t0, max_iters=50, huber_px=4.0, **c)
    ang = angle_deg(dev['ori'], twin['ori'])
    dp = np.linalg.norm(dev['pos'].astype(np.float64) - twin['pos'], axis=1)
    print(f'n = {n}: angle max {ang.max():.2e} deg, position max {dp.max():.2e} m, trials max {dev["iters"].max()}')
    assert not (dev['status'] & 16).any() and np.array_equal(dev['status'], twin['status'])
    assert np.median(ang) < ANG_MED and ang.max() < ANG_MAX and np.median(dp) < POS_MED and dp.max() < POS_MAX
    assert np.all(dev['fit'][:, 3] < dev['fit'][:, 2])
    assert np.abs(dev['fit'].astype(np.float64) - twin['fit']).max() <= 1e-5 * np.abs(twin['fit']).max()
    for k in ('ori', 'pos', 'fit', 'cov', 'iters', 'status'):
        assert np.array_equal(_bits(lone[k][0]), _bits(dev[k][63])), k


def test_zero_accept_returns_the_input_bit_for_bit(eng, golden):
    """Every trial rejected (refine_inputs.axis_case: a zero pivot under any damping): the pose keeps the input's bits,
    the run ends when the damping passes 1e12, and the covariance of the singular normal matrix is NaN."""
    kp3d, K, kp, w, q0, t0 = axis_case()
    _configure(eng, dict(kp3d=kp3d, K=K, nu=1920.0, nv=1200.0, dist=None))
    try:
        o = _refine(eng, kp, q0, t0, weights=torch.from_numpy(w), max_iters=50, huber_px=0.0)
    finally:
        _configure(eng, _cam(golden('keypoints.npz')))
    twin = RF.refine_pose_host(kp, q0, t0, kp3d, K, 1920.0, 1200.0, weights=w, max_iters=50, huber_px=0.0)
    assert np.array_equal(_bits(o['ori']), _bits(q0)) and np.array_equal(_bits(o['pos']), _bits(t0))
    assert not o['status'].any() and np.array_equal(o['iters'], twin['iters'])
    assert np.all(o['fit'][:, 3] == o['fit'][:, 2]) and np.all(np.isnan(o['cov']))
    np.testing.assert_allclose(o['fit'], twin['fit'], rtol=1e-5)


def test_pipeline_matches_single_engine(golden):
    """(i): StreamPipeline.submit_keypoints with the refinement on, three streams, B = 3 frames at 240 x 384: every
    output of every batch equals one engine's on one stream, bit for bit; the scorer hook takes the refined pose and
    does not read the informational bits as decode failures."""
    from spef_amd.pipeline import StreamPipeline
    from spef_amd.score import FLAG_STATUS
    g = golden('keypoints.npz')
    i = int(np.argmin(np.abs(g['t'][:, 2] - np.median(g['t'][:, 2]))))
    arch = mobilenet_v2('keypoints')
    sd = plant_keypoint_head(synthetic_state_dict(arch, seed=1001, head_std=2e-4), g['kp2d'][i])
    rng = np.random.Generator(np.random.PCG64(31))
    batches = [torch.from_numpy(rng.integers(0, 256, (3, 240, 384, 3), dtype=np.uint8)).cuda() for _ in range(4)]
    pipe = StreamPipeline(Bl.pack(sd, arch, dtype='fp16x2'), 'cuda:0', depth=3)
    try:
        pipe.set_keypoints(g['kp3d'], g['K'], float(g['nu']), float(g['nv']))
        pipe.set_keypoint_refine(50, 4.0)
        outs = [pipe.submit_keypoints(x) for x in batches]
        pipe.synchronize()
        ref = pipe.engines[0]
        for x, o in zip(batches, outs):
            raw, _ = ref.forward(x)
            r = ref.decode_keypoints(raw)
            torch.cuda.synchronize()
            assert set(r) == {'keypoints', 'ori', 'pos', 'status', 'ori_epnp', 'pos_epnp', 'fit', 'refine_iters'}
            np.testing.assert_array_equal(o['raw'].cpu().numpy(), raw.cpu().numpy())
            for k in r:
                np.testing.assert_array_equal(o[k].cpu().numpy(), r[k].cpu().numpy(), err_msg=k)
            assert not (o['status'] & 16).any().item() and (o['fit'][:, 3] < o['fit'][:, 2]).all().item()
        # the scorer hook: one trial leaves bit 32 on every row, which is no decode failure; the scored pose is the
        # refined one (its error against itself is zero, EPnP's is not)
        pipe.set_keypoint_refine(1, 4.0)
        want = ref.decode_keypoints(ref.forward(batches[0])[0])
        torch.cuda.synchronize()
        assert (want['status'] == 32).all().item() and not torch.equal(want['ori'], want['ori_epnp'])
        scorer = pipe.engine.scorer(1, 1, 16)
        try:
            pipe.submit_keypoints(batches[0], score=(scorer, {'ori': want['ori'].cpu().numpy(),
                                                              'pos': want['pos'].cpu().numpy()}))
            res = scorer.result()
        finally:
            scorer.close()
        assert not int(res['flags'][0, 0]) & FLAG_STATUS
        assert res['pos_error'][0, 0] == 0.0
    finally:
        pipe.close()
