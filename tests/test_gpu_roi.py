"""Track-guided region of interest on the GPU (csrc/k_roi.hip): the crop-and-resize against Engine.preprocess and Pillow
bit for bit, the boxes and the prediction against the NumPy twin (spef_amd/spe/roi.py) exactly, the un-mapping, what the
crop buys in front of EPnP, the loop of SPEMi355x.predict_tracked_roi against a host-driven one, and the bad arguments."""
import ctypes as C

import numpy as np
import pytest
import torch

import roi_inputs as RI
from spef_amd import _lib as L
from spef_amd import blob as Bl
from spef_amd.arch import mobilenet_v2
from spef_amd.quaternion import angle_deg
from spef_amd.spe import roi as R
from spef_amd.weights import plant_keypoint_head, synthetic_state_dict

pytestmark = pytest.mark.gpu

SMALL = (97, 131)                      # odd frame sides: rows of 393 bytes, no alignment anywhere
SIZES = [(30, 48), (23, 37)]           # one tile and partial tiles; 37 x 3 = 111 bytes per output row


@pytest.fixture(scope='module')
def fx():
    return RI.fixture()


@pytest.fixture(scope='module')
def kp_sd(golden):
    """The planted keypoint head of the bench's keypoint sub-record (weights.plant_keypoint_head)."""
    g = golden('keypoints.npz')
    i = int(np.argmin(np.abs(g['t'][:, 2] - np.median(g['t'][:, 2]))))
    return plant_keypoint_head(synthetic_state_dict(mobilenet_v2('keypoints'), seed=1001, head_std=2e-4), g['kp2d'][i])


@pytest.fixture(scope='module')
def engine(kp_sd, fx):
    from spef_amd.engine import Engine
    e = Engine(Bl.pack(kp_sd, mobilenet_v2('keypoints'), dtype='fp16x2'), 'cuda:0')
    e.set_keypoints(fx['kp3d'], fx['K'], float(fx['nu']), float(fx['nv']))
    yield e
    e.close()


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).cuda()


# ------------------------------------------------------------------------------------------------ 1, 2: the resample
@pytest.mark.parametrize('size', SIZES)
def test_full_frame_boxes_equal_preprocess(engine, size):
    fr = _dev(RI.frames_u8(3, *SMALL, seed=size[0]))
    box = _dev(np.tile([0, 0, SMALL[1], SMALL[0]], (3, 1)), np.int32)
    st = torch.full((3,), -1, dtype=torch.int32, device='cuda')
    got = engine.preprocess_roi(fr, box, size, status=st)
    want = engine.preprocess(fr, size)
    assert torch.equal(got, want) and not st.any().item()


SMALL_BOXES = [(20, 15, 101, 66),      # interior, 81 x 51
               (0, 0, 77, 60),         # touching the top-left corner
               (64, 38, 131, 97),      # touching the bottom-right corner
               (50, 40, 79, 59)]       # 29 x 19: narrower and lower than both outputs (upscaling, ksize 3)


@pytest.mark.parametrize('size', SIZES)
def test_four_boxes_equal_pillow(engine, size):
    fr = RI.frames_u8(4, *SMALL, seed=7 + size[1])
    got = engine.preprocess_roi(_dev(fr), _dev(SMALL_BOXES, np.int32), size).cpu().numpy()
    for i, box in enumerate(SMALL_BOXES):
        np.testing.assert_array_equal(got[i], RI.pil_crop_resize(fr[i], box, size), err_msg=str(box))


def test_full_size_frame_equals_pillow(engine):
    """1200 x 1920 to 240 x 384 (scale 5, ksize 11: the worst case the LDS tile is sized for): a 500 x 800 box and the
    full frame, which is also Engine.preprocess' output."""
    fr = RI.frames_u8(2, RI.HIN, RI.WIN, seed=11)
    boxes = [(611, 402, 1411, 902), (0, 0, RI.WIN, RI.HIN)]
    got = engine.preprocess_roi(_dev(fr), _dev(boxes, np.int32), (RI.H, RI.W)).cpu().numpy()
    for i, box in enumerate(boxes):
        np.testing.assert_array_equal(got[i], RI.pil_crop_resize(fr[i], box, (RI.H, RI.W)), err_msg=str(box))
    np.testing.assert_array_equal(got[1], engine.preprocess(_dev(fr[1:]), (RI.H, RI.W)).cpu().numpy()[0])


@pytest.mark.parametrize('bad', [(-1, 10, 80, 60), (10, 10, 132, 60), (10, 90, 80, 98), (40, 30, 40, 60),
                                 (60, 30, 20, 60)],
                         ids=['left of the frame', 'right of the frame', 'below the frame', 'no width', 'negative width'])
def test_caller_box_outside_the_frame_gives_zeros(engine, bad):
    fr = RI.frames_u8(3, *SMALL, seed=5)
    boxes = [SMALL_BOXES[0], bad, SMALL_BOXES[2]]
    st = torch.full((3,), -1, dtype=torch.int32, device='cuda')
    out = torch.full((3, 23, 37, 3), 9, dtype=torch.uint8, device='cuda')
    engine.preprocess_roi(_dev(fr), _dev(boxes, np.int32), (23, 37), out=out, status=st)
    got = out.cpu().numpy()
    assert st.cpu().tolist() == [0, L.ROI_BAD_BOX, 0]
    assert not got[1].any()
    for i in (0, 2):   # the neighbours stay exact
        np.testing.assert_array_equal(got[i], RI.pil_crop_resize(fr[i], boxes[i], (23, 37)))


# ------------------------------------------------------------------------------------------------ 3: boxes, prediction
def test_predict_equals_the_twin(engine):
    states, _ = RI.tracker_states(n_streams=3, steps=20)
    trk = engine.tracker(3)
    try:
        for step in range(0, 60, 3):
            rows = states[step:step + 3]
            trk.set_state(rows)
            p = trk.predict()
            q, t, have = R.predict(rows)
            np.testing.assert_array_equal(p['ori'].cpu().numpy(), q)
            np.testing.assert_array_equal(p['pos'].cpu().numpy(), t)
            np.testing.assert_array_equal(p['have'].cpu().numpy(), have)
            np.testing.assert_array_equal(trk.state().cpu().numpy(), rows)    # the state is only read
        one = trk.predict(first=1, n=2)                                       # a sub-range of the streams
        np.testing.assert_array_equal(one['ori'].cpu().numpy(), q[1:])
    finally:
        trk.close()


@pytest.mark.parametrize('camera', ['speed', 'speed_plus'])
def test_boxes_equal_the_twin(engine, fx, camera):
    K, dist = (fx['K'], None) if camera == 'speed' else (fx['K_plus'], fx['dist'])
    states, _ = RI.tracker_states(n_streams=3, steps=20)
    quat, pos, have = R.predict(states)
    engine.set_keypoints(fx['kp3d'], K, float(fx['nu']), float(fx['nv']), dist)
    try:
        box, st = engine.roi_boxes(_dev(quat), _dev(pos), (RI.HIN, RI.WIN), (RI.H, RI.W), 0.2, 32.0, have=_dev(have))
        want, wst = R.boxes(quat, pos, fx['kp3d'], K, dist, RI.HIN, RI.WIN, RI.H, RI.W, 0.2, 32.0, have)
        np.testing.assert_array_equal(box.cpu().numpy(), want)
        np.testing.assert_array_equal(st.cpu().numpy(), wst)
        assert 0 < (wst == 0).sum() < len(wst)
        # without the flag a row that had no track is a pose like any other (zeros: Z = 0, the full frame)
        box2, st2 = engine.roi_boxes(_dev(quat), _dev(pos), (RI.HIN, RI.WIN), (RI.H, RI.W), 0.2, 32.0)
        want2, wst2 = R.boxes(quat, pos, fx['kp3d'], K, dist, RI.HIN, RI.WIN, RI.H, RI.W, 0.2, 32.0)
        np.testing.assert_array_equal(box2.cpu().numpy(), want2)
        np.testing.assert_array_equal(st2.cpu().numpy(), wst2)
    finally:
        engine.set_keypoints(fx['kp3d'], fx['K'], float(fx['nu']), float(fx['nv']))


def test_hand_cases_on_the_device(engine, fx):
    engine.set_keypoints(RI.HAND_KP3D, RI.HAND_K, float(RI.WIN), float(RI.HIN))
    try:
        q = np.array([c[1] for c in RI.HAND_CASES], np.float32)
        t = np.array([c[2] for c in RI.HAND_CASES], np.float32)
        have = np.array([c[3] for c in RI.HAND_CASES], np.int32)
        box, st = engine.roi_boxes(_dev(q), _dev(t), (RI.HIN, RI.WIN), (RI.H, RI.W), RI.HAND_MARGIN, RI.HAND_MIN_SIDE,
                                   have=_dev(have))
        assert [tuple(b) for b in box.cpu().tolist()] == [c[4] for c in RI.HAND_CASES]
        assert st.cpu().tolist() == [c[5] for c in RI.HAND_CASES]
    finally:
        engine.set_keypoints(fx['kp3d'], fx['K'], float(fx['nu']), float(fx['nv']))


# ------------------------------------------------------------------------------------------------ 4: the un-mapping
def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def test_unmap_is_the_twins(engine, fx):
    nu, nv = float(fx['nu']), float(fx['nv'])
    rng = np.random.default_rng(31)
    B = 48
    x0, y0 = rng.integers(0, 1500, B), rng.integers(0, 900, B)
    box = np.stack([x0, y0, x0 + rng.integers(32, 420, B), y0 + rng.integers(32, 300, B)], 1).astype(np.int32)
    s = rng.uniform(0, 1, (B, 24)).astype(np.float32)
    got = engine.unmap_keypoints(_dev(s), _dev(box), apply_sigmoid=False).cpu().numpy()
    want = R.unmap(s, box, nu, nv, apply_sigmoid=False)
    assert np.all(np.abs(got.astype(np.float64) - want) <= _ulp32(want))
    # the sigmoid is the one spef_decode_keypoints applies: its own keypoints, mapped by the twin
    raw = rng.normal(0, 2, (B, 24)).astype(np.float32)
    got = engine.unmap_keypoints(_dev(raw), _dev(box), apply_sigmoid=True).cpu().numpy()
    sig = engine.decode_keypoints(_dev(raw), apply_sigmoid=True)['keypoints'].cpu().numpy()
    want = R.unmap(sig, box, nu, nv, apply_sigmoid=False)
    assert np.all(np.abs(got.astype(np.float64) - want) <= _ulp32(want))
    assert np.abs(sig - R.sigmoid32(raw)).max() <= 2.0 ** -23       # and that is the float32 sigmoid of the twin


def test_unmapped_noise_free_keypoints_recover_the_pose(engine, golden):
    """The EPnP known-answer bounds of tests/test_gpu_keypoints.py (5e-4 deg, 0.2 mm) on keypoints that went through
    the crop: exact projections -> crop coordinates (float32, what a head would output) -> un-mapped on the device."""
    g = golden('keypoints.npz')
    n = 96
    q, t = g['q'][:n], g['t'][:n]
    box, st = R.boxes(q, t, g['kp3d'], g['K'], None, RI.HIN, RI.WIN, RI.H, RI.W, 0.2, 32.0)
    assert (st == 0).sum() > n // 2
    kp = np.stack([R.project(q[i].astype(np.float64), t[i].astype(np.float64), g['kp3d'], g['K']).reshape(-1)
                   for i in range(n)]) / np.tile([float(g['nu']), float(g['nv'])], 12)
    s = R.remap(kp, box, float(g['nu']), float(g['nv'])).astype(np.float32)
    full = engine.unmap_keypoints(_dev(s), _dev(box), apply_sigmoid=False)
    out = engine.decode_keypoints(full, apply_sigmoid=False)
    assert not out['status'].any().item()
    assert angle_deg(out['ori'].cpu().numpy(), q).max() < 5e-4
    assert np.linalg.norm(out['pos'].cpu().numpy() - t, axis=1).max() < 2e-4


# ------------------------------------------------------------------------------------------------ 5: what it buys
def test_same_head_noise_costs_less_through_the_crop(engine, fx):
    """The head's error is fixed in normalised units of its input. The same noise (sigma 1e-3, one seed) is added once
    to full-frame keypoints and once to crop coordinates of 32 poses whose box is at most a third of the frame wide:
    after EPnP the median orientation error must be lower through the crop. The ratio is printed (DESIGN.md section 3
    records it next to the geometric ratio box width / nu); no factor is asserted."""
    nu, nv = float(fx['nu']), float(fx['nv'])
    q, t = RI.small_target_poses(32)
    box, st = R.boxes(q, t, fx['kp3d'], fx['K'], None, RI.HIN, RI.WIN, RI.H, RI.W, 0.2, 32.0)
    assert not st.any() and np.all(box[:, 2] - box[:, 0] <= RI.WIN // 3)
    kp = np.stack([R.project(q[i].astype(np.float64), t[i].astype(np.float64), fx['kp3d'], fx['K']).reshape(-1)
                   for i in range(32)]) / np.tile([nu, nv], 12)
    noise = np.random.default_rng(2024).normal(0.0, 1e-3, kp.shape)
    plain = engine.decode_keypoints(_dev((kp + noise).astype(np.float32)), apply_sigmoid=False)
    crop = (R.remap(kp, box, nu, nv) + noise).astype(np.float32)
    roi = engine.decode_keypoints(engine.unmap_keypoints(_dev(crop), _dev(box), apply_sigmoid=False),
                                  apply_sigmoid=False)
    e_plain = angle_deg(plain['ori'].cpu().numpy(), q)
    e_roi = angle_deg(roi['ori'].cpu().numpy(), q)
    geo = float(np.mean((box[:, 2] - box[:, 0]) / nu))
    print(f'median orientation error: full frame {np.median(e_plain):.4f} deg, ROI {np.median(e_roi):.4f} deg, ratio '
          f'{np.median(e_roi) / np.median(e_plain):.3f}; mean box width / nu {geo:.3f}')
    assert np.median(e_roi) < np.median(e_plain)


# ------------------------------------------------------------------------------------------------ 6: the loop
RAW, NET, S, T = (300, 480), (240, 384), 2, 4
TRACK = dict(q=(1e-4, 1e-4, 1e-4, 1e-4), p0=(1e-2, 1e-2, 1e-2, 1e-2), r=(1e-2, 1e-2))


@pytest.fixture(scope='module')
def spe(engine, fx):
    """SPEMi355x in keypoint mode on 300 x 480 raw frames: the SPEED camera at a quarter of its resolution."""
    from spef_amd.spe.keypoints import KeyPoints
    from spef_amd.spe.spe_utils import SPEUtils
    from spef_amd.spe_mi355x import SPEMi355x

    class Cam:
        K = np.diag([0.25, 0.25, 1.0]) @ fx['K']
        nu, nv = float(RAW[1]), float(RAW[0])
    su = SPEUtils(Cam, 'keypoints', pos_mode='keypoints', keypoints_path=KeyPoints(Cam, fx['kp3d']))
    m = SPEMi355x(engine, 'cuda:0', su)
    yield m, Cam
    m._close_track()
    engine.set_keypoints(fx['kp3d'], fx['K'], float(fx['nu']), float(fx['nv']))


@pytest.fixture(scope='module')
def raw_frames():
    from spef_amd.data.synthetic import synth_frames
    return torch.from_numpy(synth_frames(T * S, RAW[0], RAW[1], 40_000))


def test_loop_equals_a_host_driven_loop(spe, raw_frames, fx):
    m, Cam = spe
    eng = m.engine
    trk = m.tracker(S, **TRACK)
    trk.reset()
    still, tracked, lat = m.predict_tracked_roi(raw_frames, NET, n_streams=S, **TRACK)
    assert lat > 0 and still['roi'].shape == (T * S, 4) and still['roi'].dtype == np.int32
    assert tracked['roi'] is still['roi'] and tracked['roi_status'].shape == (T * S,)
    # the first step has no track: the full frame; later steps crop
    assert np.all(still['roi'][:S] == [0, 0, RAW[1], RAW[0]]) and np.all(still['roi_status'][:S] == L.ROI_FULL_FRAME)
    assert (still['roi_status'][S:] == 0).any()
    # the same loop driven from the host, one call per primitive and step, with the twin's prediction and boxes
    trk.reset()
    x = raw_frames.cuda()
    roi, ori, pos, tori, tpos = [], [], [], [], []
    for t in range(T):
        q, p, have = R.predict(trk.state().cpu().numpy())
        box, st = R.boxes(q, p, fx['kp3d'], Cam.K, None, RAW[0], RAW[1], NET[0], NET[1], 0.2, 32.0, have)
        small = eng.preprocess_roi(x[t * S:(t + 1) * S], _dev(box), NET)
        raw0, _ = eng.forward(small)
        dec = eng.decode_keypoints(eng.unmap_keypoints(raw0, _dev(box)), apply_sigmoid=False)
        out = trk.step(dec, 1)
        roi.append(box)
        ori.append(dec['ori'].cpu().numpy())
        pos.append(dec['pos'].cpu().numpy())
        tori.append(out['ori'].cpu().numpy())
        tpos.append(out['pos'].cpu().numpy())
    np.testing.assert_array_equal(still['roi'], np.concatenate(roi))
    np.testing.assert_array_equal(still['ori'], np.concatenate(ori))
    np.testing.assert_array_equal(still['pos'], np.concatenate(pos))
    np.testing.assert_array_equal(tracked['ori'], np.concatenate(tori))
    np.testing.assert_array_equal(tracked['pos'], np.concatenate(tpos))


def test_loop_with_every_box_fallen_back_equals_predict_frames_and_the_tracker(spe, raw_frames):
    m, _ = spe
    trk = m.tracker(S, **TRACK)
    trk.reset()
    still, tracked, _ = m.predict_tracked_roi(raw_frames, NET, n_streams=S, margin=100.0, **TRACK)
    assert np.all(still['roi'] == [0, 0, RAW[1], RAW[0]]) and np.all(still['roi_status'] == L.ROI_FULL_FRAME)
    trk.reset()
    for t in range(T):
        rows = slice(t * S, (t + 1) * S)
        pose, _ = m.predict_frames(raw_frames[rows], NET)
        np.testing.assert_array_equal(still['ori'][rows], pose['ori'])
        np.testing.assert_array_equal(still['pos'][rows], pose['pos'])
        np.testing.assert_array_equal(still['keypoints'][rows], pose['keypoints'])
        out = trk.step({'ori': _dev(pose['ori']), 'pos': _dev(pose['pos'])}, 1)
        np.testing.assert_array_equal(tracked['ori'][rows], out['ori'].cpu().numpy())
        np.testing.assert_array_equal(tracked['pos'][rows], out['pos'].cpu().numpy())


def test_loop_refuses_a_ursonet_blob(raw_frames):
    from spef_amd.engine import Engine
    from spef_amd.spe.spe_utils import SPEUtils
    from spef_amd.spe_mi355x import SPEMi355x
    su = SPEUtils(None, 'classification', 12, 3, False, 'regression')
    eng = Engine(Bl.pack(synthetic_state_dict(mobilenet_v2(), seed=1001)), 'cuda:0')
    try:
        with pytest.raises(ValueError):
            SPEMi355x(eng, 'cuda:0', su).predict_tracked_roi(raw_frames, NET)
    finally:
        eng.close()


def test_predict_sequence_tracker_roi(spe, raw_frames):
    """Inference.predict_sequence(..., 'TrackerROI') on raw frames of one stream is predict_tracked_roi's loop."""
    from spef_amd.inference import Inference
    m, _ = spe
    inf = Inference(m.engine, 'gpu_mi355x', m.spe_utils)      # an Engine passes through: the module's, shared
    try:
        inf.tracker_params = TRACK
        with pytest.raises(ValueError):
            inf.predict_sequence(raw_frames[0::S], 'TrackerROI')     # roi_size not set
        inf.roi_size = NET
        seq = inf.predict_sequence(raw_frames[0::S], 'TrackerROI')
        m.tracker(1, **TRACK).reset()
        still, tracked, _ = m.predict_tracked_roi(raw_frames[0::S], NET, 1, **TRACK)
        assert len(seq) == T
        for t, (pose_still, latency, pose_video) in enumerate(seq):
            np.testing.assert_array_equal(pose_video['ori'], tracked['ori'][t])
            np.testing.assert_array_equal(pose_video['roi'], tracked['roi'][t])
            assert latency > 0 and 'bbox' in pose_video and pose_still['roi_status'] == still['roi_status'][t]
    finally:
        inf.inference_engine._close_track()
        inf.inference_engine = None      # the engine belongs to the module's fixture: not closed here


# ------------------------------------------------------------------------------------------------ 7: bad arguments
def _vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def test_bad_arguments_come_back_through_ctypes(engine, fx):
    lib, ctx = engine.lib, engine.ctx
    B = 2
    quat = torch.zeros((B, 4), device='cuda')
    pos = torch.zeros((B, 3), device='cuda')
    box = torch.full((B, 4), -7, dtype=torch.int32, device='cuda')
    st = torch.full((B,), -7, dtype=torch.int32, device='cuda')
    fr = torch.zeros((B, 8, 8, 3), dtype=torch.uint8, device='cuda')
    out = torch.full((B, 4, 4, 3), 7, dtype=torch.uint8, device='cuda')
    raw = torch.zeros((B, 24), device='cuda')
    kp = torch.full((B, 24), -7.0, device='cuda')
    A = L.ERR_ARG

    def boxes(q=quat, p=pos, n=B, hin=RI.HIN, win=RI.WIN, h=RI.H, w=RI.W, margin=0.2, min_side=32.0, bo=box, s=st):
        return lib.spef_roi_boxes(ctx, _vp(q), _vp(p), None, n, hin, win, h, w, margin, min_side, _vp(bo), _vp(s), None)
    assert boxes(q=None) == A and boxes(p=None) == A and boxes(bo=None) == A and boxes(s=None) == A
    assert boxes(n=0) == A and boxes(hin=0) == A and boxes(w=0) == A
    assert boxes(margin=-0.1) == A and boxes(margin=float('nan')) == A and boxes(margin=float('inf')) == A
    assert boxes(min_side=0.5) == A and boxes(min_side=float('nan')) == A
    assert lib.spef_roi_boxes(None, _vp(quat), _vp(pos), None, B, 8, 8, 4, 4, 0.2, 32.0, _vp(box), _vp(st), None) == A

    def pre(f=fr, b=box, n=B, hin=8, win=8, o=out, h=4, w=4):
        return lib.spef_preprocess_roi(ctx, _vp(f), _vp(b), n, hin, win, _vp(o), h, w, None, None)
    assert pre(f=None) == A and pre(b=None) == A and pre(o=None) == A
    assert pre(n=0) == A and pre(n=65536) == A and pre(hin=0) == A and pre(w=-1) == A

    def unmap(r=raw, b=box, n=B, k=kp):
        return lib.spef_roi_unmap_keypoints(ctx, _vp(r), _vp(b), n, 1, _vp(k), None)
    assert unmap(r=None) == A and unmap(b=None) == A and unmap(k=None) == A and unmap(n=0) == A

    trk = engine.tracker(2)
    try:
        hv = torch.full((2,), -7, dtype=torch.int32, device='cuda')

        def predict(h=trk.handle, first=0, n=2, q=quat, p=pos, v=hv):
            return lib.spef_track_predict(h, first, n, _vp(q), _vp(p), _vp(v), None)
        assert predict(h=None) == A and predict(q=None) == A and predict(p=None) == A and predict(v=None) == A
        assert predict(first=-1) == A and predict(first=1, n=2) == A and predict(n=0) == A
        assert b'stream index' in lib.spef_last_error()
    finally:
        trk.close()

    # without spef_set_keypoints: SPEF_ERR_STATE
    from spef_amd.engine import Engine
    bare = Engine(Bl.pack(synthetic_state_dict(mobilenet_v2(), seed=1001)), 'cuda:0')
    try:
        assert lib.spef_roi_boxes(bare.ctx, _vp(quat), _vp(pos), None, B, RI.HIN, RI.WIN, RI.H, RI.W, 0.2, 32.0,
                                  _vp(box), _vp(st), None) == L.ERR_STATE
        assert lib.spef_roi_unmap_keypoints(bare.ctx, _vp(raw), _vp(box), B, 1, _vp(kp), None) == L.ERR_STATE
        assert b'spef_set_keypoints' in lib.spef_last_error()
    finally:
        bare.close()
    # nothing was enqueued: every output still holds what it was filled with
    torch.cuda.synchronize()
    assert (box == -7).all().item() and (st == -7).all().item() and (out == 7).all().item() and (kp == -7).all().item()
    assert (hv == -7).all().item()
