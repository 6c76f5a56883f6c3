"""The ROI twin (spef_amd/spe/roi.py) on the host: its projection and tight box against the reference's ``project`` and
``create_bbox_from_keypoints`` (tests/golden/roi.npz), the box rule against cases computed by hand, the tie guard of the
case generator, the prediction against the tracker's own step, and the un-mapping against its inverse."""
import numpy as np
import pytest

import roi_inputs as RI
from spef_amd.spe import roi as R
from spef_amd.spe import track as TK


@pytest.fixture(scope='module')
def fx():
    return RI.fixture()


def test_projection_and_tight_box_are_the_references(fx):
    """20 poses, 10 without and 10 with the SPEED+ distortion. The reference multiplies the pose matrix through
    np.dot (BLAS: its own summation order, possibly fused), the twin sums in a stated order: they agree to a few ulp of
    a pixel coordinate of ~1e3, far below the 1e-6 px the box rule keeps from a tie -- 1e-9 px is asserted."""
    nu, nv = float(fx['nu']), float(fx['nv'])
    for i in range(fx['q'].shape[0]):
        plus = bool(fx['plus'][i])
        px = R.project(fx['q'][i].astype(np.float64), fx['t'][i].astype(np.float64), fx['kp3d'],
                       fx['K_plus'] if plus else fx['K'], fx['dist'] if plus else None)
        assert px is not None and px.shape == (12, 2)
        assert np.max(np.abs(px - fx['px'][i])) < 1e-9, i
        # the reference's box is of float32 normalised keypoints, scaled to pixels and back in float32: three float32
        # roundings of a coordinate in [0, 1], 2^-24 relative each, off the twin's float64 extremes
        box = np.array(R.tight_box(px)) / [nu, nv, nu, nv]
        assert np.max(np.abs(box - fx['bbox'][i])) <= 3 * 2.0 ** -24, i
        # and with those roundings restated, the same numbers
        kp32 = (px / [nu, nv]).reshape(-1).astype(np.float32)
        x, y = kp32[0::2] * int(nu), kp32[1::2] * int(nv)
        ref = np.array([x.min() / int(nu), y.min() / int(nv), x.max() / int(nu), y.max() / int(nv)])
        assert np.array_equal(ref.astype(np.float64), fx['bbox'][i]), i
    assert fx['plus'].sum() == 10


def test_distortion_moves_the_projection(fx):
    i = 12
    a = R.project(fx['q'][i], fx['t'][i], fx['kp3d'], fx['K_plus'], fx['dist'])
    b = R.project(fx['q'][i], fx['t'][i], fx['kp3d'], fx['K_plus'], None)
    assert np.max(np.abs(a - b)) > 0.05


@pytest.mark.parametrize('case', RI.HAND_CASES, ids=[c[0] for c in RI.HAND_CASES])
def test_box_rule_by_hand(case):
    _, q, t, have, want, status = case
    box, st = R.box_of_pose(np.array(q, np.float32), np.array(t, np.float32), RI.HAND_KP3D, RI.HAND_K, None, RI.HIN,
                            RI.WIN, RI.H, RI.W, RI.HAND_MARGIN, RI.HAND_MIN_SIDE, have)
    assert tuple(int(v) for v in box) == want and st == status


def test_boxes_lie_in_the_frame_at_the_network_aspect():
    states, _ = RI.tracker_states()
    g = RI.fixture()
    quat, pos, have = R.predict(states)
    box, st = R.boxes(quat, pos, g['kp3d'], g['K_plus'], g['dist'], RI.HIN, RI.WIN, RI.H, RI.W, 0.2, 32.0, have)
    assert np.all(box[:, 0] >= 0) and np.all(box[:, 1] >= 0) and np.all(box[:, 2] <= RI.WIN) and np.all(box[:, 3] <= RI.HIN)
    w, h = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
    assert np.all(w >= 32) and np.all(h >= 32)
    tight = st == 0
    assert 10 <= tight.sum() < len(st) and np.all(st[have == 0] == R.FULL_FRAME)
    assert np.all(np.abs(w[tight] - h[tight] * (RI.W / RI.H)) <= 1.0 + 1e-9)   # both sides rounded: half a pixel each
    assert np.all(box[~tight] == [0, 0, RI.WIN, RI.HIN])
    # boxes that were shifted in from every edge are among them
    assert (box[tight, 0] == 0).any() or (box[tight, 1] == 0).any() or (box[tight, 2] == RI.WIN).any() or \
        (box[tight, 3] == RI.HIN).any()


def test_case_generator_drops_at_most_one_percent():
    states, dropped = RI.tracker_states()
    assert states.shape == (60, TK.STATE_DOUBLES)
    assert dropped <= 0.01 * (states.shape[0] + dropped)
    assert RI.near_tie([10.4999995]) and RI.near_tie([-3.5 + 2e-7]) and not RI.near_tie([10.49999, 7.0, 7.4])


def test_prediction_is_the_trackers_own():
    """predict = step 3 of spe.track: a tracker stepped with no valid measurement coasts to exactly that pose."""
    states, _ = RI.tracker_states()
    quat, pos, have = R.predict(states)
    trk = TK.PoseTrackerHost(states.shape[0])
    trk.set_state(states)
    ok = np.isfinite(states).all(axis=1) & (states[:, 0] != 0)
    out = trk.step(np.full((states.shape[0], 4), np.nan), np.zeros((states.shape[0], 3)))
    assert ok.sum() >= 40
    assert np.array_equal(out['ori'][ok].astype(np.float32), quat[ok])
    assert np.array_equal(out['pos'][ok].astype(np.float32), pos[ok])
    assert np.array_equal(have, (states[:, 0] != 0).astype(np.int32)) and not quat[have == 0].any()
    assert np.array_equal(trk.state()[ok], states[ok]) is False   # the step moved its state; predict read a copy
    assert np.allclose(np.linalg.norm(quat[ok].astype(np.float64), axis=1), 1.0, atol=1e-6)


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def test_unmap_and_forward_map_are_inverse_to_one_ulp():
    g = RI.fixture()
    nu, nv = float(g['nu']), float(g['nv'])
    rng = np.random.default_rng(21)
    B, nk = 64, 24
    x0 = rng.integers(0, 1500, B)
    y0 = rng.integers(0, 900, B)
    box = np.stack([x0, y0, x0 + rng.integers(32, 420, B), y0 + rng.integers(32, 300, B)], 1).astype(np.int32)
    size = np.tile([nu, nv], nk // 2)
    side = np.tile(np.stack([box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]], 1), (1, nk // 2)).astype(np.float64)
    # un-map, then the forward map: the one float32 rounding of the full-frame coordinate is all that is lost
    s = rng.uniform(0.0, 1.0, (B, nk)).astype(np.float32)
    kp = R.unmap(s, box, nu, nv, apply_sigmoid=False)
    assert kp.dtype == np.float32
    back = R.remap(kp, box, nu, nv)
    assert np.all(np.abs(back - s.astype(np.float64)) * side / size <= _ulp32(kp))
    # the forward map, then un-map: a full-frame keypoint inside its box comes back within 1 ulp
    again = R.unmap(R.remap(kp, box, nu, nv).astype(np.float32), box, nu, nv, apply_sigmoid=False)
    assert np.all(np.abs(again.astype(np.float64) - kp.astype(np.float64)) <= _ulp32(kp))
    # the full-frame box is the identity up to that rounding
    full = np.tile(np.array([[0, 0, int(nu), int(nv)]], np.int32), (B, 1))
    assert np.all(np.abs(R.unmap(s, full, nu, nv, False).astype(np.float64) - s) <= _ulp32(s))
    # and the sigmoid is the float32 one
    raw = rng.normal(0, 2, (B, nk)).astype(np.float32)
    assert np.array_equal(R.unmap(raw, full, nu, nv, True), R.unmap(R.sigmoid32(raw), full, nu, nv, False))


def test_crop_then_resize_is_not_resize_with_box():
    """Why the kernel crops first: Pillow's resize(box=...) reads pixels outside the box."""
    from PIL import Image
    fr = RI.frames_u8(1, 120, 192, seed=3)[0]
    box = (40, 30, 140, 90)
    a = RI.pil_crop_resize(fr, box, (30, 48))
    b = np.asarray(Image.fromarray(fr).resize((48, 30), Image.BILINEAR, box=box))
    assert np.abs(a.astype(int) - b.astype(int)).max() > 0
