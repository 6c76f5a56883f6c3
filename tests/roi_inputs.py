"""Inputs shared by tests/test_roi_host.py and tests/test_gpu_roi.py (not a test module): the hand-computed cases of the
box rule, seeded tracker states and poses kept away from rounding ties, and keypoint rows for the un-mapping."""
import os

import numpy as np

from spef_amd.spe import roi as R
from spef_amd.spe import track as TK

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
HIN, WIN, H, W = 1200, 1920, 240, 384          # SPEED frames, the network input of the flagship
TIE_PX = 1e-6                                   # a value about to be rounded stays this far from a tie

# ---- a model and a camera one can project by hand: R = I puts (+-0.5, +-0.25, 0) at (960 + 100 tx +- 50, 600 + 100 ty
# +- 25) for tz = 10; the two points on the optical axis of the model keep it from being coplanar and stay inside
HAND_KP3D = np.array([[0.5, 0.25, 0], [0.5, -0.25, 0], [-0.5, 0.25, 0], [-0.5, -0.25, 0], [0, 0, 0.1], [0, 0, -0.1]],
                     np.float32)
HAND_K = np.array([[1000.0, 0, 960], [0, 1000.0, 600], [0, 0, 1]])
HAND_MARGIN, HAND_MIN_SIDE = 0.25, 32.0
_I = (1.0, 0.0, 0.0, 0.0)
_Z90 = (np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5))   # a quarter turn about the optical axis: the target stands upright
# (name, q, t, have, expected box, expected status). The tight box is 100 x 50 px about (960 + 100 tx, 600 + 100 ty);
# the margin makes it 150 x 75; the aspect 1.6 heightens it to 150 x 93.75 -> 150 x 94, x0 = floor(cx - 75 + 0.5),
# y0 = floor(cy - 46.875 + 0.5).
HAND_CASES = [
    ('centre, heightened to the aspect', _I, (0, 0, 10), 1, (885, 553, 1035, 647), 0),
    ('left edge', _I, (-9.3, 0, 10), 1, (0, 553, 150, 647), 0),             # cx = 30: x0 = -45 -> 0
    ('right edge', _I, (9.3, 0, 10), 1, (1770, 553, 1920, 647), 0),         # cx = 1890: x0 = 1815 -> 1920 - 150
    ('top edge', _I, (0, -5.8, 10), 1, (885, 0, 1035, 94), 0),              # cy = 20: y0 = -27 -> 0
    ('bottom edge', _I, (0, 5.8, 10), 1, (885, 1106, 1035, 1200), 0),       # cy = 1180: y0 = 1133 -> 1200 - 94
    # tz = 100: 10 x 5 px -> 15 x 7.5 -> both raised to 32 -> widened to 51.2 x 32 -> 51 x 32 at (960 - 25.6, 600 - 16)
    ('minimum side, then widened', _I, (0, 0, 100), 1, (934, 584, 985, 616), 0),
    # upright: 50 x 100 px -> 75 x 150 -> widened to 240 x 150 at (960 - 120, 600 - 75)
    ('aspect widened', _Z90, (0, 0, 10), 1, (840, 525, 1080, 675), 0),
    # tz = 0.7: 1428.6 px wide, 2142.9 with the margin: wider than the frame
    ('larger than the frame', _I, (0, 0, 0.7), 1, (0, 0, WIN, HIN), 1),
    ('a point behind the camera', _I, (0, 0, 0.05), 1, (0, 0, WIN, HIN), 1),   # (0, 0, -0.1) has Z = -0.05
    ('NaN position', _I, (np.nan, 0, 10), 1, (0, 0, WIN, HIN), 1),
    ('NaN quaternion', (np.nan, 0, 0, 0), (0, 0, 10), 1, (0, 0, WIN, HIN), 1),
    ('no track', _I, (0, 0, 10), 0, (0, 0, WIN, HIN), 1),
]


def fixture():
    return np.load(os.path.join(GOLDEN, 'roi.npz'), allow_pickle=False)


def near_tie(values, eps=TIE_PX):
    """Whether a value v that is rounded as floor(v + 0.5) lies within ``eps`` of a tie (v + 0.5 an integer)."""
    v = np.asarray(values, np.float64) + 0.5
    return bool(np.any(np.abs(v - np.round(v)) < eps))


def tracker_states(n_streams=3, steps=20, seed=5):
    """-> (states [steps * n_streams x 160], dropped): seeded tracker states, time-major like the rows of a video:
    Tango-sized targets 4 to 30 m away anywhere in and slightly beyond the field of view (boxes that touch the edges
    and boxes that leave the frame), rates up to 0.1 rad and 0.05 m per frame; every tenth row has no track and one in
    twenty a non-finite state. A row whose box rounds within ``TIE_PX`` of a tie (under either test camera) is drawn
    again; ``dropped`` counts those."""
    g = fixture()
    rng = np.random.default_rng(seed)
    rows, dropped = [], 0
    while len(rows) < steps * n_streams:
        st = np.zeros(TK.STATE_DOUBLES)
        st[0] = 1.0
        q = rng.normal(size=4)
        st[3:7] = q / np.linalg.norm(q)
        z = rng.uniform(4.0, 30.0)
        st[7:10] = [rng.uniform(-0.36, 0.36) * z, rng.uniform(-0.23, 0.23) * z, z]
        st[10:13] = rng.uniform(-0.1, 0.1, 3)
        st[13:16] = rng.uniform(-0.05, 0.05, 3)
        st[16:] = np.eye(12).reshape(-1)
        kind = rng.integers(0, 20)
        if kind in (0, 1):
            st[0] = 0.0
        elif kind == 2:
            st[7 + rng.integers(0, 3)] = (np.nan, np.inf)[int(rng.integers(0, 2))]
        quat, pos, have = R.predict(st[None])
        tie = False
        for K, dist in ((g['K'], None), (g['K_plus'], g['dist'])):
            r = []
            R.box_of_pose(quat[0], pos[0], g['kp3d'], K, dist, HIN, WIN, H, W, 0.2, 32.0, have[0], rounded=r)
            tie = tie or (bool(r) and near_tie(r))
        if tie:
            dropped += 1
            continue
        rows.append(st)
    return np.stack(rows), dropped


def small_target_poses(count=32, seed=9):
    """-> (q [count x 4], t [count x 3]) float32: fixture-camera poses whose ROI (margin 0.2, min side 32) is at most a
    third of the frame wide, drawn with one fixed seed -- the comparison of the same head noise with and without the
    crop."""
    g = fixture()
    rng = np.random.default_rng(seed)
    qs, ts = [], []
    while len(qs) < count:
        q = rng.normal(size=4)
        q = (q / np.linalg.norm(q)).astype(np.float32)
        z = rng.uniform(8.0, 25.0)
        t = np.array([rng.uniform(-0.2, 0.2) * z, rng.uniform(-0.12, 0.12) * z, z], np.float32)
        box, st = R.box_of_pose(q, t, g['kp3d'], g['K'], None, HIN, WIN, H, W, 0.2, 32.0)
        if st == 0 and box[2] - box[0] <= WIN // 3:
            qs.append(q)
            ts.append(t)
    return np.stack(qs), np.stack(ts)


def pil_crop_resize(frame, box, size):
    """Pillow's Image.crop(box).resize((W, H), BILINEAR) of one uint8 HWC frame -> uint8 [H x W x 3]."""
    from PIL import Image
    im = Image.fromarray(frame).crop(tuple(int(v) for v in box))
    return np.asarray(im.resize((int(size[1]), int(size[0])), Image.BILINEAR))


def frames_u8(b, h, w, seed):
    """Seeded frames with structure at every scale (noise over gradients), uint8 [b x h x w x 3], three distinct
    channels so that a channel mix-up shows."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (xx * 255.0 / max(w - 1, 1))[None, :, :, None] * np.array([1.0, 0.5, 0.25]) + \
        (yy * 255.0 / max(h - 1, 1))[None, :, :, None] * np.array([0.0, 0.5, 0.75])
    return np.clip(base * 0.5 + rng.integers(0, 128, (b, h, w, 3)), 0, 255).astype(np.uint8)
