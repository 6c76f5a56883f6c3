"""Track-guided region of interest for keypoint mode -- the NumPy twin and the specification of csrc/k_roi.hip's
prediction (``spef_track_predict``), box rule (``spef_roi_boxes``) and un-mapping (``spef_roi_unmap_keypoints``).

Where the tracker expects the target, the network sees only that part of the frame: the box of the predicted pose is
cropped and resized to the network input (``spef_preprocess_roi``: Pillow's ``crop(box).resize(BILINEAR)``, bit-exact),
and the keypoints the head gives, normalised to the crop, are mapped back to the full frame by an exact affine map. The
head's error, fixed in normalised units of its input, then costs ``box width / nu`` as many full-frame pixels.

All arithmetic is float64 in the stated order, without fused multiply-adds (the kernels compile under ``fp
contract(off)``), so the device's boxes equal these integer for integer.

``predict`` (one stream, state row of ``spe.track``: have, coast, 0, q[4], t[3], w[3], v[3], P[144]):
  have = state[0] != 0; without a track the pose is zeros. Otherwise q+ = normalise(exp([w]x) (x) q), flipped into the
  hemisphere of q, and t+ = t + v -- step 3 of ``spe.track`` -- rounded to float32. The state is not changed.

``box_of_pose`` (one row; frames ``Hin`` x ``Win``, network input ``H`` x ``W``):
 1. the row falls back to the full frame (0, 0, Win, Hin) with status bit 1 when have is 0 or q or t is not finite;
 2. R = quat2dcm(q) of the quaternion as given (``spef_amd.quaternion.quat2dcm``, squares as products); for the origin
    and then each model point p (float32 -> float64): X = ((R00 p0 + R01 p1) + R02 p2) + t0, likewise Y and Z; Z <= 0
    (or NaN) falls back; x = X / Z, y = Y / Z;
 3. with distortion (k1, k2, p1, p2, k3), the forward model of the reference's ``KeyPoints.project`` in its order of
    operations: r2 = x x + y y, cdist = ((1 + k1 r2) + (k2 r2) r2) + ((k3 r2) r2) r2,
    x' = (x cdist + ((p1 2) x) y) + p2 (r2 + (2 x) x), y' = (y cdist + p1 (r2 + (2 y) y)) + ((p2 2) x) y;
 4. u = K00 x + K02, v = K11 y + K12; a pixel that is not finite falls back;
 5. min and max of u and of v over the n + 1 points (the reference's ``create_bbox_from_keypoints`` on keypoints that
    include the origin); cx = (umin + umax) 0.5, w = umax - umin, likewise cy and h;
 6. grow: w = w + (2 margin) w, h likewise; raise: w = max(w, min_side), h likewise;
 7. aspect a = W / H: when w < h a the box is widened, w = h a, otherwise heightened, h = w / a;
 8. w + 0.5 >= Win + 1 or h + 0.5 >= Hin + 1 (or NaN) falls back; wi = floor(w + 0.5), hi = floor(h + 0.5); wi > Win or
    hi > Hin falls back;
 9. x0 = floor((cx - w 0.5) + 0.5), y0 likewise; shifted into the frame with the size kept: x0 < 0 -> 0, x0 + wi > Win
    -> Win - wi; x1 = x0 + wi, y1 = y0 + hi (exclusive).

``unmap`` (one coordinate): s = the head output, through the float32 sigmoid 1 / (1 + exp(-x)) when asked; the
keypoint is float32((lo + float64(s) (hi - lo)) / size) with (lo, hi, size) = (x0, x1, nu) for u and (y0, y1, nv) for
v. ``remap`` is the forward map, full frame -> crop, in float64.
"""
from __future__ import annotations

import math

import numpy as np

from . import track as TK

FULL_FRAME, BAD_BOX = 1, 2     # status bits of spef_roi_boxes / spef_preprocess_roi


def predict(state):
    """``state`` [S x 160] (``PoseTracker.state``) -> (quat [S x 4] float32, pos [S x 3] float32, have [S] int32)."""
    state = np.asarray(state, np.float64).reshape(-1, TK.STATE_DOUBLES)
    S = state.shape[0]
    quat, pos, have = np.zeros((S, 4), np.float32), np.zeros((S, 3), np.float32), np.zeros(S, np.int32)
    for s in range(S):
        st = state[s]
        if st[0] == 0.0:
            continue
        q, t, w, v = st[3:7], st[7:10], st[10:13], st[13:16]
        qp = TK._unit(TK.qmul(TK.qexp(w), q))
        if qp @ q < 0.0:
            qp = -qp
        quat[s], pos[s], have[s] = qp, t + v, 1
    return quat, pos, have


def _rot(q):
    q0, q1, q2, q3 = (float(x) for x in q)
    return [[2 * (q0 * q0) - 1 + 2 * (q1 * q1), 2 * q1 * q2 - 2 * q0 * q3, 2 * q1 * q3 + 2 * q0 * q2],
            [2 * q1 * q2 + 2 * q0 * q3, 2 * (q0 * q0) - 1 + 2 * (q2 * q2), 2 * q2 * q3 - 2 * q0 * q1],
            [2 * q1 * q3 - 2 * q0 * q2, 2 * q2 * q3 + 2 * q0 * q1, 2 * (q0 * q0) - 1 + 2 * (q3 * q3)]]


def project(q, t, kp3d, K, dist=None):
    """Steps 2 to 4 -> pixels [(n + 1) x 2], origin first, or None when a point has Z <= 0 or a pixel is not finite."""
    R = _rot(q)
    t0, t1, t2 = (float(x) for x in t)
    K = np.asarray(K, np.float64).reshape(3, 3)
    fu, fv, uc, vc = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    d = None if dist is None else [float(x) for x in np.asarray(dist, np.float64).reshape(-1)]
    if d is not None:
        d = d + [0.0] * (5 - len(d))
        if not any(d):
            d = None
    pts = [(0.0, 0.0, 0.0)] + [tuple(float(c) for c in p) for p in np.asarray(kp3d, np.float32).reshape(-1, 3)]
    out = []
    for p0, p1, p2 in pts:
        X = ((R[0][0] * p0 + R[0][1] * p1) + R[0][2] * p2) + t0
        Y = ((R[1][0] * p0 + R[1][1] * p1) + R[1][2] * p2) + t1
        Z = ((R[2][0] * p0 + R[2][1] * p1) + R[2][2] * p2) + t2
        if not Z > 0.0:
            return None
        x, y = X / Z, Y / Z
        if d is not None:
            xu, yu = x, y
            r2 = xu * xu + yu * yu
            cdist = ((1 + d[0] * r2) + (d[1] * r2) * r2) + ((d[4] * r2) * r2) * r2
            x = (xu * cdist + ((d[2] * 2) * xu) * yu) + d[3] * (r2 + (2 * xu) * xu)
            y = (yu * cdist + d[2] * (r2 + (2 * yu) * yu)) + ((d[3] * 2) * xu) * yu
        u, v = fu * x + uc, fv * y + vc
        if not (math.isfinite(u) and math.isfinite(v)):
            return None
        out.append((u, v))
    return np.array(out, np.float64)


def tight_box(px):
    """Step 5's extremes -> (umin, vmin, umax, vmax)."""
    return float(np.min(px[:, 0])), float(np.min(px[:, 1])), float(np.max(px[:, 0])), float(np.max(px[:, 1]))


def box_of_pose(q, t, kp3d, K, dist, Hin, Win, H, W, margin=0.2, min_side=32.0, have=1, rounded=None):
    """One row -> ((x0, y0, x1, y1), status). ``rounded``, a list, receives the four values step 8 and 9 round (before
    the + 0.5 ... floor), for the case generators that keep away from ties."""
    full = ((0, 0, int(Win), int(Hin)), FULL_FRAME)
    q = np.asarray(q, np.float32).astype(np.float64).reshape(4)
    t = np.asarray(t, np.float32).astype(np.float64).reshape(3)
    if not have or not (np.all(np.isfinite(q)) and np.all(np.isfinite(t))):
        return full
    px = project(q, t, kp3d, K, dist)
    if px is None:
        return full
    umin, vmin, umax, vmax = tight_box(px)
    margin, min_side = float(margin), float(min_side)
    cx, cy = (umin + umax) * 0.5, (vmin + vmax) * 0.5
    w, h = umax - umin, vmax - vmin
    w = w + (2 * margin) * w
    h = h + (2 * margin) * h
    w, h = max(w, min_side), max(h, min_side)
    a = float(W) / float(H)
    if w < h * a:
        w = h * a
    else:
        h = w / a
    if not (w + 0.5 < float(Win) + 1.0) or not (h + 0.5 < float(Hin) + 1.0):
        return full
    wi, hi = int(math.floor(w + 0.5)), int(math.floor(h + 0.5))
    fx0, fy0 = math.floor((cx - w * 0.5) + 0.5), math.floor((cy - h * 0.5) + 0.5)
    if rounded is not None:
        rounded[:] = [w, h, cx - w * 0.5, cy - h * 0.5]
    if wi > Win or hi > Hin or wi < 1 or hi < 1:
        return full
    x0 = 0 if fx0 < 0.0 else (Win - wi if fx0 + wi > float(Win) else int(fx0))
    y0 = 0 if fy0 < 0.0 else (Hin - hi if fy0 + hi > float(Hin) else int(fy0))
    return (x0, y0, x0 + wi, y0 + hi), 0


def boxes(quat, pos, kp3d, K, dist, Hin, Win, H, W, margin=0.2, min_side=32.0, have=None):
    """Rows -> (box [B x 4] int32, status [B] int32): ``Engine.roi_boxes``."""
    quat = np.asarray(quat, np.float32).reshape(-1, 4)
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    B = quat.shape[0]
    box, status = np.zeros((B, 4), np.int32), np.zeros(B, np.int32)
    for b in range(B):
        box[b], status[b] = box_of_pose(quat[b], pos[b], kp3d, K, dist, Hin, Win, H, W, margin, min_side,
                                        1 if have is None else int(have[b]))
    return box, status


def sigmoid32(x):
    """The head's activation in float32, as ``spef_decode_keypoints`` applies it."""
    x = np.asarray(x, np.float32)
    return (np.float32(1.0) / (np.float32(1.0) + np.exp(-x, dtype=np.float32))).astype(np.float32)


def unmap(raw, box, nu, nv, apply_sigmoid=True):
    """raw [B x 2(n+1)] (crop coordinates) -> normalised full-frame keypoints, float32: ``Engine.unmap_keypoints``."""
    raw = np.asarray(raw, np.float32)
    s = (sigmoid32(raw) if apply_sigmoid else raw).astype(np.float64)
    box = np.asarray(box, np.float64).reshape(-1, 4)
    out = np.empty_like(s)
    out[:, 0::2] = (box[:, 0:1] + s[:, 0::2] * (box[:, 2:3] - box[:, 0:1])) / float(np.float32(nu))
    out[:, 1::2] = (box[:, 1:2] + s[:, 1::2] * (box[:, 3:4] - box[:, 1:2])) / float(np.float32(nv))
    return out.astype(np.float32)


def remap(kp, box, nu, nv):
    """The forward map: normalised full-frame keypoints -> crop coordinates (float64; what a crop-trained head targets)."""
    kp = np.asarray(kp, np.float64)
    box = np.asarray(box, np.float64).reshape(-1, 4)
    out = np.empty_like(kp)
    out[:, 0::2] = (kp[:, 0::2] * float(np.float32(nu)) - box[:, 0:1]) / (box[:, 2:3] - box[:, 0:1])
    out[:, 1::2] = (kp[:, 1::2] * float(np.float32(nv)) - box[:, 1:2]) / (box[:, 3:4] - box[:, 1:2])
    return out
