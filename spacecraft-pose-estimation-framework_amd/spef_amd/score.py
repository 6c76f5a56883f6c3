"""Host twin of the scoring kernels (csrc/k_score.hip): the statement of what they compute, in NumPy.

Per row: ``SPEUtils.get_score`` (src/spe/spe_utils.py:103-159) and the per-image error lists of ``evaluation()``
(src/tools/evaluation.py:82-85). Per log: the means, population std, median, median absolute deviation, min and max
that ``evaluation()`` (:88-99) and the temporal tool (temporal.py:27-48) report.

Arithmetic: elementwise float32 with every operation rounded on its own; every sum float64 in a fixed order, rounded to
float32 where NumPy's float32 result stood; ``acos`` / ``sqrt`` are the float64 functions rounded to float32. The
kernels follow it to the last bit except where a float64 ``acos`` / ``atan2`` lands within 1e-16 of a float32 rounding
boundary.

The fixed order of a statistics sum over a log of m slots: thread ``i`` of 256 adds slots i, i + 256, i + 512, ... in
that order (a flagged slot adds 0.0); the 256 partial sums are then combined as a balanced tree of neighbours (lanes
2k and 2k+1, then pairs of those, ...: ``block_sum256_d`` in csrc/spef_reduce.hpp).
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

ROW_FIELDS = ('pos_err', 'pos_norm', 'ori_rad', 'ori_deg', 'ori_stable')     # one log row: five float32
FLAG_DOT, FLAG_NONFINITE, FLAG_ZERO_TARGET, FLAG_STATUS = 1, 2, 4, 8        # row flags
# spef_score_finalize's fields, in order (SPEF_SCORE_FIELDS doubles per (group, track)); 'flags' = OR of the row flags
STAT_FIELDS = ('n', 'n_bad', 'n_dropped', 'ori_score', 'pos_score', 'esa_score', 'ori_error', 'pos_error', 'ori_std',
               'pos_std', 'ori_median', 'pos_median', 'ori_mad', 'pos_mad', 'ori_min', 'ori_max', 'pos_min', 'pos_max',
               'flags')
LDS_ROWS = 8192          # finalize sorts in LDS while the log's row count fits this tile, in global memory above
MAX_CAPACITY = 1 << 20
_F32 = np.float32


def _sum32(*terms: np.ndarray) -> np.ndarray:
    """float32 terms added left to right in float64, rounded to float32."""
    acc = terms[0].astype(np.float64)
    for t in terms[1:]:
        acc = acc + t.astype(np.float64)
    return acc.astype(_F32)


def _sqrt32(x: np.ndarray) -> np.ndarray:
    return np.sqrt(x.astype(np.float64)).astype(_F32)


def score_rows(q_pred, t_pred, q_true, t_true, status: Optional[np.ndarray] = None):
    """-> (rows float32 [B, 5] in ROW_FIELDS order, flags int32 [B]); a flagged row is all NaN."""
    qp, tp = np.ascontiguousarray(q_pred, _F32).reshape(-1, 4), np.ascontiguousarray(t_pred, _F32).reshape(-1, 3)
    qt, tt = np.ascontiguousarray(q_true, _F32).reshape(-1, 4), np.ascontiguousarray(t_true, _F32).reshape(-1, 3)
    B = qp.shape[0]
    assert tp.shape[0] == B and qt.shape[0] == B and tt.shape[0] == B
    with np.errstate(all='ignore'):
        d = tt - tp
        d2 = d * d
        pos_err = _sqrt32(_sum32(d2[:, 0], d2[:, 1], d2[:, 2]))
        t2 = tt * tt
        tnorm = _sqrt32(_sum32(t2[:, 0], t2[:, 1], t2[:, 2]))
        pos_norm = pos_err / tnorm
        pr = qp * qt
        dot = np.abs(_sum32(pr[:, 0], pr[:, 1], pr[:, 2], pr[:, 3]))
        ac = np.arccos(np.minimum(dot, _F32(1)).astype(np.float64)).astype(_F32)
        ori_rad = _F32(2) * ac
        ori_deg = (ori_rad * _F32(180)) / _F32(np.pi)
        # the stable angle, all float64: 2 atan2(|qp - s qt|, |qp + s qt|), s = sign(qp . qt) -- the angle between
        # the unit quaternions (oracle.decode_ref.angle_deg_stable in radians), half the rotation angle ori_rad
        a, b = qp.astype(np.float64), qt.astype(np.float64)
        pd = a * b
        dd = ((pd[:, 0] + pd[:, 1]) + pd[:, 2]) + pd[:, 3]
        s = np.where(dd < 0, -1.0, 1.0)[:, None]
        m, p = a - s * b, a + s * b
        m2, p2 = m * m, p * p
        nm = np.sqrt(((m2[:, 0] + m2[:, 1]) + m2[:, 2]) + m2[:, 3])
        npl = np.sqrt(((p2[:, 0] + p2[:, 1]) + p2[:, 2]) + p2[:, 3])
        ori_stable = (2.0 * np.arctan2(nm, npl)).astype(_F32)
        flags = np.zeros(B, np.int32)
        flags |= np.where(dot > _F32(1.01), FLAG_DOT, 0).astype(np.int32)
        finite = np.isfinite(qp).all(1) & np.isfinite(tp).all(1) & np.isfinite(qt).all(1) & np.isfinite(tt).all(1)
        flags |= np.where(finite, 0, FLAG_NONFINITE).astype(np.int32)
        flags |= np.where(tnorm == 0, FLAG_ZERO_TARGET, 0).astype(np.int32)
        if status is not None:
            flags |= np.where(np.asarray(status).reshape(-1) != 0, FLAG_STATUS, 0).astype(np.int32)
    rows = np.stack([pos_err, pos_norm, ori_rad, ori_deg, ori_stable], axis=1).astype(_F32)
    rows[flags != 0] = np.nan
    return rows, flags


def _tree_sum(x: np.ndarray) -> float:
    """The statistics kernel's float64 sum of one value per log slot (module docstring)."""
    m = x.shape[0]
    pad = np.zeros((-m) % 256, np.float64)
    v = np.concatenate([x.astype(np.float64), pad]).reshape(-1, 256)
    acc = np.zeros(256, np.float64)
    for r in v:                       # slots i, i + 256, ... in order
        acc = acc + r
    while acc.shape[0] > 1:           # neighbours, then pairs of neighbours, ...
        acc = acc[0::2] + acc[1::2]
    return float(acc[0])


def _median32(sorted_x: np.ndarray) -> float:
    n = sorted_x.shape[0]
    if n & 1:
        return _F32(sorted_x[n // 2])
    with np.errstate(all='ignore'):
        return _F32((sorted_x[n // 2 - 1] + sorted_x[n // 2]) * _F32(0.5))


def _order_stats(x: np.ndarray):
    """float32 values of the good rows -> (median, mad, min, max) as np.median / the reference's mad() give them."""
    s = np.sort(x)
    med = _median32(s)
    with np.errstate(all='ignore'):
        dev = np.sort(np.abs(x - med))
    return float(med), float(_median32(dev)), float(s[0]), float(s[-1])


def score_stats(rows: np.ndarray, flags: np.ndarray, n_dropped: int = 0) -> Dict[str, float]:
    """Statistics of one (group, track) log: ``rows`` [m, 5] / ``flags`` [m] in log order -> STAT_FIELDS."""
    rows = np.asarray(rows, _F32).reshape(-1, 5)
    flags = np.asarray(flags, np.int32).reshape(-1)
    good = flags == 0
    n = int(good.sum())
    out = {k: float('nan') for k in STAT_FIELDS}
    out.update(n=float(n), n_bad=float(rows.shape[0] - n), n_dropped=float(n_dropped),
               flags=float(np.bitwise_or.reduce(flags)) if flags.size else 0.0)
    if n == 0:
        return out
    z = np.where(good[:, None], rows, _F32(0)).astype(np.float64)
    with np.errstate(all='ignore'):
        ori_score = _tree_sum(z[:, 2]) / n
        pos_score = _tree_sum(z[:, 1]) / n
        mean_deg = _tree_sum(z[:, 3]) / n
        mean_pos = _tree_sum(z[:, 0]) / n
        do = np.where(good, z[:, 3] - mean_deg, 0.0)
        dp = np.where(good, z[:, 0] - mean_pos, 0.0)
        out.update(ori_score=ori_score, pos_score=pos_score, esa_score=ori_score + pos_score,
                   ori_error=(ori_score * 180.0) / np.pi, pos_error=mean_pos,
                   ori_std=float(np.sqrt(_tree_sum(do * do) / n)), pos_std=float(np.sqrt(_tree_sum(dp * dp) / n)))
    for tag, col in (('ori', 3), ('pos', 0)):
        med, md, lo, hi = _order_stats(rows[good, col])
        out[f'{tag}_median'], out[f'{tag}_mad'], out[f'{tag}_min'], out[f'{tag}_max'] = med, md, lo, hi
    return out


def get_score(true_pose: dict, pred_pose: dict) -> Dict[str, float]:
    """``SPEUtils.get_score`` in the specified arithmetic (raises its ValueError on a dot product above 1.01)."""
    rows, flags = score_rows(pred_pose['ori'], pred_pose['pos'], true_pose['ori'], true_pose['pos'])
    if np.any(flags & FLAG_DOT):
        raise ValueError('Intermediate sum issue due to error in model prediction (orientation)')   # spe_utils.py:138
    st = score_stats(rows, flags)
    return {k: st[k] for k in ('esa_score', 'ori_score', 'pos_score', 'ori_error', 'pos_error')}
