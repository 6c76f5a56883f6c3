"""Multi-hypothesis orientation decode -- the NumPy twin and the specification of csrc/k_modes.hip
(``spef_decode_modes``; ``Engine.decode_modes``).

The orientation head is a soft classifier over the bins q_i of the context's table, and the decode collapses its PDF
into one Markley average. An ambiguous view puts two or more orientations into the PDF at once; their Markley average
lies between them and is none of them. This decode keeps up to ``k_max`` of them: each mode is the Markley average, the
mass and the theta block (``spe.decode_cov.theta_block``) of one cluster of bins. Which of them is the spacecraft's
orientation is for the tracker to say (``spe.track.PoseTrackerHost.step_modes``).

One row at a time, all arithmetic float64; ``p`` is float32 [n] (the decode's ``ori_soft`` or the video filter's
``ori_filt``), c = cos(sep_deg / 2) and |a . b| the absolute 4-D dot product (q and -q are one rotation):

 0. the row is invalid when ``p`` is not all finite or sum p is not positive and finite: ``modes_status`` bit 1,
    ``n_modes`` = 0, every output NaN;
 1. seeds by greedy suppression: a bin is alive while it is no seed and |q_j . q_s| < c for every seed s so far; for
    k = 0 .. k_max - 1
    take the alive bin of largest p (the float32 values compared exactly, ties to the lowest index) and stop when there
    is none, when that p <= 0, or when k > 0 and p < seed_rel * p_seed0. m_k = the seed's bin;
 2. ``rounds`` Lloyd rounds: bin i goes to the mode of largest |q_i . m_k| (ties to the lowest k); m_k becomes the top
    eigenvector of sum_{i in k} p_i q_i q_i^T (a Markley average over the cluster); a cluster whose mass is not
    positive keeps its m_k;
 3. prune: assign once more, mass_k = sum_{i in k} p_i / sum p; visit the modes by descending mass (ties to the lowest
    k) and drop one whose mass is below ``min_mass`` or not positive, or with |m_k . m_j| >= c for a mode j already
    kept (min_mass <= 1 / k_max: the heaviest mode always stays);
 4. final: assign over the survivors (kept in the order of their k), recompute m_k and mass_k, and the theta block of
    the cluster's bins about m_k (``theta_block`` of the PDF with every other bin's p set to 0) + floor_var I. The
    modes are returned by descending mass (stable), each quaternion with scalar part >= 0 (a zero scalar part: the first
    non-zero component positive).

With one surviving mode the result is the plain Markley decode of the whole PDF, with mass 1 and ``decode_cov``'s theta
block. No step looks at another row: a row's result does not depend on the batch it is in.

``margin`` (the twin only): the smallest distance of any discrete decision of the row from its threshold -- the seed
suppression (| |q_j . q_s| - c | over the bins whose p is at least the smallest seed's), the assignments (best minus
second-best |q_i . m_k| over the bins with p > 0, in every pass whose modes are no longer the seeds themselves: |q . m|
is evaluated with the same rounded operations on both sides, ``_absdot``, so against rows of the table the decision is
reproducible bit for bit, exact ties included -- and the Euler-angle grid is symmetric enough to produce them on a
large share of a PDF's mass), the seed ordering (the gaps between the float32 seed
values and the next alive candidate are exact and need none), the prune (|mass - min_mass|, | |m_k . m_j| - c |, the
gaps of the mass ordering, both there and in the final sort) and every cluster's relative eigen-gap
(l_1 - l_2) / l_1. A device row may legitimately differ from the twin where the margin is at rounding level.
"""
from __future__ import annotations

import math

import numpy as np

from .decode_cov import _sym, theta_block

MODES_MAX = 4                 # SPEF_MODES_MAX
INVALID = 1                   # modes_status bit
DEFAULTS = dict(k_max=2, sep_deg=45.0, seed_rel=0.1, min_mass=0.05, rounds=3, floor_var=0.0)


def check_params(k_max=2, sep_deg=45.0, seed_rel=0.1, min_mass=0.05, rounds=3, floor_var=0.0):
    """-> (k_max, rounds, sep_deg, seed_rel, min_mass, floor_var); AssertionError on what spef_decode_modes refuses."""
    k_max, rounds = int(k_max), int(rounds)
    sep_deg, seed_rel, min_mass, floor_var = float(sep_deg), float(seed_rel), float(min_mass), float(floor_var)
    assert 1 <= k_max <= MODES_MAX, f'k_max must be in 1..{MODES_MAX}'
    assert 0 <= rounds <= 8, 'rounds must be in 0..8'
    assert all(np.isfinite(v) for v in (sep_deg, seed_rel, min_mass, floor_var)), 'parameters must be finite'
    assert 0.0 < sep_deg <= 180.0, 'sep_deg must be in (0, 180]'
    assert 0.0 <= seed_rel <= 1.0, 'seed_rel must be in [0, 1]'
    assert 0.0 <= min_mass <= 1.0 / k_max, 'min_mass must be in [0, 1 / k_max]'
    assert floor_var >= 0.0, 'floor_var must be >= 0'
    return k_max, rounds, sep_deg, seed_rel, min_mass, floor_var


def cos_half_sep(sep_deg: float) -> float:
    """c = cos(sep / 2), evaluated as the library does (libm on the host)."""
    return math.cos(sep_deg * (math.pi / 180.0) * 0.5)


def _absdot(h, m):
    """|q_i . m| of every row: each product and sum rounded on its own, left to right (the kernel evaluates exactly
    this, without fused multiply-adds)."""
    return np.abs(((h[:, 0] * m[0] + h[:, 1] * m[1]) + h[:, 2] * m[2]) + h[:, 3] * m[3])


def canonical(q):
    """q or -q: scalar part >= 0; with a zero scalar part the first non-zero component positive."""
    for v in q:
        if v != 0.0:
            return -q if v < 0.0 else q
    return q


def _assign(h, ms, p, margin, exact=False):
    """-> (index of the mode of largest |q_i . m_k| per bin, ties to the lowest k; the margin updated). ``exact``: the
    modes are rows of the table, the decision is reproducible bit for bit and needs no margin."""
    d = np.stack([_absdot(h, m) for m in ms], axis=1)
    a = np.argmax(d, axis=1)
    if not exact and len(ms) > 1 and np.any(p > 0):
        s = np.sort(d[p > 0], axis=1)
        margin = min(margin, float((s[:, -1] - s[:, -2]).min()))
    return a, margin


def _cluster(h, p, mask):
    """-> (a = sum_{i in cluster} p_i q_i q_i^T, its mass)."""
    w = np.where(mask, p, 0.0)
    return _sym((h * w[:, None]).T @ h), float(w.sum())


def _gap(a):
    """The relative eigen-gap (l_1 - l_2) / l_1 of the symmetric a (1 when l_1 is not positive)."""
    lam = np.linalg.eigvalsh(a)
    return float((lam[-1] - lam[-2]) / lam[-1]) if lam[-1] > 0 else 1.0


def _top(a, margin):
    """-> (top eigenvector of the symmetric a, the margin with its relative eigen-gap)."""
    return np.linalg.eigh(a)[1][:, -1], min(margin, _gap(a))


def decode_modes_row(p, ori_bins, k_max=2, sep_deg=45.0, seed_rel=0.1, min_mass=0.05, rounds=3, floor_var=0.0,
                     gaps=None):
    """One row -> (quat [n_modes x 4], mass [n_modes], theta blocks [n_modes x 3 x 3], status, margin), float64.
    ``gaps`` (a list, when given) receives the relative eigen-gap of every returned mode's cluster."""
    k_max, rounds, sep_deg, seed_rel, min_mass, floor_var = check_params(k_max, sep_deg, seed_rel, min_mass, rounds,
                                                                         floor_var)
    p32 = np.asarray(p, np.float32).reshape(-1)
    h = np.asarray(ori_bins, np.float64)
    assert h.shape == (p32.size, 4), 'the PDF and the orientation table differ in length'
    p = p32.astype(np.float64)
    sp = float(p.sum()) if np.all(np.isfinite(p)) else np.nan
    if not (sp > 0.0 and sp < np.inf):
        return np.zeros((0, 4)), np.zeros(0), np.zeros((0, 3, 3)), INVALID, np.inf
    c = cos_half_sep(sep_deg)
    margin = np.inf

    # ---- 1. seeds
    alive = np.ones(p.size, bool)
    seeds = []
    for k in range(k_max):
        if not alive.any():
            break
        j = int(np.argmax(np.where(alive, p32, -np.inf)))      # the first of equal values
        if not p32[j] > 0 or (k > 0 and float(p32[j]) < seed_rel * float(p32[seeds[0]])):
            break
        seeds.append(j)
        alive &= _absdot(h, h[j]) < c
        alive[j] = False                                        # even where c rounds to 1 and |q_j . q_j| falls below it
    for s in seeds:                                             # suppression decisions that could have made a seed
        rel = p32 >= p32[seeds[-1]]
        rel[s] = False
        if rel.any():
            margin = min(margin, float(np.abs(_absdot(h[rel], h[s]) - c).min()))
    ms = [h[s].copy() for s in seeds]
    exact = True                                                # the modes are still rows of the table

    # ---- 2. Lloyd rounds
    for _ in range(rounds):
        a, margin = _assign(h, ms, p, margin, exact)
        for k in range(len(ms)):
            A, mass = _cluster(h, p, a == k)
            if mass > 0:
                ms[k], margin = _top(A, margin)
                exact = False

    # ---- 3. prune
    a, margin = _assign(h, ms, p, margin, exact)
    mass = np.array([_cluster(h, p, a == k)[1] / sp for k in range(len(ms))])
    order = np.argsort(-mass, kind='stable')
    if len(order) > 1:
        margin = min(margin, float(np.abs(np.diff(mass[order])).min()))
    kept = []
    for k in order:
        margin = min(margin, abs(mass[k] - min_mass))
        drop = mass[k] < min_mass or not mass[k] > 0
        for j in kept:
            dj = abs(float(ms[k] @ ms[j]))
            margin = min(margin, abs(dj - c))
            drop = drop or dj >= c
        if not drop:
            kept.append(int(k))
    if not kept:
        kept = [int(order[0])]
    ms = [ms[k] for k in sorted(kept)]

    # ---- 4. final
    a, margin = _assign(h, ms, p, margin, exact)
    quat, mass, blocks, gap = [], [], [], []
    for k in range(len(ms)):
        A, mk = _cluster(h, p, a == k)
        gap.append(_gap(A))
        if mk > 0:
            ms[k], margin = _top(A, margin)
        blk, _ = theta_block(np.where(a == k, p, 0.0), ms[k], h)
        quat.append(canonical(ms[k]))
        mass.append(mk / sp)
        blocks.append(blk + floor_var * np.eye(3))
    mass = np.array(mass)
    order = np.argsort(-mass, kind='stable')
    if len(order) > 1:
        margin = min(margin, float(np.abs(np.diff(mass[order])).min()))
    if gaps is not None:
        gaps[:] = [gap[k] for k in order]
    return np.array(quat)[order], mass[order], np.array(blocks)[order], 0, margin


def decode_modes_host(ori_pdf, ori_bins, k_max=2, sep_deg=45.0, seed_rel=0.1, min_mass=0.05, rounds=3, floor_var=0.0,
                      dtype=np.float32) -> dict:
    """``ori_pdf`` [B x n] float32 and the orientation table [n x 4] -> {'mode_quat' [B x k_max x 4], 'mode_mass'
    [B x k_max], 'mode_cov' [B x k_max x 3 x 3] (NaN past n_modes), 'n_modes' [B], 'modes_status' [B] int32, 'margin'
    [B] and 'eig_gap' [B x k_max] (every mode's (l_1 - l_2) / l_1) float64}, the first three rounded to ``dtype``
    (float32: what the device returns)."""
    k_max = check_params(k_max, sep_deg, seed_rel, min_mass, rounds, floor_var)[0]
    ori_pdf = np.asarray(ori_pdf, np.float32)
    ori_pdf = ori_pdf.reshape(-1, ori_pdf.shape[-1])
    B = ori_pdf.shape[0]
    out = {'mode_quat': np.full((B, k_max, 4), np.nan), 'mode_mass': np.full((B, k_max), np.nan),
           'mode_cov': np.full((B, k_max, 3, 3), np.nan), 'n_modes': np.zeros(B, np.int32),
           'modes_status': np.zeros(B, np.int32), 'margin': np.full(B, np.inf), 'eig_gap': np.full((B, k_max), np.nan)}
    for b in range(B):
        gaps = []
        q, m, blk, st, mg = decode_modes_row(ori_pdf[b], ori_bins, k_max, sep_deg, seed_rel, min_mass, rounds,
                                             floor_var, gaps)
        n = len(m)
        out['eig_gap'][b, :n] = gaps
        out['mode_quat'][b, :n], out['mode_mass'][b, :n], out['mode_cov'][b, :n] = q, m, blk
        out['n_modes'][b], out['modes_status'][b], out['margin'][b] = n, st, mg
    for k in ('mode_quat', 'mode_mass', 'mode_cov'):
        out[k] = out[k].astype(dtype)
    return out
