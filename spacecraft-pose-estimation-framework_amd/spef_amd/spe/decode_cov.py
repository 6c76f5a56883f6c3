"""Pose covariance of the soft-classification decode -- the NumPy twin and the specification of csrc/k_cov.hip
(``spef_decode_cov``; ``Engine.decode_cov``).

The decode averages a PDF over the orientation bins (Markley, a = sum_i p_i q_i q_i^T) and over the position grid and
keeps the mean. What the same PDFs say about the spread around that mean is the measurement covariance the pose
tracker (``spe.track``) wants, in its own convention: order (theta, t), theta a left perturbation in the camera frame,
R = exp([theta]x) R^. All arithmetic is float64; the inputs of one row are a PDF ``p`` (float32: the decode's
``ori_soft`` / ``pos_soft``, or the video filter's filtered PDFs) and the pose it was decoded to (``q^`` renormalised
in float64, ``t^``).

  cov [6 x 6]   theta block = sum_i p_i theta_i theta_i^T / sum_i p_i + floor_var[0] I, theta_i = qlog(qmul(q_i,
                conj(q^))) with exactly ``spe.track.qlog`` / ``qmul`` (the rotation vector on the hemisphere of scalar
                part >= 0): the tracker's innovation is that Log, so the covariance is in the units the filter weighs it
                in. Every bin enters with its own p, redundant ones included, as in the Markley average.
                t block = sum_i p_i (g_i - t^)(g_i - t^)^T / sum_i p_i + floor_var[1] I over the position grid, in this
                centred form (never sum p g g^T - t^ t^^T). The cross blocks are zero.
                A head in regression mode has no PDF: its block is fixed_var[k] I (the caller passes the tracker's r).
  ori_hinv [4 x 4]  inv(a), a left unnormalised: the second value of the reference's
                OrientationSoftClassification.decode ("the uncertainty in the maximum likelihood sense",
                classification_utils.py:142), rounded to float32. Computed through the Cholesky factor of a.
  cov_status    a word of its own, never ORed into the decode status (the scorer flags any row whose decode status is
                nonzero): ORI = 1 the orientation PDF or q^ is not finite, q^ is zero or sum p <= 0 -- the theta block
                is NaN; HINV = 2 a is not positive definite to float64, i.e. a Cholesky pivot is not finite or not
                above 2^-48 of its diagonal entry (what the rounding of the sums leaves of an exact zero; a one-hot PDF,
                where the reference's np.linalg.inv raises LinAlgError) -- ori_hinv is NaN, the theta block stands;
                POS = 4 the position PDF or t^ is not finite or sum p <= 0 -- the t block is NaN.

A row with a NaN block reaches the tracker as a non-finite covariance, which it replaces by diag(r) (track.py step 4).
"""
from __future__ import annotations

import numpy as np

from .track import qmul

ORI, HINV, POS = 1, 2, 4
PIVOT_REL = 2.0 ** -48      # a Cholesky pivot at or below this fraction of its diagonal entry is zero to float64


def _sym(m) -> np.ndarray:
    """The upper triangle mirrored: symmetric bit for bit, as the kernel writes it."""
    return np.triu(m) + np.triu(m, 1).T


def markley_matrix(p, ori_bins) -> np.ndarray:
    """a = sum_i p_i q_i q_i^T in float64 (not normalised)."""
    h = np.asarray(ori_bins, np.float64)
    return (h * np.asarray(p, np.float64)[:, None]).T @ h


def chol_inverse(a):
    """-> (inv(a), ok) of the symmetric 4 x 4 ``a`` through a = L L^T; ok is False (and the inverse NaN) when a pivot
    is not finite or not above PIVOT_REL of its diagonal entry."""
    n = a.shape[0]
    L = np.zeros((n, n))
    for j in range(n):
        d = a[j, j] - L[j, :j] @ L[j, :j]
        if not (d > PIVOT_REL * a[j, j] and d < np.inf):
            return np.full((n, n), np.nan), False
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (a[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    M = np.zeros((n, n))                      # L^-1
    for c in range(n):
        M[c, c] = 1.0 / L[c, c]
        for i in range(c + 1, n):
            M[i, c] = -(L[i, c:i] @ M[c:i, c]) / L[i, i]
    return _sym(M.T @ M), True


def qlog_rows(d) -> np.ndarray:
    """``spe.track.qlog`` of every row of ``d`` [n x 4] -> [n x 3]: the same expressions, evaluated for all rows at
    once (tests/test_decode_cov_host.py holds it against the row-by-row loop bit for bit)."""
    d = np.where(d[:, :1] < 0, -d, d)
    n2 = d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2] + d[:, 3] * d[:, 3]
    n = np.sqrt(n2)
    small = n < 1e-8
    with np.errstate(divide='ignore', invalid='ignore'):
        f = np.where(small, 2.0 / d[:, 0] * (1.0 - n2 / (3.0 * d[:, 0] * d[:, 0])),
                     2.0 * np.arctan2(n, d[:, 0]) / np.where(small, 1.0, n))
    return f[:, None] * d[:, 1:]


def theta_block(p, quat, ori_bins):
    """-> (sum_i p_i theta_i theta_i^T / sum_i p_i [3 x 3], ok) of one row."""
    p = np.asarray(p, np.float64)
    q = np.asarray(quat, np.float64)
    sp, qn2 = p.sum(), float(q @ q)
    if not (np.all(np.isfinite(p)) and sp > 0 and np.all(np.isfinite(q)) and 0 < qn2 < np.inf):
        return np.full((3, 3), np.nan), False
    qc = q / np.sqrt(qn2) * [1.0, -1.0, -1.0, -1.0]
    th = qlog_rows(qmul(np.asarray(ori_bins, np.float64).T, qc).T)
    return _sym((th * p[:, None]).T @ th) / sp, True


def t_block(p, pos, pos_grid):
    """-> (sum_i p_i (g_i - t^)(g_i - t^)^T / sum_i p_i [3 x 3], ok) of one row."""
    p = np.asarray(p, np.float64)
    t = np.asarray(pos, np.float64)
    sp = p.sum()
    if not (np.all(np.isfinite(p)) and sp > 0 and np.all(np.isfinite(t))):
        return np.full((3, 3), np.nan), False
    e = np.asarray(pos_grid, np.float64) - t
    return _sym((e * p[:, None]).T @ e) / sp, True


def decode_cov_host(ori_pdf, pos_pdf, quat, pos, ori_bins=None, pos_grid=None, fixed_var=(100.0, 100.0),
                    floor_var=(0.0, 0.0), dtype=np.float32) -> dict:
    """``ori_pdf`` [B x n_ori] or None (orientation in regression mode), ``pos_pdf`` [B x n_pos] or None (position in
    regression mode), ``quat`` [B x 4], ``pos`` [B x 3], the decode tables -> {'cov' [B x 6 x 6], 'ori_hinv'
    [B x 4 x 4] (NaN without an orientation PDF), 'cov_status' [B] int32}, rounded to ``dtype`` (float32: what the
    device returns; float64: the unrounded values)."""
    fixed_var = np.asarray(fixed_var, np.float64).reshape(2)
    floor_var = np.asarray(floor_var, np.float64).reshape(2)
    assert np.all(np.isfinite(fixed_var)) and np.all(fixed_var >= 0), 'fixed_var must be finite and >= 0'
    assert np.all(np.isfinite(floor_var)) and np.all(floor_var >= 0), 'floor_var must be finite and >= 0'
    B = (quat if ori_pdf is None and pos_pdf is None else ori_pdf if ori_pdf is not None else pos_pdf).shape[0]
    cov = np.zeros((B, 6, 6))
    hinv = np.full((B, 4, 4), np.nan)
    status = np.zeros(B, np.int32)
    eye = np.eye(3)
    for b in range(B):
        if ori_pdf is None:
            cov[b, :3, :3] = fixed_var[0] * eye
        else:
            blk, ok = theta_block(ori_pdf[b], quat[b], ori_bins)
            cov[b, :3, :3] = blk + floor_var[0] * eye
            hinv[b], pd = chol_inverse(markley_matrix(ori_pdf[b], ori_bins))
            status[b] |= (0 if ok else ORI) | (0 if pd else HINV)
        if pos_pdf is None:
            cov[b, 3:, 3:] = fixed_var[1] * eye
        else:
            blk, ok = t_block(pos_pdf[b], pos[b], pos_grid)
            cov[b, 3:, 3:] = blk + floor_var[1] * eye
            status[b] |= 0 if ok else POS
    return {'cov': cov.astype(dtype), 'ori_hinv': hinv.astype(dtype), 'cov_status': status}
