"""Adaptive temporal PDF filter of the reference's ``Inference`` engine (src/temporal/pdf_compare.py:9-134).

Host NumPy, per frame: it blends the current soft-classification histogram (``pose['ori_soft']`` /
``pose['pos_soft']``, produced on the GPU by ``SPEMi355x``) with the previous filtered one, weighted by
``exp(-alpha * distance)``. Pinned to the reference by tests/golden/temporal_pdf.npz (every distance metric).
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

METRICS = ('l2', 'kl', 'js', 'hellinger', 'tv', 'wasserstein')


def _sum32(a: np.ndarray) -> np.ndarray:
    """Sum over the bins in float64, rounded to float32: where NumPy's float32 sum stands in ``TemporalPDF``."""
    return a.sum(-1, dtype=np.float64).astype(np.float32)


def _log32(r: np.ndarray) -> np.ndarray:
    """log correctly rounded to float32, as the kernel's (NumPy's own float32 log is up to 3 ulp off; the
    Kullback-Leibler / Jensen-Shannon sums of slowly moving PDFs cancel, and magnify any noise in their terms)."""
    return np.log(r.astype(np.float64)).astype(np.float32)


def _exp32(x: np.ndarray) -> np.ndarray:
    return np.exp(x.astype(np.float64)).astype(np.float32)


def _distances(p: np.ndarray, q: np.ndarray, metric: str) -> np.ndarray:
    """``TemporalPDF.compute_distance`` of rows [S, n] (already renormalised): float32 elementwise, float64 sums."""
    if metric == 'l2':
        return np.sqrt(_sum32((p - q) ** 2))
    if metric == 'kl':
        eps = np.float32(1e-12)
        ps, qs = p + eps, q + eps
        return _sum32(ps * _log32(ps / qs))
    if metric == 'js':
        mid = np.float32(0.5) * (p + q)
        a = (p * _log32(p / mid)).astype(np.float64) + (q * _log32(q / mid)).astype(np.float64)
        return np.sqrt(np.float32(0.5) * a.sum(-1).astype(np.float32))
    if metric == 'hellinger':
        return np.sqrt(np.float32(0.5) * _sum32((np.sqrt(p) - np.sqrt(q)) ** 2))
    if metric == 'tv':
        return np.float32(0.5) * _sum32(np.abs(p - q))
    if metric == 'wasserstein':                           # the cumulative sums in float64
        c = np.cumsum(p.astype(np.float64) - q.astype(np.float64), axis=-1)
        return np.abs(c).sum(-1).astype(np.float32) / np.float32(p.shape[-1])
    raise ValueError(f'Unsupported distance metric: {metric}')


def filter_sequences(pdfs: np.ndarray, n: float = 1.0, alpha: float = 1.0, metric: str = 'l2',
                     state: Optional[dict] = None) -> Tuple[np.ndarray, np.ndarray, dict]:
    """The adaptive filter over time-major sequences: ``pdfs`` [T, S, bins] holds T time steps of S independent
    streams -> (filtered PDFs [T, S, bins], distances [T, S], state). The vectorised twin of one ``TemporalPDF``
    per stream, and the host statement of what the device filter (csrc/k_video.hip, ``Engine.video_filter``)
    computes: float32 elementwise (each operation rounded on its own, exp / log correctly rounded), every sum in
    float64 rounded to float32 -- the kernel's results to the last bit, except where a float64 sum lands within
    1e-16 of a float32 rounding boundary. Cutting a sequence into calls (``state`` = the state the previous call
    returned; None = every stream reset) changes nothing.

    A frame whose sum is not a positive finite number passes through as it came with distance NaN and leaves the
    stream's state untouched, and so does the state when a blend does not sum to a positive finite number."""
    metric = metric.lower()
    if metric not in METRICS:
        raise ValueError(f'Unsupported distance metric: {metric}')
    x = np.ascontiguousarray(pdfs, np.float32)
    assert x.ndim == 3, 'pdfs must be [T, S, bins]'
    T, S, nb = x.shape
    if state is None:
        prev, sp, have = np.zeros((S, nb), np.float32), np.ones(S, np.float32), np.zeros(S, bool)
    else:
        prev, sp, have = state['pdf'].copy(), state['sum'].copy(), state['have'].copy()
        assert prev.shape == (S, nb)
    nf, af = np.float32(n), np.float32(alpha)
    out = np.empty_like(x)
    dist = np.empty((T, S), np.float32)

    def ok(v):
        return np.isfinite(v) & (v > 0)

    with np.errstate(all='ignore'):
        s1 = _sum32(x)                                    # state-independent: both normalisation sums
        cn = x / s1[..., None]
        s2 = _sum32(cn)
        good = ok(s1) & ok(s2)
        for t in range(T):
            d = _distances(cn[t] / s2[t][:, None], prev / sp[:, None], metric)
            w = _exp32(-af * d)
            w = np.where(w < 0, np.float32(0), np.where(w > 1, np.float32(1), w)).astype(np.float32)
            u = (w * nf)[:, None] * cn[t] + (np.float32(1) - w)[:, None] * prev
            su = _sum32(u)
            new = u / su[:, None]
            spn = _sum32(new)
            first = good[t] & ~have
            upd = good[t] & have
            out[t] = np.where(upd[:, None], new, np.where(first[:, None], cn[t], x[t]))
            dist[t] = np.where(upd, d, np.where(first, np.float32(0), np.float32(np.nan)))
            keep = upd & ok(su) & ok(spn)
            prev = np.where(keep[:, None], new, np.where(first[:, None], cn[t], prev))
            sp = np.where(keep, spn, np.where(first, s2[t], sp))
            have = have | first
    return out, dist, {'pdf': prev, 'sum': sp, 'have': have}


class TemporalPDF:
    """Same constructor, attributes and methods as the reference ``TemporalPDF`` (pdf_compare.py:10-22)."""

    def __init__(self, n: float = 1.0, alpha: float = 1.0, distance_metric: str = 'l2'):
        self.n = n
        self.alpha = alpha
        self.distance_metric = distance_metric.lower()
        self.previous_pdf = None

    def reset(self) -> None:
        self.previous_pdf = None

    def compute_distance(self, pdf1: np.ndarray, pdf2: np.ndarray) -> float:
        """pdf_compare.py:32-78: both PDFs renormalised, then the configured distance."""
        p = pdf1 / np.sum(pdf1)
        q = pdf2 / np.sum(pdf2)
        m = self.distance_metric
        if m == 'l2':
            return np.linalg.norm(p - q)
        if m == 'kl':
            eps = 1e-12                                   # log(0) guard, :55
            ps, qs = p + eps, q + eps
            return np.sum(ps * np.log(ps / qs))
        if m == 'js':
            mid = 0.5 * (p + q)
            return np.sqrt(0.5 * (np.sum(p * np.log(p / mid)) + np.sum(q * np.log(q / mid))))
        if m == 'hellinger':
            return np.sqrt(0.5 * np.sum((np.sqrt(p) - np.sqrt(q)) ** 2))
        if m == 'tv':
            return 0.5 * np.sum(np.abs(p - q))
        if m == 'wasserstein':                            # 1-D: L1 of the CDFs over the bin count
            return np.sum(np.abs(np.cumsum(p) - np.cumsum(q))) / len(p)
        raise ValueError(f'Unsupported distance metric: {self.distance_metric}')

    def compute_weight(self, distance: float) -> float:
        """pdf_compare.py:80-92: exp(-alpha d) clipped to [0, 1]."""
        return np.clip(np.exp(-self.alpha * distance), 0.0, 1.0)

    def update_pdf(self, current_pdf: np.ndarray) -> Tuple[np.ndarray, float]:
        """pdf_compare.py:94-134: -> (filtered PDF, distance to the previous one); the first frame passes through."""
        current_pdf = current_pdf / np.sum(current_pdf)
        if self.previous_pdf is None:
            self.previous_pdf = current_pdf
            return current_pdf, 0.0
        distance = self.compute_distance(current_pdf, self.previous_pdf)
        weight = self.compute_weight(distance)
        updated = weight * self.n * current_pdf + (1 - weight) * self.previous_pdf
        updated = updated / np.sum(updated)
        self.previous_pdf = updated
        return updated, distance
