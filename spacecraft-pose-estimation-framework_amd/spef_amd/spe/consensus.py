"""Outlier-robust keypoint decode: exhaustive 3-point consensus. The NumPy fp64 twin of ``csrc/k_consensus.hip``.

EPnP (csrc/k_epnp.hip) weighs every keypoint equally and the refinement behind it (spe/refine.py) starts from EPnP's
pose, so two or more bad keypoints can put the start outside Huber's basin. This stage sits between the two: a model of
n <= 16 points has at most C(16, 3) = 560 minimal samples, so every triple of candidate points is solved (P3P, Grunert's
quartic in the form of Haralick et al. 1994) and every hypothesis is scored on all candidates with a truncated squared
reprojection error. No sampling, no seed; the result of a problem does not depend on the batch it is in. The kernel
and this module state one algorithm with the same constants; ``consensus_host`` is the host path and the kernel's
reference in the tests, vectorised over the batch, the triples and the roots.

Per problem:
  observations  ``refine.observations`` (what EPnP and the refinement solve on); bearings f = (x, y, 1) / |.|.
  candidates    points with confidence c > 0 (all of them without ``weights``).
  samples       all triples i < j < k of the model, in lexicographic order (the triple's index is its rank among all
                C(n, 3)); a triple with a point that is no candidate, or whose model triangle is degenerate
                (|(Xj - Xi) x (Xk - Xi)| <= 1e-6 (longest edge)^2), is skipped.
  solve         the quartic's real roots in closed form (Ferrari: the largest real root of the resolvent cubic by
                Cardano / the trigonometric form, two Newton steps on the cubic, two quadratics), two Newton steps on
                the original quartic, roots sorted ascending; for each root v > 0 with u > 0 the three distances,
                two Newton steps on the law-of-cosines equations they solve (the hypothesis then reprojects its own
                sample to 1e-9 px; without them u = N(v) / D(v) leaves up to 4e-3 px where D is small), and the pose
                from the two congruent triangles (orthonormal triads, no SVD).
  score         valid only if every model point has Z > 0; cost = sum over candidates of min(e^2, tau^2); the lowest
                cost wins, ties go to the lowest triple index, then to the lowest root.
  accept        at least ``min_inliers`` candidates with e^2 < tau^2.

Status bit ``NO_CONSENSUS`` = 64 (ORed into the status word handed in; informational, like the refinement's 16 and
32): a non-finite keypoint or weight, a negative weight, fewer than 3 candidates, no valid hypothesis, or fewer
inliers than ``min_inliers``. Such a row keeps its pose bit for bit, its weights are the input confidences (or 1),
its cost is NaN, and its triple and root are -1.
"""
from __future__ import annotations

import numpy as np

from .refine import dcm2quat, observations, quat2dcm

NO_CONSENSUS = 64
DEGENERATE = 1e-6          # model triangle: |cross| <= DEGENERATE * (longest edge)^2
A4_MIN = 1e-12             # quartic: |A4| <= A4_MIN * max |A_k| is skipped
POLISH_STEPS = 2           # Newton steps on the three distances after the quartic
_CHUNK = 128              # problems per vectorised pass (bounds the temporaries)


def default_min_inliers(n: int) -> int:
    """max(4, ceil(n / 2)): 6 for the 11-point Tango model."""
    return max(4, (int(n) + 1) // 2)


def triples(n: int) -> np.ndarray:
    """All i < j < k of range(n) in lexicographic order [C(n, 3) x 3]; the row number is the triple's index."""
    return np.array([(i, j, k) for i in range(n) for j in range(i + 1, n) for k in range(j + 1, n)], np.int64)


def _newton(coef, x, steps=2):
    """``steps`` Newton steps on the polynomial with coefficients ``coef`` (highest first); a step whose derivative is
    zero (or whose result is not finite) is not taken."""
    for _ in range(steps):
        f = coef[0]
        df = np.zeros_like(x)
        for a in coef[1:]:
            df = df * x + f
            f = f * x + a
        with np.errstate(all='ignore'):
            x2 = x - f / df
        x = np.where((df != 0) & np.isfinite(x2), x2, x)
    return x


def quartic_roots(A4, A3, A2, A1, A0) -> np.ndarray:
    """Real roots of A4 x^4 + ... + A0 [... x 4], ascending, +inf where there is none (or the quartic is skipped)."""
    with np.errstate(all='ignore'):
        big = np.maximum(np.maximum(np.abs(A3), np.abs(A2)), np.maximum(np.abs(A1), np.abs(A0)))
        ok = np.abs(A4) > A4_MIN * np.maximum(np.abs(A4), big)
        i4 = 1.0 / np.where(ok, A4, 1.0)
        b, c, d, e = A3 * i4, A2 * i4, A1 * i4, A0 * i4
        b2 = b * b
        p = c - 0.375 * b2
        q = d - 0.5 * b * c + 0.125 * b2 * b
        r = e - 0.25 * b * d + 0.0625 * b2 * c - (3.0 / 256.0) * b2 * b2
        # resolvent cubic m^3 + c2 m^2 + c1 m + c0, largest real root (c0 <= 0: it is >= 0)
        c2, c1, c0 = p, 0.25 * p * p - r, -0.125 * q * q
        P = c1 - c2 * c2 / 3.0
        Q = 2.0 * c2 * c2 * c2 / 27.0 - c2 * c1 / 3.0 + c0
        D = 0.25 * Q * Q + P * P * P / 27.0
        one = D > 0
        sD = np.sqrt(np.where(one, D, 0.0))
        A = np.cbrt(0.5 * np.abs(Q) + sD)
        A = np.where(Q > 0, -A, A)
        t1 = A - P / (3.0 * np.where(one, A, 1.0))
        k = np.sqrt(np.maximum(-P / 3.0, 0.0))
        k3 = k * k * k
        cs = np.clip(-Q / (2.0 * np.where(k3 > 0, k3, 1.0)), -1.0, 1.0)
        t3 = np.where(k3 > 0, 2.0 * k * np.cos(np.arccos(cs) / 3.0), 0.0)
        m = np.where(one, t1, t3) - c2 / 3.0
        m = _newton((np.ones_like(m), c2, c1, c0), m)
        ok &= np.isfinite(m) & (m > 0)
        w = np.sqrt(np.where(ok, 2.0 * m, 1.0))
        qw = 2.0 * q / w
        base = -2.0 * p - 2.0 * m
        d1, d2 = base - qw, base + qw
        s1, s2 = np.sqrt(np.maximum(d1, 0.0)), np.sqrt(np.maximum(d2, 0.0))
        sh = 0.25 * b
        y = np.stack([0.5 * (w - s1) - sh, 0.5 * (w + s1) - sh, 0.5 * (-w - s2) - sh, 0.5 * (-w + s2) - sh], -1)
        have = np.stack([d1 >= 0, d1 >= 0, d2 >= 0, d2 >= 0], -1) & ok[..., None]
        y = _newton((A4[..., None], A3[..., None], A2[..., None], A1[..., None], A0[..., None]), np.where(have, y, 0.0))
        y = np.where(have & np.isfinite(y), y, np.inf)
    r0, r1, r2, r3 = y[..., 0], y[..., 1], y[..., 2], y[..., 3]
    r0, r1 = np.minimum(r0, r1), np.maximum(r0, r1)        # the kernel's sorting network
    r2, r3 = np.minimum(r2, r3), np.maximum(r2, r3)
    r0, r2 = np.minimum(r0, r2), np.maximum(r0, r2)
    r1, r3 = np.minimum(r1, r3), np.maximum(r1, r3)
    r1, r2 = np.minimum(r1, r2), np.maximum(r1, r2)
    return np.stack([r0, r1, r2, r3], -1)


def _polish(s1, s2, s3, ca, cb, cg, a2, b2, c2, steps=POLISH_STEPS):
    """``steps`` Newton steps on the three law-of-cosines equations the distances solve (s2^2 + s3^2 - 2 s2 s3 cos alpha
    = a^2 and its two siblings), 3 x 3 by Cramer's rule: u comes from v through a quotient that can be small, and
    this brings the camera triangle back to the model's to rounding. A step with a singular Jacobian (or a result that
    is not finite) is not taken."""
    for _ in range(steps):
        with np.errstate(all='ignore'):
            f1 = s2 * s2 + s3 * s3 - 2 * s2 * s3 * ca - a2
            f2 = s1 * s1 + s3 * s3 - 2 * s1 * s3 * cb - b2
            f3 = s1 * s1 + s2 * s2 - 2 * s1 * s2 * cg - c2
            j12, j13 = 2 * (s2 - s3 * ca), 2 * (s3 - s2 * ca)
            j21, j23 = 2 * (s1 - s3 * cb), 2 * (s3 - s1 * cb)
            j31, j32 = 2 * (s1 - s2 * cg), 2 * (s2 - s1 * cg)
            det = j12 * j23 * j31 + j13 * j21 * j32          # the diagonal of the Jacobian is zero
            d1 = (-f1 * j23 * j32 + j12 * j23 * f3 + j13 * f2 * j32) / det
            d2 = (j13 * j21 * f3 + f1 * j23 * j31 - j13 * f2 * j31) / det
            d3 = (j12 * f2 * j31 + f1 * j21 * j32 - j12 * j21 * f3) / det
            good = (det != 0) & np.isfinite(d1) & np.isfinite(d2) & np.isfinite(d3)
        s1, s2, s3 = np.where(good, s1 - d1, s1), np.where(good, s2 - d2, s2), np.where(good, s3 - d3, s3)
    return s1, s2, s3


def _unit(v):
    with np.errstate(all='ignore'):
        return v / np.sqrt(np.sum(v * v, axis=-1, keepdims=True))


def _reproject(R, t, X, uv, K):
    """-> squared reprojection error [... x n] (px^2) and all-points-in-front [...] of the poses R [... x 3 x 3],
    t [... x 3] against the observations uv [B x n x 2] (broadcast over the axes between)."""
    fu, fv, uc, vc = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    Xc = np.einsum('...ij,nj->...ni', R, X) + t[..., None, :]
    extra = (1,) * (R.ndim - 3)
    uo = uv.reshape(uv.shape[:1] + extra + uv.shape[1:])
    with np.errstate(all='ignore'):
        iz = 1.0 / Xc[..., 2]
        ru = fu * (Xc[..., 0] * iz) + uc - uo[..., 0]
        rv = fv * (Xc[..., 1] * iz) + vc - uo[..., 1]
        return ru * ru + rv * rv, np.all(Xc[..., 2] > 0, axis=-1)


def hypotheses(uv, X, K, cand, tau):
    """Every hypothesis of every triple: uv [B x n x 2] observations (px), X [n x 3] model, cand [B x n] bool.
    -> (cost [B x T x 4], +inf where there is no valid hypothesis; R [B x T x 4 x 3 x 3]; t [B x T x 4 x 3];
    scored [B x T x 4] bool: a pose was formed and reprojected)."""
    n = X.shape[0]
    fu, fv, uc, vc = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    tr = triples(n)
    ti, tj, tk = tr[:, 0], tr[:, 1], tr[:, 2]
    Xi, Xj, Xk = X[ti], X[tj], X[tk]
    a2 = np.sum((Xj - Xk) ** 2, -1)
    b2 = np.sum((Xi - Xk) ** 2, -1)
    c2 = np.sum((Xi - Xj) ** 2, -1)
    nm = np.cross(Xj - Xi, Xk - Xi)
    nm2 = np.sum(nm * nm, -1)
    longest = np.maximum(a2, np.maximum(b2, c2))
    model_ok = nm2 > (DEGENERATE * longest) ** 2
    with np.errstate(all='ignore'):
        m1 = (Xj - Xi) / np.sqrt(c2)[:, None]
        m3 = nm / np.sqrt(nm2)[:, None]
        m2 = np.cross(m3, m1)
        ib2 = 1.0 / b2
        qq, pp = (a2 - c2) * ib2, (a2 + c2) * ib2
        ab, cb = a2 * ib2, c2 * ib2
        bmc, bma = (b2 - c2) * ib2, (b2 - a2) * ib2
        bl = np.sqrt(b2)

        f = _unit(np.stack([(uv[..., 0] - uc) / fu, (uv[..., 1] - vc) / fv, np.ones(uv.shape[:2])], -1))   # [B x n x 3]
        fi, fj, fk = f[:, ti], f[:, tj], f[:, tk]
        ca, cbeta, cg = np.sum(fj * fk, -1), np.sum(fi * fk, -1), np.sum(fi * fj, -1)
        ca2, cg2 = ca * ca, cg * cg
        A4 = (qq - 1) ** 2 - 4 * cb * ca2
        A3 = 4 * (qq * (1 - qq) * cbeta - (1 - pp) * ca * cg + 2 * cb * ca2 * cbeta)
        A2 = 2 * (qq * qq - 1 + 2 * qq * qq * cbeta * cbeta + 2 * bmc * ca2 - 4 * pp * ca * cbeta * cg + 2 * bma * cg2)
        A1 = 4 * (-qq * (1 + qq) * cbeta + 2 * ab * cg2 * cbeta - (1 - pp) * ca * cg)
        A0 = (1 + qq) ** 2 - 4 * ab * cg2
        use = model_ok[None, :] & cand[:, ti] & cand[:, tj] & cand[:, tk]
        v = quartic_roots(A4, A3, A2, A1, A0)                    # [B x T x 4]
        v = np.where(use[..., None], v, np.inf)
        e = lambda z: z[..., None]                              # noqa: E731  [B x T] -> [B x T x 1]
        live = np.isfinite(v) & (v > 0)
        vv = np.where(live, v, 1.0)
        den = 2 * (e(cg) - vv * e(ca))
        u = ((e(qq) - 1) * vv * vv - 2 * e(qq) * e(cbeta) * vv + 1 + e(qq)) / den
        live &= (den != 0) & np.isfinite(u) & (u > 0)
        s1 = bl[None, :, None] / np.sqrt(1 + vv * vv - 2 * vv * e(cbeta))
        s2, s3 = u * s1, vv * s1
        s1, s2, s3 = _polish(s1, s2, s3, e(ca), e(cbeta), e(cg), a2[None, :, None], b2[None, :, None], c2[None, :, None])
        live &= (s1 > 0) & (s2 > 0) & (s3 > 0)
        Yi =s1[..., None] * fi[:, :, None, :]
        Yj = s2[..., None] * fj[:, :, None, :]
        Yk = s3[..., None] * fk[:, :, None, :]
        d1 = Yj - Yi
        nc = np.cross(d1, Yk - Yi)
        l1, l3 = np.sum(d1 * d1, -1), np.sum(nc * nc, -1)
        live &= (l1 > 0) & (l3 > 0) & np.isfinite(l1) & np.isfinite(l3)
        e1 = d1 / np.sqrt(np.where(live, l1, 1.0))[..., None]
        e3 = nc / np.sqrt(np.where(live, l3, 1.0))[..., None]
        e2 = np.cross(e3, e1)
        R = e1[..., :, None] * m1[None, :, None, None, :] + e2[..., :, None] * m2[None, :, None, None, :] + \
            e3[..., :, None] * m3[None, :, None, None, :]
        t = Yi - np.einsum('btrij,tj->btri', R, Xi)
        R = np.where(live[..., None, None], R, np.eye(3))
        t = np.where(live[..., None], t, 0.0)
        e2px, front = _reproject(R, t, X, uv, K)                 # [B x T x 4 x n]
        cost = np.sum(np.where(cand[:, None, None, :], np.minimum(e2px, tau * tau), 0.0), -1)
        cost = np.where(live & front & np.isfinite(cost), cost, np.inf)
    return cost, R, t, live


def _prepare(kp, kp3d, K, nu, nv, dist, weights):
    kp = np.ascontiguousarray(kp, np.float32)
    X = np.asarray(kp3d, np.float32).astype(np.float64).reshape(-1, 3)
    K = np.asarray(K, np.float64).reshape(3, 3)
    B, n = kp.shape[0], X.shape[0]
    assert kp.shape[1] == 2 * (n + 1) and 4 <= n <= 16
    conf = np.ones((B, n), np.float32) if weights is None else np.array(weights, np.float32).reshape(B, n)
    uv = observations(kp, K, nu, nv, dist)
    with np.errstate(all='ignore'):
        row_bad = ~np.all(np.isfinite(uv), axis=(1, 2)) | ~np.all(np.isfinite(conf) & (conf >= 0), axis=-1)
        cand = (conf > 0) & ~row_bad[:, None]
    return kp, X, K, conf, np.where(row_bad[:, None, None], 0.0, uv), row_bad, cand


def triple_cost(kp, kp3d, K, nu, nv, triple, dist=None, weights=None, inlier_px=8.0) -> np.ndarray:
    """The lowest cost over the roots of triple ``triple[b]`` (its index among all C(n, 3)) of every problem [B],
    +inf where the triple has no valid hypothesis."""
    kp, X, K, conf, uv, row_bad, cand = _prepare(kp, kp3d, K, nu, nv, dist, weights)
    tau = float(np.float32(inlier_px))
    idx = np.broadcast_to(np.asarray(triple, np.int64), (kp.shape[0],))
    out = np.full(kp.shape[0], np.inf)
    for a in range(0, kp.shape[0], _CHUNK):
        s = slice(a, a + _CHUNK)
        cost = hypotheses(uv[s], X, K, cand[s], tau)[0]
        out[s] = cost[np.arange(cost.shape[0]), idx[s]].min(axis=-1)
    return out


def pose_cost(quat, pos, kp, kp3d, K, nu, nv, dist=None, weights=None, inlier_px=8.0):
    """The score of given poses (``quat`` [B x 4], ``pos`` [B x 3]): -> (cost [B] fp64, +inf where a model point is not
    in front of the camera; squared reprojection errors [B x n] in px^2)."""
    kp, X, K, conf, uv, row_bad, cand = _prepare(kp, kp3d, K, nu, nv, dist, weights)
    tau = float(np.float32(inlier_px))
    q = np.asarray(quat, np.float64).reshape(-1, 4)
    R = quat2dcm(q / np.sqrt(np.sum(q * q, axis=-1, keepdims=True)))
    e2, front = _reproject(R, np.asarray(pos, np.float64).reshape(-1, 3), X, uv, K)
    cost = np.sum(np.where(cand, np.minimum(e2, tau * tau), 0.0), -1)
    return np.where(front, cost, np.inf), e2


def consensus_host(kp, kp3d, K, nu, nv, dist=None, weights=None, inlier_px=8.0, min_inliers=None, quat=None, pos=None,
                   status=None) -> dict:
    """Exhaustive 3-point consensus on the normalised keypoints ``kp`` [B x 2(n+1)] (origin first, after the sigmoid).
    ``weights``: confidences [B x n] >= 0 or None (all 1); ``inlier_px``: the truncation tau in pixels;
    ``min_inliers``: 4..n, None = ``default_min_inliers(n)``; ``quat`` / ``pos``: the start pose (EPnP's), kept bit for
    bit on a row without consensus and the hemisphere of the returned quaternion otherwise (None: identity, origin);
    ``status``: the status words to OR into, or None.

    -> {'ori' [B x 4] f32, 'pos' [B x 3] f32, 'inliers' [B x n] bool, 'weights' [B x n] f32 (c_i or 1 for inliers, 0
    otherwise), 'n_inliers' [B] i32, 'triple' [B] i32, 'root' [B] i32, 'scored' [B] i32 (hypotheses reprojected),
    'cost' [B] f64 (the kernel's is its float32), 'status' [B] i32, 'R' [B x 3 x 3] / 't' [B x 3] f64 (the winning
    hypothesis before the float32 rounding; the start pose's where there is none)}."""
    kp, X, K, conf, uv, row_bad, cand = _prepare(kp, kp3d, K, nu, nv, dist, weights)
    B, n = conf.shape
    tau = float(np.float32(inlier_px))
    assert np.isfinite(tau) and tau > 0
    mi = default_min_inliers(n) if min_inliers is None else int(min_inliers)
    assert 4 <= mi <= n, 'min_inliers must be in 4..n'
    q_in = np.tile(np.float32([1, 0, 0, 0]), (B, 1)) if quat is None else \
        np.ascontiguousarray(quat, np.float32).reshape(B, 4)
    t_in = np.zeros((B, 3), np.float32) if pos is None else np.ascontiguousarray(pos, np.float32).reshape(B, 3)
    st = np.zeros(B, np.int32) if status is None else np.array(status, np.int32).reshape(B)

    best = np.full(B, np.inf)
    flat = np.zeros(B, np.int64)
    scored = np.zeros(B, np.int32)
    Rb, tb = np.tile(np.eye(3), (B, 1, 1)), np.zeros((B, 3))
    for a in range(0, B, _CHUNK):
        s = slice(a, a + _CHUNK)
        cost, R, t, live = hypotheses(uv[s], X, K, cand[s], tau)
        c = cost.reshape(cost.shape[0], -1)
        f = np.argmin(c, axis=-1)                      # the first minimum: lowest triple, then lowest root
        r = np.arange(c.shape[0])
        best[s], flat[s] = c[r, f], f
        scored[s] = live.reshape(c.shape[0], -1).sum(-1)
        Rb[s], tb[s] = R.reshape(c.shape[0], -1, 3, 3)[r, f], t.reshape(c.shape[0], -1, 3)[r, f]
    found = np.isfinite(best) & (cand.sum(-1) >= 3)
    e2, _ = _reproject(Rb, tb, X, uv, K)
    inl = cand & (e2 < tau * tau) & found[:, None]
    n_inl = inl.sum(-1).astype(np.int32)
    okay = found & (n_inl >= mi)

    with np.errstate(all='ignore'):
        qo = dcm2quat(Rb)
        qs = q_in.astype(np.float64)
        start_ok = np.all(np.isfinite(qs), axis=-1) & (np.sum(qs * qs, axis=-1) > 0)
        qo *= np.where(start_ok[:, None] & (np.sum(qo * qs, axis=-1, keepdims=True) < 0), -1.0, 1.0)
    st[~okay] |= NO_CONSENSUS
    qs64 = qs / np.sqrt(np.maximum(np.sum(qs * qs, axis=-1, keepdims=True), 1e-300))
    return {'ori': np.where(okay[:, None], qo.astype(np.float32), q_in),
            'pos': np.where(okay[:, None], tb.astype(np.float32), t_in),
            'inliers': inl & okay[:, None],
            'weights': np.where(okay[:, None], np.where(inl, conf, np.float32(0)), conf).astype(np.float32),
            'n_inliers': np.where(okay, n_inl, 0).astype(np.int32),
            'triple': np.where(okay, flat // 4, -1).astype(np.int32),
            'root': np.where(okay, flat % 4, -1).astype(np.int32),
            'scored': scored,
            'cost': np.where(okay, best, np.nan),
            'status': st,
            'R': np.where(okay[:, None, None], Rb, quat2dcm(np.where(start_ok[:, None], qs64, [1.0, 0, 0, 0]))),
            't': np.where(okay[:, None], tb, t_in.astype(np.float64))}
