"""Pose tracking for video: an error-state Kalman filter over the per-frame pose of any head -- the NumPy twin and the
specification of csrc/k_track.hip (``spef_track_step``; ``Engine.tracker``).

State per stream: a unit quaternion q (scalar first), a position t, an angular rate w in rad per frame and a velocity
v in m per frame, with the 12 x 12 covariance P of the error state (theta, t, w, v). The rate is a left perturbation
in the camera frame, R_{k+1} = exp([w]x) R_k -- the convention of the pose refinement (``spe.refine``), whose 6 x 6
covariance is therefore a measurement covariance as it stands. One step is one frame; there is no dt.

The model is constant velocity with F = [[I6, I6], [0, I6]]: the orientation error is carried over a frame as if
exp([w]x) were the identity, which holds for small inter-frame rotations (|w| << 1 rad per frame).

One frame of one stream, measurement (q_m, t_m[, cov][, status]), all arithmetic in float64:
 1. the measurement is invalid when ``status & 15`` is nonzero (bits 16 and 32 are informational), q_m or t_m is not
    finite, or |q_m| = 0;
 2. without a track an invalid row passes through unchanged (d2 = NaN, track status 1 | 8) and a valid one starts the
    track: q = q_m / |q_m|, t = t_m, w = v = 0, P = diag(p0), output that pose, d2 = 0, status 0;
 3. predict: q- = normalise(exp(w) (x) q), t- = t + v, P- = F P F^T + Q; with P = [[A, B], [B^T, C]] in 6 x 6 blocks
    that is [[((A + (B + B^T)) + C) + Qa, B + C], [., C + Qc]], summed in this order (symmetric bit for bit);
 4. innovation y = [Log(q_m (x) conj(q-)), t_m - t-] (the difference flipped to w >= 0; series below |v| = 1e-8),
    R = cov_scale (cov + cov^T) / 2 when all 36 entries are finite, else diag(r); S = P-[0:6, 0:6] + R = L L^T; a pivot
    that is not positive and finite makes the measurement invalid; z = L^-1 y, d2 = z^T z = y^T S^-1 y;
 5. an invalid (bit 1) or gated (gate_chi2 > 0 and d2 > gate_chi2: bit 2) measurement coasts: the count of consecutive
    coasted frames goes up, state and output are the prediction, w and v are kept. A gated row whose count now
    exceeds max_coast starts the track again from this measurement instead (bits 2 | 4, count 0);
 6. update, through the Cholesky factor: W = P-[:, 0:6] L^-T (so K = W L^-1 and K S K^T = W W^T), delta = W z = K y;
    q = normalise(exp(delta_theta) (x) q-), t = t- + delta_t, w += delta_w, v += delta_v, P = P- - W W^T (every entry
    the same fixed-order sum, so P stays symmetric bit for bit; with H = [I6 0] this is (I - K H) P-); count = 0;
 7. the state quaternion is kept in the hemisphere of the stream's previous one (dot product not negative; the first
    frame of a track that had no state keeps the measurement's sign), and is the output; so are t, d2 and, when asked
    for, P[0:6, 0:6] and (w, v).

``track_status`` is a word of its own (not the decode status): 1 = measurement invalid, coasted; 2 = gated; 4 = track
started again from this row; 8 = no track, row passed through.

Rows are time-major (row ``t * S + s`` = step t of stream s) as on the video and scoring paths, and a stream's result
depends neither on S nor on how a sequence is cut into calls.

``step_modes`` (``spef_track_step_modes``) is the same filter fed up to K orientation candidates per row, the modes of
``spe.modes``: the candidate the prediction makes most likely becomes (q_m, cov) of step 4 -- its docstring states the
rule -- and steps 2 to 7 run unchanged on it. This is what resolves a two-peaked orientation PDF.
"""
from __future__ import annotations

import numpy as np

STATE_DOUBLES = 160      # have, coast, 0, q[4], t[3], w[3], v[3], P[144] row-major (SPEF_TRACK_STATE_DOUBLES)
INVALID, GATED, REINIT, NO_TRACK = 1, 2, 4, 8
# the reference's constants (kalman.py KalmanFilterPosSimple: q = p = I, r = 100 I), not tuned
DEFAULTS = dict(q=(1.0, 1.0, 1.0, 1.0), p0=(1.0, 1.0, 1.0, 1.0), r=(100.0, 100.0), cov_scale=1.0, gate_chi2=0.0,
                max_coast=0)


def check_params(q=DEFAULTS['q'], p0=DEFAULTS['p0'], r=DEFAULTS['r'], cov_scale=1.0, gate_chi2=0.0, max_coast=0):
    """-> the parameters as (q[4], p0[4], r[2], cov_scale, gate_chi2, max_coast); a scalar q / p0 / r is repeated.
    Raises AssertionError on a negative or non-finite value (what spef_track_create refuses)."""
    def vec(a, n):
        a = np.asarray(a, np.float64).reshape(-1)
        a = np.repeat(a, n) if a.size == 1 else a
        assert a.size == n and np.all(np.isfinite(a)) and np.all(a >= 0), 'tracker variances must be finite and >= 0'
        return a
    cov_scale, gate_chi2, max_coast = float(cov_scale), float(gate_chi2), int(max_coast)
    assert np.isfinite(cov_scale) and cov_scale >= 0 and np.isfinite(gate_chi2) and gate_chi2 >= 0 and max_coast >= 0
    return vec(q, 4), vec(p0, 4), vec(r, 2), cov_scale, gate_chi2, max_coast


def qmul(a, b):
    """Hamilton product, scalar first: R(a (x) b) = R(a) R(b)."""
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                     a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def qexp(w):
    """The quaternion of the rotation vector w (series below |w|^2 = 1e-16)."""
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if th2 < 1e-16:
        c, s = 1.0 - th2 / 8.0, 0.5 - th2 / 48.0
    else:
        th = np.sqrt(th2)
        c, s = np.cos(0.5 * th), np.sin(0.5 * th) / th
    return np.array([c, s * w[0], s * w[1], s * w[2]])


def qlog(d):
    """The rotation vector of the unit quaternion d, |angle| <= pi (d and -d give the same)."""
    if d[0] < 0:
        d = -d
    n2 = d[1] * d[1] + d[2] * d[2] + d[3] * d[3]
    n = np.sqrt(n2)
    f = 2.0 / d[0] * (1.0 - n2 / (3.0 * d[0] * d[0])) if n < 1e-8 else 2.0 * np.arctan2(n, d[0]) / n
    return np.array([f * d[1], f * d[2], f * d[3]])


def _unit(q):
    return q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])


def _chol6(S):
    """-> (L, ok): lower Cholesky factor of the 6 x 6 S, column by column; ok is False on a pivot that is not positive
    and finite."""
    L = np.zeros((6, 6))
    for j in range(6):
        d = S[j, j]
        for k in range(j):
            d -= L[j, k] * L[j, k]
        if not (d > 0.0 and d < np.inf):
            return L, False
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            v = S[i, j]
            for k in range(j):
                v -= L[i, k] * L[j, k]
            L[i, j] = v / L[j, j]
    return L, True


class PoseTrackerHost:
    """The filter of the module docstring for ``n_streams`` streams; mirrors ``engine.PoseTracker``."""

    def __init__(self, n_streams: int = 1, **params):
        assert 1 <= int(n_streams) <= 65536
        self.n_streams = int(n_streams)
        self.q, self.p0, self.r, self.cov_scale, self.gate_chi2, self.max_coast = check_params(**params)
        self._state = np.zeros((self.n_streams, STATE_DOUBLES))

    def reset(self, stream=None) -> None:
        if stream is None:
            self._state[:] = 0.0
        else:
            assert 0 <= int(stream) < self.n_streams
            self._state[int(stream)] = 0.0

    def state(self, first: int = 0, n=None) -> np.ndarray:
        n = self.n_streams - first if n is None else n
        assert first >= 0 and n >= 1 and first + n <= self.n_streams
        return self._state[first:first + n].copy()

    def set_state(self, state, first: int = 0) -> None:
        state = np.asarray(state, np.float64).reshape(-1, STATE_DOUBLES)
        assert first >= 0 and first + state.shape[0] <= self.n_streams
        self._state[first:first + state.shape[0]] = state

    def _start(self, st, qm, tm):
        st[:] = 0.0
        st[0] = 1.0
        st[3:7] = _unit(qm)
        st[7:10] = tm
        st[16:] = np.diag(np.repeat(self.p0, 3)).reshape(-1)

    def _predict(self, st):
        """Step 3 -> (P-, q-, t-)."""
        q, t, w, v = st[3:7].copy(), st[7:10].copy(), st[10:13].copy(), st[13:16].copy()
        P = st[16:].reshape(12, 12)
        A, B, C = P[:6, :6], P[:6, 6:], P[6:, 6:]
        Qd = np.diag(np.repeat(self.q, 3))
        Pm = np.empty((12, 12))
        Pm[:6, :6] = ((A + (B + B.T)) + C) + Qd[:6, :6]
        Pm[:6, 6:] = B + C
        Pm[6:, :6] = Pm[:6, 6:].T
        Pm[6:, 6:] = C + Qd[6:, 6:]
        return Pm, _unit(qmul(qexp(w), q)), t + v

    def _innovation(self, Pm, qp, tp, qm, tm, cov):
        """Step 4 -> (L, ok, z, d2): z is None and d2 NaN when a pivot of S fails."""
        qn = _unit(qm)
        y = np.concatenate([qlog(qmul(qn, qp * [1.0, -1.0, -1.0, -1.0])), tm - tp])
        R = np.diag(np.repeat(self.r, 3))
        if cov is not None and np.all(np.isfinite(cov)):
            cov = np.asarray(cov, np.float64).reshape(6, 6)
            R = self.cov_scale * ((cov + cov.T) * 0.5)
        L, ok = _chol6(Pm[:6, :6] + R)
        z, d2 = None, np.nan
        if ok:
            z = np.zeros(6)
            for i in range(6):
                s = y[i]
                for k in range(i):
                    s -= L[i, k] * z[k]
                z[i] = s / L[i, i]
            d2 = 0.0
            for k in range(6):
                d2 += z[k] * z[k]
        return L, ok, z, d2

    def _frame_modes(self, st, cands, tm, cov, status):
        """One frame of one stream with orientation candidates ``cands`` = [(q_k, mass_k, theta block_k)] and the
        shared (t_m, cov, status) -> (quat, pos, d2, track status, chosen, cost gap). The choice is made here; steps
        2 to 7 are ``_frame``'s, on the chosen (q_k, C_k)."""
        base = (int(status) & 15) == 0 and bool(np.all(np.isfinite(tm)))
        Cs, ok_k = [], []
        for qk, mk, blk in cands:
            C = np.array(cov, np.float64).reshape(6, 6)
            C[:3, :3] = np.asarray(blk, np.float64).reshape(3, 3)
            Cs.append(C)
            n2 = float(qk @ qk)
            ok_k.append(base and bool(np.all(np.isfinite(qk))) and 0.0 < n2 < np.inf and bool(np.isfinite(mk)) and
                        mk > 0.0)
        pick, gap = -1, np.inf
        if st[0] == 0.0:
            pick = next((k for k, g in enumerate(ok_k) if g), -1)
        else:
            Pm, qp, tp = self._predict(st)
            costs = {}
            for k, (qk, mk, _) in enumerate(cands):
                if not ok_k[k]:
                    continue
                L, ok, _, d2 = self._innovation(Pm, qp, tp, qk, tm, Cs[k])
                if ok:
                    lnl = 0.0
                    for j in range(6):
                        lnl += np.log(L[j, j])
                    costs[k] = (d2 + 2.0 * lnl) - 2.0 * np.log(mk)
            for k, c in costs.items():                      # the smallest cost, ties to the lowest k
                if pick < 0 or c < costs[pick]:
                    pick = k
            if len(costs) > 1:
                rest = sorted(c for k, c in costs.items() if k != pick)
                gap = rest[0] - costs[pick]
        if pick < 0:
            q0 = cands[0][0] if cands else np.full(4, np.nan)
            qo, to, d2, ts = self._frame(st, np.full(4, np.nan), tm, None, status)
            return (q0 if ts & NO_TRACK else qo), to, d2, ts, -1, gap
        return self._frame(st, cands[pick][0], tm, Cs[pick], status) + (pick, gap)

    def _frame(self, st, qm, tm, cov, status):
        """One frame of one stream on the state row ``st`` (in place) -> (quat, pos, d2, track status)."""
        valid = (int(status) & 15) == 0 and bool(np.all(np.isfinite(qm))) and bool(np.all(np.isfinite(tm)))
        valid = valid and float(qm @ qm) > 0.0 and float(qm @ qm) < np.inf
        if st[0] == 0.0:
            if not valid:
                return qm, tm, np.nan, INVALID | NO_TRACK
            self._start(st, qm, tm)
            return st[3:7].copy(), st[7:10].copy(), 0.0, 0
        q, t, w, v = st[3:7].copy(), st[7:10].copy(), st[10:13].copy(), st[13:16].copy()
        Pm, qp, tp = self._predict(st)
        d2, ok = np.nan, False
        if valid:
            L, ok, z, d2 = self._innovation(Pm, qp, tp, qm, tm, cov)
        ts = 0
        if not ok:
            ts = INVALID
        elif self.gate_chi2 > 0.0 and d2 > self.gate_chi2:
            ts = GATED
        if ts:
            coast = st[1] + 1.0
            if ts == GATED and coast > self.max_coast:
                prev = q
                self._start(st, qm, tm)
                if st[3:7] @ prev < 0.0:
                    st[3:7] = -st[3:7]
                return st[3:7].copy(), st[7:10].copy(), d2, GATED | REINIT
            if qp @ q < 0.0:
                qp = -qp
            st[1] = coast
            st[3:7], st[7:10] = qp, tp
            st[16:] = Pm.reshape(-1)
            return qp, tp, d2, ts
        W = np.zeros((12, 6))
        for i in range(12):
            for k in range(6):
                s = Pm[i, k]
                for m in range(k):
                    s -= W[i, m] * L[k, m]
                W[i, k] = s / L[k, k]
        delta = np.zeros(12)
        for i in range(12):
            for k in range(6):
                delta[i] += W[i, k] * z[k]
        qu = _unit(qmul(qexp(delta[0:3]), qp))
        if qu @ q < 0.0:
            qu = -qu
        Pn = Pm.copy()
        for k in range(6):
            Pn -= np.outer(W[:, k], W[:, k])
        st[1] = 0.0
        st[3:7], st[7:10] = qu, tp + delta[3:6]
        st[10:13], st[13:16] = w + delta[6:9], v + delta[9:12]
        st[16:] = Pn.reshape(-1)
        return st[3:7].copy(), st[7:10].copy(), d2, 0

    def step(self, quat, pos, cov=None, status=None, T=None) -> dict:
        """``quat`` [T * S x 4], ``pos`` [T * S x 3], ``cov`` None or [T * S x 6 x 6], ``status`` None or [T * S],
        time-major -> {'ori', 'pos', 'mahalanobis', 'track_status', 'cov' [T * S x 6 x 6], 'rates' [T * S x 6]}
        (float64; the rates are (w, v); a passed-through row has NaN in 'cov' and 'rates')."""
        quat = np.asarray(quat, np.float64).reshape(-1, 4)
        pos = np.asarray(pos, np.float64).reshape(-1, 3)
        B, S = quat.shape[0], self.n_streams
        T = B // S if T is None else int(T)
        assert T >= 1 and B == T * S and pos.shape[0] == B, f'{B} rows are not T = {T} steps of {S} streams'
        cov = None if cov is None else np.asarray(cov, np.float64).reshape(B, 6, 6)
        status = np.zeros(B, np.int64) if status is None else np.asarray(status).reshape(B)
        out = {'ori': np.empty((B, 4)), 'pos': np.empty((B, 3)), 'mahalanobis': np.empty(B),
               'track_status': np.zeros(B, np.int32), 'cov': np.empty((B, 6, 6)), 'rates': np.empty((B, 6))}
        for s in range(S):
            st = self._state[s]
            for t in range(T):
                r = t * S + s
                qo, to, d2, ts = self._frame(st, quat[r], pos[r], None if cov is None else cov[r], status[r])
                out['ori'][r], out['pos'][r], out['mahalanobis'][r], out['track_status'][r] = qo, to, d2, ts
                if ts & NO_TRACK:
                    out['cov'][r], out['rates'][r] = np.nan, np.nan
                else:
                    out['cov'][r] = st[16:].reshape(12, 12)[:6, :6]
                    out['rates'][r] = st[10:16]
        return out

    def step_modes(self, mode_quat, mode_mass, mode_cov, n_modes, pos, cov, status=None, T=None) -> dict:
        """``step`` with up to K orientation candidates per row (``spe.modes.decode_modes_host``'s outputs):
        ``mode_quat`` [T * S x K x 4], ``mode_mass`` [T * S x K], ``mode_cov`` [T * S x K x 3 x 3], ``n_modes``
        [T * S]; ``pos`` [T * S x 3] and ``cov`` [T * S x 6 x 6] (required: it supplies the t block) are shared by a
        row's candidates. Candidate k < n_modes is valid when its quaternion is finite and non-zero and its mass finite
        and > 0; its covariance C_k is ``cov`` with the theta block replaced by ``mode_cov[k]`` and then goes through
        step 4's rule. With a track the candidate of smallest cost_k = d2_k + 2 sum_j ln L_k[j][j] - 2 ln mass_k
        (twice the negative log-likelihood; a failed pivot makes it invalid; ties to the lowest k) is the measurement,
        without one the lowest valid k; with no valid candidate the measurement is invalid. Steps 2 to 7 then run
        unchanged. -> ``step``'s dict and 'chosen' [T * S] (-1: none) and 'cost_gap' [T * S] (second-best minus best
        cost; inf with fewer than two candidates weighed)."""
        mode_quat = np.asarray(mode_quat, np.float64)
        B, S = mode_quat.shape[0], self.n_streams
        K = mode_quat.shape[1]
        mode_mass = np.asarray(mode_mass, np.float64).reshape(B, K)
        mode_cov = np.asarray(mode_cov, np.float64).reshape(B, K, 3, 3)
        n_modes = np.asarray(n_modes).reshape(B)
        pos = np.asarray(pos, np.float64).reshape(B, 3)
        cov = np.asarray(cov, np.float64).reshape(B, 6, 6)
        T = B // S if T is None else int(T)
        assert T >= 1 and B == T * S and mode_quat.shape == (B, K, 4), f'{B} rows are not T = {T} steps of {S} streams'
        status = np.zeros(B, np.int64) if status is None else np.asarray(status).reshape(B)
        out = {'ori': np.empty((B, 4)), 'pos': np.empty((B, 3)), 'mahalanobis': np.empty(B),
               'track_status': np.zeros(B, np.int32), 'cov': np.empty((B, 6, 6)), 'rates': np.empty((B, 6)),
               'chosen': np.zeros(B, np.int32), 'cost_gap': np.empty(B)}
        for s in range(S):
            st = self._state[s]
            for t in range(T):
                r = t * S + s
                n = int(min(max(n_modes[r], 0), K))
                cands = [(mode_quat[r, k], mode_mass[r, k], mode_cov[r, k]) for k in range(n)]
                qo, to, d2, ts, pick, gap = self._frame_modes(st, cands, pos[r], cov[r], status[r])
                if ts & NO_TRACK:
                    qo = mode_quat[r, 0]
                out['ori'][r], out['pos'][r], out['mahalanobis'][r], out['track_status'][r] = qo, to, d2, ts
                out['chosen'][r], out['cost_gap'][r] = pick, gap
                if ts & NO_TRACK:
                    out['cov'][r], out['rates'][r] = np.nan, np.nan
                else:
                    out['cov'][r] = st[16:].reshape(12, 12)[:6, :6]
                    out['rates'][r] = st[10:16]
        return out
