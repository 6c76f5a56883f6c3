"""Fixed-interval smoothing of a recorded video: the Rauch-Tung-Striebel backward pass over the posteriors of the pose
tracker (``spe.track``) -- the NumPy twin and the specification of csrc/k_smooth.hip (``spef_track_smooth``;
``engine.PoseHistory``).

The tracker estimates frame k from frames 0..k. On a recorded sequence every later frame is known as well, and the
backward pass folds it in: it needs no measurement, only the filter's posterior state (q, t, w, v) and the 12 x 12 P
of every frame, which ``spef_track_step_hist`` / ``spef_track_history_push`` record (``record`` here). A history row is
the tracker's state row (``track.STATE_DOUBLES`` doubles) with that frame's ``track_status`` in slot 2.

This is the RTS recursion under the filter's own model: F = [[I6, I6], [0, I6]], which carries the orientation error
over a frame as if exp([w]x) were the identity (small inter-frame rotations, |w| << 1 rad per frame), and the error
state (theta, t, w, v) with theta a left perturbation. It is exact for the linear (t, v) part and first order in theta.

A window is the frames first .. first + T - 1 of one stream; k runs from the last frame down. ``smooth_status``:
 0 = smoothed; 1 = the row has no track (have = 0): its pose is left as it came, 'cov' and 'rates' are NaN;
 2 = a chain ends here (a segment end): x^s_k = x_k and P^s_k = P_k, the filter's. That is the window's last frame, a
     row whose successor has no track, a row whose successor carries ``track_status & 4`` (the track was started again:
     nothing is smoothed across a re-initialisation), and, with bit 4 as well (6), a row whose P-_{k+1} has a Cholesky
     pivot that is not positive and finite.

Otherwise, in float64 and in this order of sums:
 a. (P-, q-, t-) = step 3 of ``spe.track`` applied to x_k (``PoseTrackerHost._predict``: the filter's value);
 b. P- = L L^T column by column, d_j = P-[j][j] - sum_{k<j} L[j][k]^2 and L[i][j] = (P-[i][j] - sum_{k<j} L[i][k]
    L[j][k]) / L[j][j], k ascending;
 c. P F^T = [[A + B, B], [B^T + C, C]] for P = [[A, B], [B^T, C]]: entry [i][j] is P[i][j] + P[i][j + 6] for j < 6;
 d. U = (P F^T) L^-T by rows: U[i][k] = (PF^T[i][k] - sum_{m<k} U[i][m] L[k][m]) / L[k][k], k = 0..11, m ascending;
 e. G = U L^-1 by rows: G[i][k] = (U[i][k] - sum_{m>k} G[i][m] L[m][k]) / L[k][k], k = 11..0, m ascending
    (G = P F^T (P-)^-1, the smoother gain; it depends on row k alone);
 f. e = [Log(q^s_{k+1} (x) conj(q-)), t^s_{k+1} - t-, w^s_{k+1} - w_k, v^s_{k+1} - v_k] (the Log as in the filter's
    innovation: flipped to a scalar part >= 0, series below |v| = 1e-8);
 g. delta[i] = sum_k G[i][k] e[k], k ascending;
 h. q^s_k = normalise(exp(delta_theta) (x) q_k), kept in the hemisphere of q_k (the filter's output for the row);
    t^s_k = t_k + delta_t, w^s_k = w_k + delta_w, v^s_k = v_k + delta_v;
 i. P^s_k = P_k + G D G^T with D = P^s_{k+1} - P-: M[i][k] = sum_m G[i][m] D[m][k] (m ascending), then entry [i][j]
    is P_k[i][j] + sum_k M[a][k] G[b][k] with a = max(i, j), b = min(i, j), k ascending. An entry and its mirror are the
    same sum, so P^s is symmetric bit for bit (P, P- and hence D are).

Streams are independent and a stream's result does not depend on S.
"""
from __future__ import annotations

import numpy as np

from . import track as TK

SMOOTHED, NO_TRACK, SEGMENT_END, BAD_PIVOT = 0, 1, 2, 4


def record(tracker: TK.PoseTrackerHost, quat, pos, cov=None, status=None, T=None):
    """Step ``tracker`` frame by frame and keep its state after every frame -> (``tracker.step``'s outputs, history
    [T x S x 160]: the state rows with slot 2 = that frame's track status)."""
    quat = np.asarray(quat, np.float64).reshape(-1, 4)
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    S = tracker.n_streams
    B = quat.shape[0]
    T = B // S if T is None else int(T)
    assert T >= 1 and B == T * S
    cov = None if cov is None else np.asarray(cov, np.float64).reshape(B, 6, 6)
    status = None if status is None else np.asarray(status).reshape(B)
    outs, hist = [], np.empty((T, S, TK.STATE_DOUBLES))
    for t in range(T):
        r = slice(t * S, (t + 1) * S)
        o = tracker.step(quat[r], pos[r], None if cov is None else cov[r], None if status is None else status[r], T=1)
        outs.append(o)
        hist[t] = tracker.state()
        hist[t, :, 2] = o['track_status']
    return {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}, hist


def _chol12(A):
    """-> (L, ok): step b; ok is False on a pivot that is not positive and finite."""
    L = np.zeros((12, 12))
    for j in range(12):
        d = A[j, j]
        for k in range(j):
            d -= L[j, k] * L[j, k]
        if not (d > 0.0 and d < np.inf):
            return L, False
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 12):
            v = A[i, j]
            for k in range(j):
                v -= L[i, k] * L[j, k]
            L[i, j] = v / L[j, j]
    return L, True


class PoseSmootherHost:
    """The backward pass of the module docstring with the parameters of the tracker that recorded the history (only the
    process noise ``q`` enters); mirrors ``engine.PoseHistory.smooth``."""

    def __init__(self, **params):
        self._trk = TK.PoseTrackerHost(1, **params)

    def gain(self, row):
        """Steps a to e on one history row -> (G, P-, q-, t-, ok); G is None when a pivot fails."""
        Pm, qp, tp = self._trk._predict(row)
        L, ok = _chol12(Pm)
        if not ok:
            return None, Pm, qp, tp, False
        P = row[16:].reshape(12, 12)
        PF = P.copy()
        PF[:, :6] = P[:, :6] + P[:, 6:]
        U, G = np.zeros((12, 12)), np.zeros((12, 12))
        for i in range(12):
            for k in range(12):
                s = PF[i, k]
                for m in range(k):
                    s -= U[i, m] * L[k, m]
                U[i, k] = s / L[k, k]
            for k in range(11, -1, -1):
                s = U[i, k]
                for m in range(k + 1, 12):
                    s -= G[i, m] * L[m, k]
                G[i, k] = s / L[k, k]
        return G, Pm, qp, tp, True

    def smooth(self, hist, quat, pos, first: int = 0, T=None) -> dict:
        """``hist`` [N x S x 160] (``record``), ``quat`` [T * S x 4] / ``pos`` [T * S x 3] the filter's outputs for the
        rows of the window (time-major) -> {'ori', 'pos', 'cov' [T * S x 6 x 6] (the pose block of P^s), 'rates'
        [T * S x 6] (w^s, v^s), 'smooth_status' [T * S]} in float64; rows without a track keep ``quat`` / ``pos``."""
        hist = np.asarray(hist, np.float64)
        N, S = hist.shape[:2]
        T = N - first if T is None else int(T)
        assert first >= 0 and T >= 1 and first + T <= N
        out = {'ori': np.array(quat, np.float64).reshape(T * S, 4), 'pos': np.array(pos, np.float64).reshape(T * S, 3),
               'cov': np.full((T * S, 6, 6), np.nan), 'rates': np.full((T * S, 6), np.nan),
               'smooth_status': np.zeros(T * S, np.int32)}
        for s in range(S):
            xs = Ps = None          # the smoothed state of frame k + 1: (q, t, w, v), P; None: a chain starts
            for f in range(T - 1, -1, -1):
                x, r = hist[first + f, s], f * S + s
                if x[0] == 0.0:
                    out['smooth_status'][r] = NO_TRACK
                    xs = Ps = None
                    continue
                nxt = hist[first + f + 1, s] if f + 1 < T else None
                st = SMOOTHED
                if nxt is None or nxt[0] == 0.0 or int(nxt[2]) & TK.REINIT:
                    st = SEGMENT_END
                else:
                    G, Pm, qp, tp, ok = self.gain(x)
                    if not ok:
                        st = SEGMENT_END | BAD_PIVOT
                q, t, w, v = x[3:7].copy(), x[7:10].copy(), x[10:13].copy(), x[13:16].copy()
                P = x[16:].reshape(12, 12).copy()
                if st == SMOOTHED:
                    e = np.concatenate([TK.qlog(TK.qmul(xs[0], qp * [1.0, -1.0, -1.0, -1.0])), xs[1] - tp, xs[2] - w,
                                        xs[3] - v])
                    delta = np.zeros(12)
                    for i in range(12):
                        for k in range(12):
                            delta[i] += G[i, k] * e[k]
                    qn = TK._unit(TK.qmul(TK.qexp(delta[0:3]), q))
                    if qn @ q < 0.0:
                        qn = -qn
                    D = Ps - Pm
                    M = np.zeros((12, 12))
                    for m in range(12):
                        M += np.outer(G[:, m], D[m])
                    Pn = np.empty((12, 12))
                    for i in range(12):
                        for j in range(i + 1):
                            a = 0.0
                            for k in range(12):
                                a += M[i, k] * G[j, k]
                            Pn[i, j] = Pn[j, i] = P[i, j] + a
                    q, t, w, v, P = qn, t + delta[3:6], w + delta[6:9], v + delta[9:12], Pn
                xs, Ps = (q, t, w, v), P
                out['ori'][r], out['pos'][r], out['smooth_status'][r] = q, t, st
                out['cov'][r], out['rates'][r] = P[:6, :6], np.concatenate([w, v])
        return out
