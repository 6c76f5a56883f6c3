"""Cases and an independent reference for the pose tracker, shared by tests/test_track_cases_host.py and
tests/test_gpu_track_cases.py (not a test module).

``textbook`` is an error-state Kalman filter written from the model in the docstring of spef_amd/spe/track.py, not from
the twin's code: explicit 12 x 12 F P F^T + Q, H = [I6 0], the gain through ``np.linalg.solve``, the Joseph form of the
covariance update, quaternion products as 4 x 4 matrices. It shares no arithmetic with the twin's factored update, so
an error in the algorithm that the kernel and the twin have in common shows as a disagreement with it. ``VARIANTS`` are
four such errors, planted in the textbook filter only (tests/test_track_cases_host.py measures what each one moves).

A case is (params, quat, pos, cov or None, status) of one stream, seeded, already rounded to the float32 / int32 the
kernel reads. ``reference(name)`` runs the twin, the twin on measurements perturbed by 1e-9 (relative) and the textbook
filter on a case once and derives the bound of every output by the rule of tests/test_gpu_track.py
(``test_kernel_matches_twin``): max(10 x sensitivity, 16 float32 ulps) of the output's largest magnitude.
"""
import collections
import functools

import numpy as np

from spef_amd.spe import track as TK

import track_inputs as TI

ULP16 = 16 * 2.0 ** -23
KEYS = ('ori', 'pos', 'mahalanobis', 'cov', 'rates')          # compared under the rule; track_status must be equal
VARIANTS = ('rate_right', 'cov_unsym', 'no_cross', 'no_cov_scale')

Case = collections.namedtuple('Case', 'params quat pos cov status sigma')
Ref = collections.namedtuple('Ref', 'twin pert text diag bounds state')
Bound = collections.namedtuple('Bound', 'mag sens tol absolute')


# ------------------------------------------------------------------------------------- the textbook filter
def _qmat(a):
    """The 4 x 4 matrix of the Hamilton product from the left: a (x) b = _qmat(a) @ b (scalar first)."""
    w, x, y, z = a
    return np.array([[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]])


def _rotvec_quat(r):
    """The unit quaternion of the rotation vector r: (cos(|r| / 2), sin(|r| / 2) r / |r|)."""
    th = np.linalg.norm(r)
    return np.concatenate([[np.cos(0.5 * th)], 0.5 * np.sinc(th / (2.0 * np.pi)) * r])


def textbook(params, quat, pos, cov=None, status=None, variant=None):
    """One stream through the textbook filter -> (outputs like ``PoseTrackerHost.step``, diagnostics). Diagnostics per
    row: 'angle' the innovation's rotation angle in rad, 'from_cov' 1 when R came from ``cov`` and 0 when it fell back
    to r, 'pivot' the smallest Cholesky pivot of S relative to its diagonal entry (0 when S has no factor),
    'gate_ratio' d2 / gate_chi2; NaN / -1 on rows that have no innovation."""
    assert variant is None or variant in VARIANTS
    pq, p0, pr, cov_scale, gate, max_coast = TK.check_params(**params)
    if variant == 'no_cov_scale':
        cov_scale = 1.0
    quat, pos = np.asarray(quat, np.float64), np.asarray(pos, np.float64)
    n = quat.shape[0]
    status = np.zeros(n, np.int64) if status is None else np.asarray(status)
    F = np.eye(12)
    F[:6, 6:] = np.eye(6)
    H = np.hstack([np.eye(6), np.zeros((6, 6))])
    Q = np.diag(np.repeat(pq, 3))
    out = {'ori': np.empty((n, 4)), 'pos': np.empty((n, 3)), 'mahalanobis': np.full(n, np.nan),
           'track_status': np.zeros(n, np.int32), 'cov': np.full((n, 6, 6), np.nan), 'rates': np.full((n, 6), np.nan)}
    diag = {'angle': np.full(n, np.nan), 'from_cov': np.full(n, -1), 'pivot': np.full(n, np.nan),
            'gate_ratio': np.full(n, np.nan)}
    have, coast = False, 0
    xq = xt = xw = xv = P = None

    def start(qm, tm, prev):
        q0 = qm / np.linalg.norm(qm)
        if prev is not None and q0 @ prev < 0.0:
            q0 = -q0
        return q0, tm.copy(), np.zeros(3), np.zeros(3), np.diag(np.repeat(p0, 3))

    for k in range(n):
        qm, tm = quat[k], pos[k]
        valid = (int(status[k]) & 15) == 0 and bool(np.isfinite(qm).all()) and bool(np.isfinite(tm).all())
        valid = valid and 0.0 < float(qm @ qm) < np.inf
        ts = 0
        if not have:
            if not valid:
                out['ori'][k], out['pos'][k], out['track_status'][k] = qm, tm, TK.INVALID | TK.NO_TRACK
                continue
            xq, xt, xw, xv, P = start(qm, tm, None)
            have, coast = True, 0
            out['mahalanobis'][k] = 0.0
        else:
            e = _rotvec_quat(xw)
            qp = _qmat(xq) @ e if variant == 'rate_right' else _qmat(e) @ xq
            qp = qp / np.linalg.norm(qp)
            tp = xt + xv
            Pm = F @ P @ F.T + Q
            if variant == 'no_cross':
                Pm[:6, :6] -= P[:6, 6:] + P[6:, :6]
            ok = False
            if valid:
                d = _qmat(qm / np.linalg.norm(qm)) @ (qp * [1.0, -1.0, -1.0, -1.0])
                if d[0] < 0.0:
                    d = -d
                nv = np.linalg.norm(d[1:])
                ang = 2.0 * np.arctan2(nv, d[0])
                y = np.concatenate([ang * d[1:] / nv if nv > 0.0 else np.zeros(3), tm - tp])
                from_cov = cov is not None and bool(np.isfinite(cov[k]).all())
                if from_cov:
                    c = np.asarray(cov[k], np.float64).reshape(6, 6)
                    R = cov_scale * (c if variant == 'cov_unsym' else 0.5 * (c + c.T))
                else:
                    R = np.diag(np.repeat(pr, 3))
                S = H @ Pm @ H.T + R
                diag['angle'][k], diag['from_cov'][k] = ang, int(from_cov)
                try:
                    piv = np.diag(np.linalg.cholesky(S)) ** 2
                    ok = bool(np.isfinite(S).all())
                    diag['pivot'][k] = (piv / np.diag(S)).min()
                except np.linalg.LinAlgError:
                    diag['pivot'][k] = 0.0
                if ok:
                    d2 = float(y @ np.linalg.solve(S, y))
                    out['mahalanobis'][k] = d2
                    if gate > 0.0:
                        diag['gate_ratio'][k] = d2 / gate
                        if d2 > gate:
                            ts = TK.GATED
            if not ok:
                ts = TK.INVALID
            if ts and ts == TK.GATED and coast + 1 > max_coast:
                xq, xt, xw, xv, P = start(qm, tm, xq)
                coast, ts = 0, TK.GATED | TK.REINIT
            elif ts:
                coast += 1
                xq, xt, P = (-qp if qp @ xq < 0.0 else qp), tp, Pm
            else:
                K = np.linalg.solve(S.T, (Pm @ H.T).T).T            # K = P- H^T S^-1
                delta = K @ y
                qu = _qmat(_rotvec_quat(delta[:3])) @ qp
                qu = qu / np.linalg.norm(qu)
                xq = -qu if qu @ xq < 0.0 else qu
                xt, xw, xv = tp + delta[3:6], xw + delta[6:9], xv + delta[9:12]
                IKH = np.eye(12) - K @ H
                P = IKH @ Pm @ IKH.T + K @ R @ K.T
                coast = 0
        out['ori'][k], out['pos'][k], out['track_status'][k] = xq, xt, ts
        out['cov'][k], out['rates'][k] = P[:6, :6], np.concatenate([xw, xv])
    return out, diag


# ------------------------------------------------------------------------------------------------- cases
NO_GATE = dict(TI.PARAMS, gate_chi2=0.0)
NO_COV = dict(q=(1e-6, 1e-4, 1e-8, 1e-8), p0=(1, 1, 1e-2, 1e-2), r=(1e-4, 1e-2), cov_scale=1.0, gate_chi2=0.0,
              max_coast=3)
COV_SCALE = dict(TI.PARAMS, cov_scale=4.0, max_coast=0)
BAD_ROWS = dict(TI.PARAMS, r=(1e-4, 1e-2))
BAD_SIGMA = np.array([1e-4, 1e-4, 1e-4, 1e-3, 1e-3, 1.0])
FAST_W = np.array([0.3, -0.2, 0.25])              # 0.44 rad per frame
LONG_T = 2048
HALF_TURN_ROW, OUTLIER_ROW = 32, 40


def _case(params, q, t, c, s, sigma=TI.SIGMA):
    return Case(params, np.ascontiguousarray(q, np.float32), np.ascontiguousarray(t, np.float32),
                None if c is None else np.ascontiguousarray(c, np.float32), np.ascontiguousarray(s, np.int32),
                np.asarray(sigma, np.float64))


def _trajectory(n, w, v):
    q, t = np.empty((n, 4)), np.empty((n, 3))
    q[0], t[0] = TI.Q0, TI.T0
    for k in range(1, n):
        q[k] = TK.qmul(TK.qexp(w), q[k - 1])
        q[k] /= np.linalg.norm(q[k])
        t[k] = t[k - 1] + v
    return q, t


def _measure(q, t, noise):
    return np.stack([TK.qmul(TK.qexp(noise[k, :3]), q[k]) for k in range(len(q))]), t + noise[:, 3:]


def _correlated():
    rng = np.random.default_rng(11)
    q, t = TI.truth()
    D = np.diag(TI.SIGMA)
    cov, noise = np.empty((TI.N, 6, 6)), np.empty((TI.N, 6))
    for k in range(TI.N):
        A = D @ rng.normal(size=(6, 6)) / np.sqrt(6.0)
        cov[k] = A @ A.T + 0.1 * D @ D
        noise[k] = np.linalg.cholesky(cov[k]) @ rng.normal(size=6)
        N = 0.3 * D @ rng.normal(size=(6, 6)) @ D
        cov[k] += 0.5 * (N - N.T)                       # what the symmetrisation has to remove
    qm, tm = _measure(q, t, noise)
    return _case(TI.PARAMS, qm, tm, cov, np.zeros(TI.N, np.int32))


def _badly_scaled():
    rng = np.random.default_rng(12)
    q, t = TI.truth()
    corr = np.eye(6)
    corr[3, 5] = corr[5, 3] = 0.999                     # x and z
    corr[0, 4] = corr[4, 0] = -0.99                     # theta_x and y
    c = np.diag(BAD_SIGMA) @ corr @ np.diag(BAD_SIGMA)
    noise = rng.normal(size=(TI.N, 6)) @ np.linalg.cholesky(c).T
    qm, tm = _measure(q, t, noise)
    return _case(TI.PARAMS, qm, tm, np.tile(c, (TI.N, 1, 1)), np.zeros(TI.N, np.int32), BAD_SIGMA)


def _fast_rotation():
    rng = np.random.default_rng(13)
    q, t = _trajectory(TI.N, FAST_W, TI.V_TRUE)
    qm, tm = _measure(q, t, rng.normal(size=(TI.N, 6)) * TI.SIGMA)
    return _case(NO_GATE, qm, tm, np.tile(np.diag(TI.SIGMA ** 2), (TI.N, 1, 1)), np.zeros(TI.N, np.int32))


def _double_cover():
    qm, tm, cov, st = TI.standard()
    sign = np.random.default_rng(14).choice([-1.0, 1.0], TI.N)
    sign[0] = 1.0
    return _case(TI.PARAMS, qm * sign[:, None], tm, cov, st)


def _unnormalised():
    qm, tm, cov, st = TI.standard()
    scale = 10.0 ** np.random.default_rng(15).uniform(-3.0, 3.0, TI.N)
    return _case(TI.PARAMS, qm * scale[:, None], tm, cov, st)


def _still():
    q = np.array([0.6, 0.2, -0.1, 0.5])                 # chosen so that the twin's innovation is exactly zero: with
    q /= np.linalg.norm(q)                              # the log's other branch that is 0 / 0; no component is a float32
    return _case(TI.PARAMS, np.tile(q, (TI.N, 1)), np.tile(TI.T0, (TI.N, 1)),
                 np.tile(np.diag(TI.SIGMA ** 2), (TI.N, 1, 1)), np.zeros(TI.N, np.int32))


def _half_turn():
    qm, tm, cov, st = TI.standard()
    qm[HALF_TURN_ROW:HALF_TURN_ROW + 1] = TI.rotate(qm[HALF_TURN_ROW:HALF_TURN_ROW + 1],
                                                    3.0 * np.array([1.0, 2.0, -1.0]) / np.sqrt(6.0))
    return _case(NO_GATE, qm, tm, cov, st)


def _no_cov():
    qm, tm, _, st = TI.standard()
    return _case(NO_COV, qm, tm, None, st)


def _cov_scale():
    qm, tm, cov, st = TI.standard()
    qm[OUTLIER_ROW:OUTLIER_ROW + 1] = TI.rotate(qm[OUTLIER_ROW:OUTLIER_ROW + 1], [0.5, 0, 0])
    tm[OUTLIER_ROW, 2] += 2.0
    return _case(COV_SCALE, qm, tm, cov / 4.0, st)


def _long_invalid():
    qm, tm, cov, st = TI.standard()
    st[20:30] = 8
    return _case(TI.PARAMS, qm, tm, cov, st)


STATUS_ROWS = {10: 16, 11: 32, 12: 48, 20: 1, 21: 2, 22: 4, 23: -1, 24: 8}


def _status_bits():
    qm, tm, cov, st = TI.standard()
    for k, v in STATUS_ROWS.items():
        st[k] = v
    return _case(TI.PARAMS, qm, tm, cov, st)


BAD = dict(status=0, nan_quat=1, zero_quat=10, inf_pos=14, nan_cov=18, inf_cov=22, negative_cov=30)


def _bad_rows():
    qm, tm, cov, st = TI.standard()
    st[BAD['status']] = 8
    qm[BAD['status']] = [3.0, 0, 0, 4.0]
    qm[BAD['nan_quat'], 2] = np.nan
    qm[BAD['zero_quat']] = 0.0
    tm[BAD['inf_pos'], 1] = np.inf
    cov[BAD['nan_cov'], 2, 3] = np.nan
    cov[BAD['inf_cov'], 4, 4] = np.inf
    cov[BAD['negative_cov']] = -10.0 * np.eye(6)
    return _case(BAD_ROWS, qm, tm, cov, st)


def _long():
    rng = np.random.default_rng(16)
    q, t = _trajectory(LONG_T, TI.W_TRUE / 32.0, TI.V_TRUE / 32.0)
    qm, tm = _measure(q, t, rng.normal(size=(LONG_T, 6)) * TI.SIGMA)
    return _case(TI.PARAMS, qm, tm, np.tile(np.diag(TI.SIGMA ** 2), (LONG_T, 1, 1)), np.zeros(LONG_T, np.int32))


_BUILD = {'h3': lambda: _case(TI.PARAMS, *TI.standard()), 'h4': lambda: _case(TI.PARAMS, *TI.dropouts()),
          'h5': lambda: _case(TI.PARAMS, *TI.jump()), 'correlated': _correlated, 'badly_scaled': _badly_scaled,
          'fast_rotation': _fast_rotation, 'double_cover': _double_cover, 'unnormalised': _unnormalised,
          'still': _still, 'half_turn': _half_turn, 'no_cov': _no_cov, 'cov_scale': _cov_scale,
          'long_invalid': _long_invalid, 'status_bits': _status_bits, 'bad_rows': _bad_rows, 'long': _long}
NAMES = tuple(_BUILD)
# cases that share a parameter set and a cov presence: the streams of one tracker on the device
GROUPS = (('h3', 'h4', 'h5', 'correlated', 'badly_scaled', 'double_cover', 'unnormalised', 'still', 'long_invalid',
           'status_bits'),
          ('fast_rotation', 'half_turn'), ('no_cov',), ('cov_scale',), ('bad_rows',), ('long',))


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILD[name]()


def tracked(out):
    """Rows that did not pass through."""
    return (out['track_status'] & TK.NO_TRACK) == 0


def perturbed(c):
    """The measurements of ``test_kernel_matches_twin``'s sensitivity run: every component moved by 1e-9, relative."""
    rng = np.random.default_rng(0)
    return (c.quat * (1 + 1e-9 * rng.choice([-1.0, 1.0], c.quat.shape)),
            c.pos * (1 + 1e-9 * rng.choice([-1.0, 1.0], c.pos.shape)))


def bound(c, twin, pert, key):
    """The rule: tol = max(10 x sensitivity, ULP16) of the largest magnitude of the twin's output over its tracked,
    finite entries. Where that magnitude is zero the bound is absolute: ULP16 for 'mahalanobis', ULP16 times the
    component's measurement sigma for 'rates'."""
    m = tracked(twin)
    a, b = twin[key][m], pert[key][m]
    fin = np.isfinite(a)
    mag = float(np.abs(a[fin]).max())
    if mag == 0.0:
        assert key in ('mahalanobis', 'rates'), key
        return Bound(0.0, 0.0, ULP16, ULP16 * (c.sigma if key == 'rates' else 1.0))
    sens = float(np.abs(a - b)[fin].max()) / mag
    return Bound(mag, sens, max(10.0 * sens, ULP16), None)


def error(got, want, bnd, cast=False):
    """-> (largest |got - want| over the tracked finite entries of ``want`` in units of the bound's allowance, whether
    the two are finite in the same places). ``got`` / ``want`` are one output of the tracked rows; with ``cast`` the
    reference is finite where its float32 is."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(over='ignore'):
        fin = np.isfinite(want.astype(np.float32)) if cast else np.isfinite(want)
    same = bool(np.array_equal(np.isfinite(got), fin))
    if not fin.any():
        return 0.0, same
    d = np.abs(np.where(fin, got - np.where(fin, want, 0.0), 0.0))
    allow = bnd.absolute if bnd.absolute is not None else bnd.tol * bnd.mag
    return float((d / allow).max()), same


@functools.lru_cache(maxsize=None)
def reference(name):
    """Twin, perturbed twin, textbook filter, its diagnostics, every output's bound and the twin's state row after
    the last frame for one case; computed once and left unchanged."""
    c = case(name)
    trk = TK.PoseTrackerHost(1, **c.params)
    twin = trk.step(c.quat, c.pos, c.cov, c.status)
    pq, pp = perturbed(c)
    pert = TK.PoseTrackerHost(1, **c.params).step(pq, pp, c.cov, c.status)
    text, diag = textbook(c.params, c.quat, c.pos, c.cov, c.status)
    return Ref(twin, pert, text, diag, {k: bound(c, twin, pert, k) for k in KEYS}, trk.state()[0])
