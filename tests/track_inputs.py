"""Inputs shared by tests/test_track_host.py and tests/test_gpu_track.py (not a test module)."""
import numpy as np

from spef_amd.spe import track as TK

N = 64
W_TRUE = np.array([0.01, -0.02, 0.015])       # rad per frame, left perturbation in the camera frame
V_TRUE = np.array([0.004, -0.003, -0.03])     # m per frame
Q0 = np.array([0.5, 0.5, -0.5, 0.5])
T0 = np.array([0.2, -0.1, 9.0])
SIGMA = np.array([0.01, 0.01, 0.01, 0.01, 0.01, 0.1])   # rad, rad, rad, m, m, m
GATE = 22.458                                 # chi^2, 6 degrees of freedom, 99.9 %
PARAMS = dict(q=(0, 0, 1e-8, 1e-8), p0=(1, 1, 1e-2, 1e-2), r=0, cov_scale=1.0, gate_chi2=GATE, max_coast=3)
ANCHOR = dict(q=1, p0=1, r=100, cov_scale=1.0, gate_chi2=0.0, max_coast=0)   # the reference's position filter


def truth(n=N):
    """-> (q [n x 4], t [n x 3]) of the constant-rate trajectory: q_{k+1} = exp(w) (x) q_k, t_{k+1} = t_k + v."""
    q, t = np.empty((n, 4)), np.empty((n, 3))
    q[0], t[0] = Q0, T0
    for k in range(1, n):
        q[k] = TK.qmul(TK.qexp(W_TRUE), q[k - 1])
        q[k] /= np.linalg.norm(q[k])
        t[k] = t[k - 1] + V_TRUE
    return q, t


def rotate(q, w):
    """exp(w) (x) q for every row."""
    return np.stack([TK.qmul(TK.qexp(np.asarray(w, np.float64)), qi) for qi in q])


def standard():
    """The standard trajectory (H3): default_rng(3) noise of SIGMA on every frame, its covariance with every row ->
    (quat [64 x 4], pos [64 x 3], cov [64 x 6 x 6], status [64] int32), float64 measurements."""
    q, t = truth()
    noise = np.random.default_rng(3).normal(0.0, 1.0, (N, 6)) * SIGMA
    qm = np.stack([TK.qmul(TK.qexp(noise[k, :3]), q[k]) for k in range(N)])
    tm = t + noise[:, 3:]
    cov = np.tile(np.diag(SIGMA ** 2), (N, 1, 1))
    return qm, tm, cov, np.zeros(N, np.int32)


def dropouts():
    """H4: frames 20..25 carry decode status 8; frame 40 is rotated 0.5 rad about x and moved 2 m in z."""
    qm, tm, cov, st = standard()
    st[20:26] = 8
    qm[40:41] = rotate(qm[40:41], [0.5, 0, 0])
    tm[40, 2] += 2.0
    return qm, tm, cov, st


def jump():
    """H5: a permanent jump from frame 30 on (0.8 rad about y, +(0.5, 0, 3) m)."""
    qm, tm, cov, st = standard()
    qm[30:] = rotate(qm[30:], [0, 0.8, 0])
    tm[30:] += [0.5, 0.0, 3.0]
    return qm, tm, cov, st


def three_streams():
    """H3, H4 and H5 side by side as S = 3 time-major rows -> (quat [192 x 4], pos, cov [192 x 6 x 6], status)."""
    parts = (standard(), dropouts(), jump())
    return tuple(np.stack([p[i] for p in parts], axis=1).reshape((N * 3,) + parts[0][i].shape[1:]) for i in range(4))


def angle_rad(qa, qb):
    """Rotation angle between unit quaternions, row by row."""
    d = np.abs(np.sum(np.asarray(qa, np.float64) * np.asarray(qb, np.float64), axis=-1))
    return 2.0 * np.arccos(np.clip(d, 0.0, 1.0))
