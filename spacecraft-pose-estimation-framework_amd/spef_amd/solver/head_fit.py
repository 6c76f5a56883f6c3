"""NumPy twin and specification of the head-fit path (csrc/k_headfit.hip, include/spef.h ``spef_headfit_*``).

The device fits the URSONet head's two Linear layers (ursonet.py:17-25) over cached backbone features; this module states
every step it takes, in the order it takes them, and is what the tests hold the kernels to. The reference lines:

  targets    OrientationSoftClassification.encode / PositionSoftClassification.encode (classification_utils.py:85-111,
             :217-240)
  dropout    nn.Dropout(0.2) on the orientation branch's input (ursonet.py); the mask is this module's hash, not torch's
             generator
  loss       SPEUtils.last_activ's softmax (spe_utils.py:75-79) + SoftClassLoss (loss.py:109); PosRegLoss (loss.py:35-37)
             as written -- ``torch.linalg.norm(pred - target)`` is the Frobenius norm over the whole batch;
             SPELoss.compute_loss (loss.py:157): beta * ori + pos
  optimizer  torch.optim.SGD(momentum, weight_decay) / torch.optim.Adam(weight_decay) as import_optimizer builds them
             (optimizer.py:45-57): L2 decay added to the gradient

Every function works in the dtype of its array arguments: float64 arrays give the float64 mathematics (held to torch's
autograd and optimizers by tests/golden/head_fit.npz), float32 arrays give the device's float32 operation order, one
rounding per operation and no fused multiply-adds.
"""
from __future__ import annotations

import numpy as np

SGD, ADAM = 0, 1
ADAM_DEFAULTS = dict(beta1=0.9, beta2=0.999, eps=1e-8)


# ------------------------------------------------------------------------------------------------------ target encoding
def encode_orientation(q, hist, var, mask=None) -> np.ndarray:
    """q [B x 4], hist [n x 4] float64 -> float32 [B x n]: k = exp(-((2 acos(min(1, |q . h|)) / pi)^2) / (2 var)), 0 where
    ``mask`` (the reference's redundant_flags) is set, normalised by its sum. A row whose input is not finite or whose sum
    is zero is NaN (the reference raises)."""
    q = np.atleast_2d(np.asarray(q, np.float64))
    hist = np.asarray(hist, np.float64)
    out = np.full((q.shape[0], hist.shape[0]), np.nan, np.float32)
    for b in range(q.shape[0]):
        if not np.all(np.isfinite(q[b])):
            continue
        dot = ((q[b, 0] * hist[:, 0] + q[b, 1] * hist[:, 1]) + q[b, 2] * hist[:, 2]) + q[b, 3] * hist[:, 3]
        a = 2.0 * np.arccos(np.minimum(1.0, np.abs(dot))) / np.pi
        k = np.exp(-(a * a) * (1.0 / (2.0 * var)))
        if mask is not None:
            k[np.asarray(mask, bool)] = 0.0
        s = np.sum(k)
        if np.isfinite(s) and s > 0.0:
            out[b] = (k / s).astype(np.float32)
    return out


def encode_position(t, grid, var) -> np.ndarray:
    """t [B x 3], grid [n x 3] float64 -> float32 [B x n]: k = exp(-|t - g|^2 / (2 var)) normalised by its sum."""
    t = np.atleast_2d(np.asarray(t, np.float64))
    grid = np.asarray(grid, np.float64)
    out = np.full((t.shape[0], grid.shape[0]), np.nan, np.float32)
    for b in range(t.shape[0]):
        if not np.all(np.isfinite(t[b])):
            continue
        d = t[b] - grid
        k = np.exp(-((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) * (1.0 / (2.0 * var)))
        s = np.sum(k)
        if np.isfinite(s) and s > 0.0:
            out[b] = (k / s).astype(np.float32)
    return out


def soft_variance(smooth: float, n_bins_per_dim: int) -> float:
    """(smooth / n_bins_per_dim)^2 / 12: the variance both encoders use (classification_utils.py:96, :228)."""
    return (smooth / n_bins_per_dim) ** 2 / 12


# ------------------------------------------------------------------------------------------------------ dropout
def dropout_hash(seed: int, step: int, idx) -> np.ndarray:
    """uint32 hash of (seed, step, element index b * K + k), all arithmetic modulo 2^32: murmur3's 32-bit finaliser of
    ``idx * 0x9E3779B1 + seed`` xor ``step * 0x85EBCA77``."""
    m = np.uint64(0xFFFFFFFF)
    x = (np.asarray(idx, np.uint64) * np.uint64(0x9E3779B1) + np.uint64(seed & 0xFFFFFFFF)) & m
    x ^= (np.uint64(step & 0xFFFFFFFF) * np.uint64(0x85EBCA77)) & m
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & m
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & m
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def dropout_keep(seed: int, step: int, B: int, K: int, p: float) -> np.ndarray:
    """bool [B x K]: element (b, k) of step ``step`` (0 = the first training step after a reset) is kept when its hash is
    at least floor(p * 2^32)."""
    thr = np.uint32(int(np.floor(p * 4294967296.0)))
    return dropout_hash(seed, step, np.arange(B * K, dtype=np.uint64)).reshape(B, K) >= thr


def dropout_apply(X: np.ndarray, keep: np.ndarray, p: float) -> np.ndarray:
    """Xd = X * float32(1 / (1 - p)) where kept, 0 elsewhere (one float32 product)."""
    inv = X.dtype.type(1.0 / (1.0 - p))
    return np.where(keep, X * inv, X.dtype.type(0))


# ------------------------------------------------------------------------------------------------------ loss and G
def log_softmax_parts(z: np.ndarray):
    """m = max z, d = z - m in z's dtype (exact for the maximum, one rounding elsewhere), then in float64: e = exp(d),
    s = sum e, p = e / s, log p = d - log s. -> (p, log p), float64."""
    d = (z - np.max(z, axis=1, keepdims=True)).astype(np.float64)
    e = np.exp(d)
    s = np.sum(e, axis=1, keepdims=True)
    return e / s, d - np.log(s)


def loss_and_g(z_ori, t_ori, z_pos, t_pos, beta=1.0, pos_mode='classification', norm_distance=False):
    """-> ((total, ori, pos) float64, G float64 [B x (n_ori + n_pos)]), G = d total / d logits.

    Classification heads: loss = mean_b -sum_i t log p; G = (p - t) * scale / B with scale = beta (ori) or 1 (pos); this
    is the gradient for targets that sum to 1, which both encoders produce. Position regression: loss = |pred - target|_F
    (/ |target|_F with norm_distance) over the whole batch; G = (pred - target) / |pred - target|_F (/ |target|_F), zero
    at a zero norm."""
    B = z_ori.shape[0]
    p, lp = log_softmax_parts(z_ori)
    t = np.asarray(t_ori, np.float64)
    lo = float(np.mean(-np.sum(t * lp, axis=1)))
    g_ori = (p - t) * (beta / B)
    tp = np.asarray(t_pos, np.float64)
    if pos_mode == 'regression':
        d = np.asarray(z_pos, np.float64) - tp
        nd, nt = float(np.sqrt(np.sum(d * d))), float(np.sqrt(np.sum(tp * tp)))
        lpos = nd / nt if norm_distance else nd
        g_pos = np.zeros_like(d)
        if nd > 0.0:
            g_pos = d / nd
            if norm_distance:
                g_pos = g_pos / nt
    else:
        pp, lpp = log_softmax_parts(z_pos)
        lpos = float(np.mean(-np.sum(tp * lpp, axis=1)))
        g_pos = (pp - tp) * (1.0 / B)
    return (beta * lo + lpos, lo, lpos), np.concatenate([g_ori, g_pos], axis=1)


def g_bound(z_ori, t_ori, z_pos, t_pos, beta=1.0):
    """(p + t) * scale / B per element: what a float32 evaluation of G is held to (times a few eps)."""
    B = z_ori.shape[0]
    p, _ = log_softmax_parts(z_ori)
    pp, _ = log_softmax_parts(z_pos)
    return np.concatenate([(p + t_ori) * (beta / B), (pp + t_pos) * (1.0 / B)], axis=1)


def gradients(G, Xo, Xp, n_ori):
    """dW [n x K] = G^T Xsel -- the rows below n_ori against Xo (the dropout copy of X), the rest against Xp = X -- and
    db [n] = sum_b G, in float64."""
    G = np.asarray(G, np.float64)
    dW = np.concatenate([G[:, :n_ori].T @ np.asarray(Xo, np.float64), G[:, n_ori:].T @ np.asarray(Xp, np.float64)])
    return dW, G.sum(axis=0)


def forward(X, W, b):
    """Logits in float64."""
    return np.asarray(X, np.float64) @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)


# ------------------------------------------------------------------------------------------------------ optimizers
def sgd_step(w, buf, g, lr, momentum=0.9, weight_decay=0.0):
    """torch.optim.SGD, dampening 0, no Nesterov: g += wd * w; buf = momentum * buf + g (a zero buffer makes the first
    step torch's ``buf = g``); w -= lr * buf. Each line below is one rounding per element in w's dtype. -> (w, buf)."""
    f = w.dtype.type
    t0 = f(weight_decay) * w
    g = g.astype(w.dtype) + t0
    t1 = f(momentum) * buf
    buf = t1 + g
    t2 = f(lr) * buf
    return w - t2, buf


def adam_bias(step: int, beta1=0.9, beta2=0.999):
    """(1 - beta1^t, sqrt(1 - beta2^t)) of step t (1-based), in float64."""
    return 1.0 - beta1 ** step, float(np.sqrt(1.0 - beta2 ** step))


def adam_step(w, m, v, g, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    """torch.optim.Adam (no amsgrad) at 1-based step ``step``: g += wd * w; m = beta1 * m + (1 - beta1) * g;
    v = beta2 * v + ((1 - beta2) * g) * g; w -= (lr / bc1) * (m / (sqrt(v) / bc2s + eps)), the bias corrections computed
    in float64 and rounded to w's dtype, as are 1 - beta1 and 1 - beta2. -> (w, m, v)."""
    f = w.dtype.type
    bc1, bc2s = adam_bias(step, beta1, beta2)
    t0 = f(weight_decay) * w
    g = g.astype(w.dtype) + t0
    t1 = f(beta1) * m
    t2 = f(1.0 - beta1) * g
    m = t1 + t2
    t3 = f(beta2) * v
    t4 = f(1.0 - beta2) * g
    t5 = t4 * g
    v = t3 + t5
    den = np.sqrt(v) / f(bc2s) + f(eps)
    ss = f(lr) / f(bc1)
    t6 = m / den
    t7 = ss * t6
    return w - t7, m, v


class HeadFitTwin:
    """The whole trainer in NumPy, in ``dtype`` (float64: the mathematics; float32: the device's operation order for the
    optimizer, the loss and G still evaluated in float64 from the logits)."""

    def __init__(self, K, n_ori, n_pos, optimizer='sgd', pos_mode='classification', beta=1.0, norm_distance=False,
                 momentum=0.9, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, dropout_p=0.0, seed=0,
                 dtype=np.float64):
        self.K, self.n_ori, self.n_pos = K, n_ori, n_pos
        self.optimizer, self.pos_mode, self.beta, self.norm_distance = optimizer, pos_mode, beta, norm_distance
        self.momentum, self.beta1, self.beta2, self.eps, self.weight_decay = momentum, beta1, beta2, eps, weight_decay
        self.dropout_p, self.seed, self.dtype = dropout_p, seed, np.dtype(dtype)
        n = n_ori + n_pos
        self.W, self.b = np.zeros((n, K), dtype), np.zeros(n, dtype)
        self.reset_state()

    def reset_state(self):
        self.state = [np.zeros_like(self.W), np.zeros_like(self.b), np.zeros_like(self.W), np.zeros_like(self.b)]
        self.steps = 0

    def set_weights(self, W, b):
        self.W, self.b = np.array(W, self.dtype), np.array(b, self.dtype)

    def evaluate(self, X, t_ori, t_pos):
        z = forward(X, self.W, self.b)
        return loss_and_g(z[:, :self.n_ori], t_ori, z[:, self.n_ori:], t_pos, self.beta, self.pos_mode,
                          self.norm_distance)[0]

    def step(self, X, t_ori, t_pos, lr):
        X = np.asarray(X, self.dtype)
        Xo = X
        if self.dropout_p > 0.0:
            Xo = dropout_apply(X, dropout_keep(self.seed, self.steps, X.shape[0], self.K, self.dropout_p), self.dropout_p)
        z = np.concatenate([forward(Xo, self.W[:self.n_ori], self.b[:self.n_ori]),
                            forward(X, self.W[self.n_ori:], self.b[self.n_ori:])], axis=1).astype(self.dtype)
        loss, G = loss_and_g(z[:, :self.n_ori], t_ori, z[:, self.n_ori:], t_pos, self.beta, self.pos_mode,
                             self.norm_distance)
        dW, db = gradients(G.astype(self.dtype), Xo, X, self.n_ori)
        self.apply(dW.astype(self.dtype), db.astype(self.dtype), lr)
        return loss

    def apply(self, dW, db, lr):
        """One optimizer step from given gradients."""
        self.steps += 1
        s = self.state
        if self.optimizer == 'sgd':
            self.W, s[0] = sgd_step(self.W, s[0], dW, lr, self.momentum, self.weight_decay)
            self.b, s[1] = sgd_step(self.b, s[1], db, lr, self.momentum, self.weight_decay)
        else:
            self.W, s[0], s[2] = adam_step(self.W, s[0], s[2], dW, lr, self.steps, self.beta1, self.beta2, self.eps,
                                           self.weight_decay)
            self.b, s[1], s[3] = adam_step(self.b, s[1], s[3], db, lr, self.steps, self.beta1, self.beta2, self.eps,
                                           self.weight_decay)
