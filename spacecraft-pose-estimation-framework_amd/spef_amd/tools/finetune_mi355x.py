"""Fit the URSONet head of a built experiment on an MI355X, the backbone frozen (where this replaces the reference's
train.py: INTEGRATION.md).

    python -m spef_amd.tools.finetune_mi355x --build experiments/build/mi355x/<name> [--data PATH | --synthetic N]
    python -m spef_amd.tools.finetune_mi355x --time-step [--bins 1728 1000] [--batch 64] [--optim adam]

Fit: loads ``model.spef`` + ``config.yaml``, runs the frozen backbone once over the dataset (``Engine.features``) into a
device cache of pooled features, encodes the targets on the device (``Engine.encode_targets``), then runs TRAIN.N_EPOCH
epochs of shuffled mini-batches of the cache through ``HeadTrainer.step`` with the loss train.py builds
(``SPELoss(ORI, POS, beta=1, norm_distance=True)``, train.py:83), TRAIN.OPTIM / LR / MOMENTUM / DECAY and the
reference's MultiStepLR or OnPlateau schedule (src/solver/optimizer.py:59-73) on the host. The last ``--valid-frac`` of the
frames is the validation split; the head of lowest validation loss is kept (src/tools/training.py:176-179). Writes
``finetune/model.spef`` (``blob.replace_head``) and ``finetune/finetune.json`` (losses, ``Engine.scorer`` error curves on
the validation split, timings) next to the build. There is no augmentation per epoch: the features are cached.

--time-step: HIP-event microseconds per captured step of a standalone trainer at K = 1280 (many graph replays after a
warm-up), beside the same step in eager PyTorch-ROCm (``F.linear``, the reference's loss, ``backward``,
``torch.optim``) and the byte floor: W and the optimizer state read once and written once at the copy rate
``spef_measure_peaks`` reports.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time


class _Plateau:
    """torch's ReduceLROnPlateau(mode='min', factor, patience) with its default relative threshold 1e-4."""

    def __init__(self, lr, factor, patience):
        self.lr, self.factor, self.patience, self.best, self.bad = lr, factor, patience, float('inf'), 0

    def step(self, epoch, loss):
        if loss < self.best * (1 - 1e-4):
            self.best, self.bad = loss, 0
        else:
            self.bad += 1
        if self.bad > self.patience:
            self.lr, self.bad = self.lr * self.factor, 0
        return self.lr


class _MultiStep:
    def __init__(self, lr, factor, milestones):
        self.lr0, self.factor, self.milestones = lr, factor, sorted(milestones)

    def step(self, epoch, loss):   # after epoch `epoch` (0-based): the rate of epoch + 1
        return self.lr0 * self.factor ** sum(1 for m in self.milestones if m <= epoch + 1)


def _event_us(fn, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def time_step(n_ori, n_pos, B, optim, K=1280, warmup=50, reps=500, device=0):
    """-> dict: microseconds per step (fused, captured; eager PyTorch), the byte floor and the copy rate behind it."""
    import torch
    from .. import _lib as L
    from ..engine import Engine
    dev = torch.device(f'cuda:{device}')
    g = torch.Generator(device='cpu').manual_seed(1)
    X = (torch.randn((B, K), generator=g) / K ** 0.5).to(dev)
    to = torch.softmax(torch.randn((B, n_ori), generator=g) * 3, dim=1).to(dev)
    pos_mode = 'regression' if n_pos == 3 else 'classification'
    tp = (torch.randn((B, 3), generator=g) if n_pos == 3 else
          torch.softmax(torch.randn((B, n_pos), generator=g) * 3, dim=1)).to(dev)
    W0 = torch.randn((n_ori + n_pos, K), generator=g) * 0.01
    eng = Engine(None, dev)
    tr = eng.head_trainer(K, n_ori, n_pos, optimizer=optim, pos_mode=pos_mode, norm_distance=True, Bmax=B, lr=1e-3,
                          weight_decay=1e-4)
    tr.set_weights(W0, torch.zeros(n_ori + n_pos))
    loss = torch.empty(3, dtype=torch.float32, device=dev)
    for _ in range(3):
        tr.step(X, to, tp, loss=loss)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tr.step(X, to, tp, loss=loss)
    for _ in range(warmup):
        graph.replay()
    fused = min(_event_us(graph.replay, reps) for _ in range(3))
    stream = min(_event_us(lambda: tr.step(X, to, tp, loss=loss), reps) for _ in range(3))
    tr.close()
    del graph
    # the same step in eager PyTorch
    lin = torch.nn.Linear(K, n_ori + n_pos).to(dev)
    with torch.no_grad():
        lin.weight.copy_(W0.to(dev))
    opt = (torch.optim.Adam(lin.parameters(), lr=1e-3, weight_decay=1e-4) if optim == 'adam' else
           torch.optim.SGD(lin.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4))

    def eager():
        opt.zero_grad()
        z = torch.nn.functional.linear(X, lin.weight, lin.bias)
        lo = torch.mean(torch.sum(-(to * torch.log(torch.softmax(z[:, :n_ori], dim=1))), dim=1))
        if n_pos == 3:
            lp = torch.linalg.norm(z[:, n_ori:] - tp) / torch.linalg.norm(tp)
        else:
            lp = torch.mean(torch.sum(-(tp * torch.log(torch.softmax(z[:, n_ori:], dim=1))), dim=1))
        (lo + lp).backward()
        opt.step()
    for _ in range(warmup):
        eager()
    eager_us = min(_event_us(eager, reps) for _ in range(3))
    eng.close()
    peaks = (C.c_double * 8)()
    L.check(L.load().spef_measure_peaks(device, 3, peaks))
    Np = (n_ori + n_pos + 15) // 16 * 16
    state = 2 if optim == 'adam' else 1
    nbytes = 2.0 * (1 + state) * Np * K * 4          # W and the state, read once and written once
    return dict(K=K, n_ori=n_ori, n_pos=n_pos, B=B, optimizer=optim, fused_graph_us=fused, fused_stream_us=stream,
                eager_torch_us=eager_us, copy_GBps=peaks[2], state_bytes=nbytes, byte_floor_us=nbytes / peaks[2] * 1e-3)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--build')
    ap.add_argument('--data', help='SPEED dataset root (images/, train.json)')
    ap.add_argument('--synthetic', type=int, default=256, help='synthetic frames when --data is absent')
    ap.add_argument('--epochs', type=int, help='default: TRAIN.N_EPOCH')
    ap.add_argument('--batch', type=int, default=64, help='mini-batch of the fit')
    ap.add_argument('--valid-frac', type=float, default=0.125)
    ap.add_argument('--dropout', type=float, default=0.2, help="the orientation branch's dropout (the reference's 0.2)")
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--time-step', action='store_true')
    ap.add_argument('--bins', type=int, nargs=2, default=(1728, 1000), help='--time-step: head widths')
    ap.add_argument('--optim', choices=('sgd', 'adam'), help='default: TRAIN.OPTIM (--time-step: adam)')
    ap.add_argument('--lr', type=float, help='default: TRAIN.LR')
    a = ap.parse_args(argv)
    if a.time_step:
        print(json.dumps(time_step(a.bins[0], a.bins[1], a.batch, a.optim or 'adam')))
        return 0
    if not a.build:
        ap.error('--build is required for a fit')
    import numpy as np
    import torch
    from .. import _lib as L
    from .. import blob as Bl
    from ..config import load_config, to_spe_utils
    from ..data.synthetic import speed_like_loader
    from ..engine import Engine
    from ..solver import head_fit as HF
    from ..spe.camera import CAMERAS

    cfg = load_config(os.path.join(a.build, 'config.yaml'))
    h, t = cfg.MODEL.HEAD, cfg.TRAIN
    assert h.ORI == 'classification', 'the head fit trains the orientation branch in classification mode only'
    dev = torch.device(f'cuda:{cfg.MI355X.DEVICE}')
    su = to_spe_utils(cfg, CAMERAS['speed_plus' if 'plus' in cfg.DATA.PATH else 'speed'])
    with open(os.path.join(a.build, 'model.spef'), 'rb') as f:
        blob0 = f.read()
    eng = Engine(blob0, dev)
    eng.set_decode_tables(su.orientation.histogram, su.position.histogram if h.POS == 'classification' else None)
    FB, size = cfg.MI355X.BATCH_SIZE, tuple(cfg.DATA.IMG_SIZE)
    if a.data:
        from ..data.speed import speed_frames
        it = ((eng.preprocess(fr.to(dev).contiguous(), size), tg) for fr, tg in
              speed_frames(os.path.join(a.data, 'images', 'train'), os.path.join(a.data, 'train.json'), FB))
    else:
        it = ((im['torch'].to(dev), tg) for im, tg in speed_like_loader((a.synthetic + FB - 1) // FB, FB, size))

    # ---- one pass of the frozen backbone into a device cache
    t0 = time.perf_counter()
    feats, quats, poss = [], [], []
    for fr, tg in it:
        feats.append(eng.features(fr.contiguous()))
        quats.append(np.asarray(tg['ori'], np.float64))
        poss.append(np.asarray(tg['pos'], np.float64))
    X = torch.cat(feats)
    q, p = np.concatenate(quats), np.concatenate(poss)
    N = X.shape[0]
    mask = None if h.ORI_DELETE_UNUSED_BINS else su.orientation.redundant_flags
    tg = eng.encode_targets(q, p if h.POS == 'classification' else None,
                            HF.soft_variance(cfg.DATA.ORI_SMOOTH_FACTOR, h.N_ORI_BINS_PER_DIM),
                            HF.soft_variance(cfg.DATA.POS_SMOOTH_FACTOR, h.N_POS_BINS_PER_DIM), mask)
    if int(tg['status'].any()):
        raise ValueError('a pose could not be encoded (non-finite, or outside every bin)')   # the reference raises too
    To = tg['ori_soft']
    Tp = tg['pos_soft'] if h.POS == 'classification' else torch.from_numpy(p.astype(np.float32)).to(dev)
    torch.cuda.synchronize(dev)
    t_feat = time.perf_counter() - t0

    n_val = max(1, int(round(N * a.valid_frac)))
    n_tr = N - n_val
    assert n_tr >= 1, 'no training frames left'
    B = min(a.batch, n_tr)
    lr0 = a.lr if a.lr is not None else t.LR
    # the loss is train.py's: SPELoss(ORI, POS, beta=1, norm_distance=True) (train.py:83)
    tr = eng.head_trainer(optimizer=a.optim or t.OPTIM.lower(), pos_mode=h.POS, beta=1.0, norm_distance=True,
                          momentum=t.MOMENTUM, weight_decay=t.DECAY, dropout_p=a.dropout, seed=a.seed, Bmax=max(B, min(n_val, 1024)), lr=lr0)
    sched = (_Plateau(lr0, t.GAMMA, t.MILESTONES[0]) if t.SCHEDULER == 'OnPlateau' else
             _MultiStep(lr0, t.GAMMA, t.MILESTONES))
    scorer = eng.scorer(1, 1, n_val)
    modes = {'regression': L.REGRESSION, 'classification': L.CLASSIFICATION}
    q_val = torch.from_numpy(q[n_tr:].astype(np.float32)).to(dev)
    p_val = torch.from_numpy(p[n_tr:].astype(np.float32)).to(dev)
    gen = torch.Generator(device='cpu').manual_seed(a.seed)
    n_epoch = a.epochs if a.epochs is not None else t.N_EPOCH
    steps = (n_tr + B - 1) // B
    rec = {'train_loss': [], 'valid_loss': [], 'lr': [], 'ori_error': [], 'pos_error': [], 'esa_score': []}
    best = (float('inf'), -1, None)
    lr = lr0
    t0 = time.perf_counter()
    for ep in range(n_epoch):
        perm = torch.randperm(n_tr, generator=gen).to(dev)
        losses = torch.zeros((steps, 3), dtype=torch.float32, device=dev)
        sizes = []
        for s in range(steps):
            idx = perm[s * B:(s + 1) * B]
            sizes.append(idx.numel())
            tr.step(X[idx], To[idx], Tp[idx], loss=losses[s])
        # validation: loss by chunks of Bmax, poses decoded and scored on the device
        vl, scorer_rows = [], 0
        scorer.reset()
        for v0 in range(n_tr, N, tr.Bmax):
            sl = slice(v0, min(v0 + tr.Bmax, N))
            out = tr.evaluate(X[sl], To[sl], Tp[sl], want_logits=True)
            z = out['logits']
            dec = eng.decode(modes[h.ORI], modes[h.POS], z[:, :tr.n_ori].contiguous(), z[:, tr.n_ori:].contiguous(),
                             want_soft=False)
            scorer.step(0, dec, (q_val[sl.start - n_tr:sl.stop - n_tr], p_val[sl.start - n_tr:sl.stop - n_tr]))
            vl.append((out['loss'], sl.stop - sl.start))
        w = np.array(sizes, np.float64)
        train_loss = float(np.sum(losses.cpu().numpy()[:, 0].astype(np.float64) * w) / w.sum())
        valid_loss = float(sum(float(l[0]) * n for l, n in vl) / n_val)
        res = scorer.result()
        rec['train_loss'].append(train_loss)
        rec['valid_loss'].append(valid_loss)
        rec['lr'].append(lr)
        for k in ('ori_error', 'pos_error', 'esa_score'):
            rec[k].append(float(res[k][0, 0]))
        if valid_loss < best[0]:
            best = (valid_loss, ep, tuple(x.clone() for x in tr.weights()))
        lr = sched.step(ep, train_loss)
        tr.set_lr(lr)
        print(f'epoch {ep}: train {train_loss:.4f} valid {valid_loss:.4f} ori {rec["ori_error"][-1]:.2f} deg '
              f'pos {rec["pos_error"][-1]:.3f} m', flush=True)
    torch.cuda.synchronize(dev)
    t_fit = time.perf_counter() - t0
    out_dir = os.path.join(a.build, 'finetune')
    os.makedirs(out_dir, exist_ok=True)
    W, b = (x.cpu().numpy() for x in best[2])
    n0 = tr.n_ori
    with open(os.path.join(out_dir, 'model.spef'), 'wb') as f:
        f.write(Bl.replace_head(blob0, W[:n0], b[:n0], W[n0:], b[n0:]))
    rec.update(best_epoch=best[1], best_valid_loss=best[0], frames=N, train_frames=n_tr, valid_frames=n_val, batch=B,
               epochs=n_epoch, feature_pass_s=t_feat, fit_s=t_fit, steps_per_epoch=steps,
               us_per_step=t_fit / max(1, n_epoch * steps) * 1e6)
    with open(os.path.join(out_dir, 'finetune.json'), 'w') as f:
        json.dump(rec, f, indent=1)
    print(f'features {t_feat:.2f} s ({N / t_feat:.0f} frames/s), fit {t_fit:.2f} s for {n_epoch} epochs of {steps} steps; '
          f'best epoch {best[1]} (valid loss {best[0]:.4f}) -> {out_dir}/model.spef')
    tr.close()
    scorer.close()
    eng.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
