"""Record tests/golden/head_fit.npz from the REFERENCE's loss and torch's autograd / optimizers (build container only).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_headfit_golden.py <reference checkout>

The reference's ``SPELoss.compute_loss`` (src/solver/loss.py) is imported read-only and applied as the training loop
applies it (src/tools/training.py:120-127: ``F.softmax`` of the head outputs, then the loss). The head itself is built here
as two ``nn.Linear`` layers -- URSONetHead (src/modeling/head/ursonet.py) is exactly ``Linear(1280, n_ori)`` behind a dropout
and ``Linear(1280, n_pos)``, but its module imports Brevitas, which is absent here. Everything is float64.

Shapes: K = 48, n_ori = 37, n_pos = 27 (classification) or 3 (regression), B = 5. Per case ``c`` in CASES the file holds
  {c}_X [5 x 48], {c}_wo / {c}_bo / {c}_wp / {c}_bp   the inputs and the head at which the loss is taken
  {c}_to [5 x 37] soft labels, {c}_tp [5 x 27] soft labels or [5 x 3] positions
  {c}_loss                                            SPELoss.compute_loss
  {c}_gwo / {c}_gbo / {c}_gwp / {c}_gbp               autograd gradients of it
  {c}_{opt}_w [3 x 64|40 x 48], {c}_{opt}_b, {c}_{opt}_loss [3]   three steps of torch.optim.SGD(lr 0.05, momentum 0.9,
      weight_decay 1e-4) / torch.optim.Adam(lr 0.01, weight_decay 1e-4) on the same batch (opt = sgd | adam): the
      weights (ori rows, then pos rows) and bias after each step, and the loss each step was taken at
No reference source is copied.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

K, N_ORI, B = 48, 37, 5
# name: (pos_mode, n_pos, norm_distance, beta)
CASES = {
    'cc_b1': ('classification', 27, False, 1.0),
    'cc_b05': ('classification', 27, False, 0.5),
    'cr_b1': ('regression', 3, False, 1.0),
    'cr_norm_b05': ('regression', 3, True, 0.5),
}
SGD = dict(lr=0.05, momentum=0.9, weight_decay=1e-4)
ADAM = dict(lr=0.01, weight_decay=1e-4)


def main(ref_root):
    import torch
    from make_golden import _install_stubs
    _install_stubs()
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref_root)
    from src.solver.loss import SPELoss
    torch.set_default_dtype(torch.float64)
    out = {}
    for ci, (name, (pos_mode, n_pos, norm, beta)) in enumerate(CASES.items()):
        rng = np.random.Generator(np.random.PCG64(4100 + ci))
        X = rng.standard_normal((B, K))
        w = {'wo': rng.standard_normal((N_ORI, K)) * 0.2, 'bo': rng.standard_normal(N_ORI) * 0.1,
             'wp': rng.standard_normal((n_pos, K)) * 0.2, 'bp': rng.standard_normal(n_pos) * 0.1}
        to = rng.random((B, N_ORI)) ** 4
        to[:, ::5] = 0.0                                  # exact zeros, as the masked bins of an encoded target
        to /= to.sum(axis=1, keepdims=True)
        if pos_mode == 'classification':
            tp = rng.random((B, n_pos)) ** 4
            tp /= tp.sum(axis=1, keepdims=True)
        else:
            tp = rng.standard_normal((B, 3)) * np.array([2.0, 2.0, 8.0]) + np.array([0.0, 0.0, 12.0])
        crit = SPELoss('classification', pos_mode, beta=beta, norm_distance=norm)

        def build():
            ori, pos = torch.nn.Linear(K, N_ORI), torch.nn.Linear(K, n_pos)
            with torch.no_grad():
                ori.weight.copy_(torch.from_numpy(w['wo']))
                ori.bias.copy_(torch.from_numpy(w['bo']))
                pos.weight.copy_(torch.from_numpy(w['wp']))
                pos.bias.copy_(torch.from_numpy(w['bp']))
            return ori, pos

        def loss_of(ori, pos):
            x = torch.from_numpy(X)
            pose = {'ori_soft': torch.nn.functional.softmax(ori(x), dim=1)}
            target = {'ori_soft': torch.from_numpy(to)}
            if pos_mode == 'classification':
                pose['pos_soft'] = torch.nn.functional.softmax(pos(x), dim=1)
                target['pos_soft'] = torch.from_numpy(tp)
            else:
                pose['pos'] = pos(x)
                target['pos'] = torch.from_numpy(tp)
            return crit.compute_loss(pose, target)

        ori, pos = build()
        loss = loss_of(ori, pos)
        loss.backward()
        out.update({f'{name}_X': X, f'{name}_to': to, f'{name}_tp': tp, f'{name}_loss': np.float64(loss.item()),
                    f'{name}_gwo': ori.weight.grad.numpy().copy(), f'{name}_gbo': ori.bias.grad.numpy().copy(),
                    f'{name}_gwp': pos.weight.grad.numpy().copy(), f'{name}_gbp': pos.bias.grad.numpy().copy()})
        out.update({f'{name}_{k}': v for k, v in w.items()})
        for oname, make in (('sgd', lambda p: torch.optim.SGD(p, **SGD)), ('adam', lambda p: torch.optim.Adam(p, **ADAM))):
            ori, pos = build()
            opt = make(list(ori.parameters()) + list(pos.parameters()))
            ws, bs, ls = [], [], []
            for _ in range(3):
                opt.zero_grad()
                loss = loss_of(ori, pos)
                loss.backward()
                opt.step()
                ls.append(loss.item())
                ws.append(np.concatenate([ori.weight.detach().numpy(), pos.weight.detach().numpy()]))
                bs.append(np.concatenate([ori.bias.detach().numpy(), pos.bias.detach().numpy()]))
            out.update({f'{name}_{oname}_w': np.stack(ws), f'{name}_{oname}_b': np.stack(bs),
                        f'{name}_{oname}_loss': np.array(ls)})
    path = os.path.join(HERE, 'head_fit.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1])
