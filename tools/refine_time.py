"""Pose-refinement kernel timing (GPU box), next to the EPnP launch it follows: B = 64, 512 and 1,800 problems per
launch on the noise-free fixture (tests/golden/keypoints.npz) and on noisy one-outlier inputs (1 px Gaussian noise, one
keypoint per frame moved 60 px; default_rng(7) as tests/refine_inputs.one_outlier), Huber 4 px, 50 trials. Both launches
are timed in the same process, interleaved (each decode_keypoints call enqueues EPnP, then the refinement), with the
engine's HIP-event profiler. Last: the whole B = 64 keypoint step (forward + decode, fp16x2 blob, 240 x 384 frames)
with the refinement off and on. SPEF_LIB selects an A/B build (tools/build_variant.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'spacecraft-pose-estimation-framework_amd')]
import numpy as np
import torch

from spef_amd import blob as Bl
from spef_amd.arch import mobilenet_v2
from spef_amd.data.synthetic import synth_frames
from spef_amd.engine import Engine
from spef_amd.quaternion import angle_deg
from spef_amd.weights import plant_keypoint_head, synthetic_state_dict

HUBER_PX, MAX_ITERS, REPS = 4.0, 50, 50


def one_outlier(g, count):
    rng = np.random.default_rng(7)
    nu, nv = float(g['nu']), float(g['nv'])
    n = g['kp2d'].shape[1] // 2 - 1
    px = g['kp2d'][:count].astype(np.float64).reshape(count, n + 1, 2) * [nu, nv]
    px += rng.normal(0, 1.0, px.shape)
    which = rng.integers(0, n, count)
    phi = rng.uniform(0, 2 * np.pi, count)
    px[np.arange(count), which + 1] += 60.0 * np.stack([np.cos(phi), np.sin(phi)], -1)
    return (px / [nu, nv]).reshape(count, -1).astype(np.float32)


g = np.load(os.path.join(ROOT, 'tests', 'golden', 'keypoints.npz'))
arch = mobilenet_v2('keypoints')
i = int(np.argmin(np.abs(g['t'][:, 2] - np.median(g['t'][:, 2]))))
sd = plant_keypoint_head(synthetic_state_dict(arch, seed=1001, head_std=2e-4), g['kp2d'][i])
eng = Engine(Bl.pack(sd, arch, dtype='fp16x2'), 'cuda:0')
eng.set_keypoints(g['kp3d'], g['K'], float(g['nu']), float(g['nv']))
eng.set_keypoint_refine(MAX_ITERS, HUBER_PX)
for P in (64, 512, 1800):
    for label, kp_np in (('noise-free', np.ascontiguousarray(g['kp2d'][:P], np.float32)), ('one outlier', one_outlier(g, P))):
        kp = torch.from_numpy(kp_np).cuda()
        o = eng.decode_keypoints(kp, apply_sigmoid=False)
        torch.cuda.synchronize()
        it = o['refine_iters'].cpu().numpy()
        st = o['status'].cpu().numpy()
        a0 = np.median(angle_deg(o['ori_epnp'].cpu().numpy(), g['q'][:P]))
        a1 = np.median(angle_deg(o['ori'].cpu().numpy(), g['q'][:P]))
        for _ in range(5):
            eng.decode_keypoints(kp, apply_sigmoid=False)
        eng.profile_begin()
        for _ in range(REPS):
            eng.decode_keypoints(kp, apply_sigmoid=False)
        prof = eng.profile_end()
        us = {k: prof[k][1] / prof[k][0] * 1e3 for k in ('epnp_kernel', 'refine_kernel')}
        print(f'P={P} {label}: epnp {us["epnp_kernel"]:.1f} us, refine {us["refine_kernel"]:.1f} us per launch; trials '
              f'median {np.median(it):.0f} max {it.max()}; status bits {sorted(set(st.tolist()))}; orientation median '
              f'{a0:.3g} -> {a1:.3g} deg', flush=True)

# the whole B = 64 keypoint step, refinement off / on, interleaved
frames = torch.from_numpy(synth_frames(64, 240, 384, 20_000)).cuda()
eng.reserve(64, 240, 384)
ms = {False: [], True: []}
for rep in range(12):
    for on in (False, True):
        eng.set_keypoint_refine(MAX_ITERS if on else None, HUBER_PX)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        raw, _ = eng.forward(frames)
        dec = eng.decode_keypoints(raw)
        b.record()
        b.synchronize()
        if rep >= 2:
            ms[on].append(a.elapsed_time(b))
it = dec['refine_iters'].cpu().numpy()
print(f'B=64 keypoint step (forward + decode, fp16x2, one stream): refine off {np.median(ms[False]) * 1e3:.0f} us, on '
      f'{np.median(ms[True]) * 1e3:.0f} us (median of {len(ms[True])}); trials median {np.median(it):.0f} max {it.max()}')
eng.close()
