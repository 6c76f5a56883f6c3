"""3-point consensus kernel: accuracy table and timing (GPU box).

First the table of DESIGN.md section 3 "Consensus path", through the kernels: the fixture poses with 1 px Gaussian
noise and k keypoints per frame moved 40 to 200 px (default_rng(11 + k), as tests/consensus_inputs.planted), orientation
error median / p90 / max of EPnP, EPnP + Huber refinement (4 px, 50 trials) and EPnP + consensus (8 px, 6 inliers) +
refinement, and the rows whose inlier mask is the planted one.

Then HIP-event time per launch at B = 64, 512 and 1,800 problems (k = 3 inputs), next to the EPnP launch it follows
and the refinement launch that follows it: the three are timed in the same process, interleaved (each decode_keypoints
call enqueues EPnP, the consensus, then the refinement), with the engine's profiler. Last: the same at 16 model points
(560 triples, three passes of the 256 threads). SPEF_LIB selects an A/B build (tools/build_variant.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'spacecraft-pose-estimation-framework_amd')]
import numpy as np
import torch

from spef_amd import blob as Bl
from spef_amd.arch import mobilenet_v2
from spef_amd.engine import Engine
from spef_amd.quaternion import angle_deg
from spef_amd.weights import synthetic_state_dict

TAU, MIN_INLIERS, HUBER_PX, MAX_ITERS, REPS = 8.0, 6, 4.0, 50, 50


def planted(g, k, count, seed=None):
    rng = np.random.default_rng(11 + k if seed is None else seed)
    nu, nv = float(g['nu']), float(g['nv'])
    n = g['kp2d'].shape[1] // 2 - 1
    px = g['kp2d'][:count].astype(np.float64).reshape(count, n + 1, 2) * [nu, nv]
    px += rng.normal(0, 1.0, px.shape)
    bad = np.zeros((count, n), bool)
    for i in range(count):
        w = rng.choice(n, k, replace=False)
        bad[i, w] = True
        phi = rng.uniform(0, 2 * np.pi, k)
        r = rng.uniform(40, 200, k)
        px[i, w + 1] += np.stack([r * np.cos(phi), r * np.sin(phi)], -1)
    return (px / [nu, nv]).reshape(count, -1).astype(np.float32), bad


def stats(a):
    return f'{np.median(a):.2f} / {np.percentile(a, 90):.2f} / {a.max():.2f}'


def decode(eng, kp, refine, consensus):
    eng.set_keypoint_refine(*refine) if refine else eng.set_keypoint_refine(None)
    eng.set_keypoint_consensus(*consensus) if consensus else eng.set_keypoint_consensus(None)
    o = eng.decode_keypoints(kp, apply_sigmoid=False)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


arch = mobilenet_v2('keypoints')
eng = Engine(Bl.pack(synthetic_state_dict(arch, seed=1001, head_std=0.002), arch, dtype='fp32'), 'cuda:0')
print('| fixture (rows) | k | EPnP | EPnP + Huber | consensus + refine | masks exact | bit 64 |')
for name, count in (('keypoints.npz', 96), ('keypoints_speedplus.npz', 64)):
    g = np.load(os.path.join(ROOT, 'tests', 'golden', name))
    eng.set_keypoints(g['kp3d'], g['K'], float(g['nu']), float(g['nv']), g['dist'] if 'dist' in g.files else None)
    for k in (1, 2, 3, 4, 5):
        kp_np, bad = planted(g, k, count)
        kp = torch.from_numpy(kp_np).cuda()
        plain = decode(eng, kp, None, None)
        huber = decode(eng, kp, (MAX_ITERS, HUBER_PX), None)
        cons = decode(eng, kp, (MAX_ITERS, HUBER_PX), (TAU, MIN_INLIERS))
        q = g['q'][:count]
        print(f'| {name} ({count}) | {k} | {stats(angle_deg(plain["ori"], q))} | {stats(angle_deg(huber["ori"], q))} | '
              f'{stats(angle_deg(cons["ori"], q))} | {int(np.all(cons["inliers"] == ~bad, axis=1).sum())} / {count} | '
              f'{int(((cons["status"] & 64) != 0).sum())} |', flush=True)
g = np.load(os.path.join(ROOT, 'tests', 'golden', 'keypoints.npz'))
eng.set_keypoints(g['kp3d'], g['K'], float(g['nu']), float(g['nv']))
for k, count, seed, fewest in ((6, 32, None, 5), (8, 32, 19, MIN_INLIERS)):   # six moved: five of eleven are left
    kp_np, bad = planted(g, k, count, seed)
    cons = decode(eng, torch.from_numpy(kp_np).cuda(), (MAX_ITERS, HUBER_PX), (TAU, fewest))
    print(f'k = {k}, at least {fewest} inliers: masks exact {int(np.all(cons["inliers"] == ~bad, axis=1).sum())} / '
          f'{count}, bit 64 on {int(((cons["status"] & 64) != 0).sum())} rows')


def timing(eng, kp, label):
    eng.set_keypoint_refine(MAX_ITERS, HUBER_PX)
    eng.set_keypoint_consensus(TAU, None)
    for _ in range(5):
        o = eng.decode_keypoints(kp, apply_sigmoid=False)
    torch.cuda.synchronize()
    eng.profile_begin()
    for _ in range(REPS):
        eng.decode_keypoints(kp, apply_sigmoid=False)
    prof = eng.profile_end()
    us = {k: prof[k][1] / prof[k][0] * 1e3 for k in ('epnp_kernel', 'consensus_kernel', 'refine_kernel')}
    it = o['refine_iters'].cpu().numpy()
    print(f'{label}: epnp {us["epnp_kernel"]:.1f} us, consensus {us["consensus_kernel"]:.1f} us, refine '
          f'{us["refine_kernel"]:.1f} us per launch; bit 64 on {int(((o["status"] & 64) != 0).sum().item())} rows; '
          f'refinement trials median {np.median(it):.0f} max {it.max()}', flush=True)


for P in (64, 512, 1800):
    timing(eng, torch.from_numpy(planted(g, 3, P)[0]).cuda(), f'P={P} n=11 (165 triples, 192 threads)')

# 16 points: the 11 Tango points and 5 seeded ones, projected with the fixture's poses, 1 px noise
from spef_amd.spe.keypoints import KeyPoints  # noqa: E402

pts = np.concatenate([g['kp3d'], np.random.default_rng(16).uniform(-0.5, 0.5, (5, 3)).astype(np.float32)])


class Cam:
    K, nu, nv = g['K'], float(g['nu']), float(g['nv'])


kps = KeyPoints(Cam, pts)
rng = np.random.default_rng(16)
eng.set_keypoints(pts, Cam.K, Cam.nu, Cam.nv)
for P in (64, 512):
    kp = np.stack([kps.create_keypoints2d(g['q'][i], g['t'][i]) for i in range(P)])
    kp = (kp + rng.normal(0, 1.0, kp.shape) / np.tile([Cam.nu, Cam.nv], 17)).astype(np.float32)
    timing(eng, torch.from_numpy(kp).cuda(), f'P={P} n=16 (560 triples, 256 threads x 3)')
eng.close()
