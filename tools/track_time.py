"""Pose-tracker kernel timing (GPU box): HIP-event microseconds per launch of spef_track_step for (T, S) = (1, 64),
(8, 8) and (64, 1), each with and without cov / cov_out, 50 launches after warm-up, with the engine's HIP-event
profiler; next to it, in the same process, the EPnP launch at B = 64 that a (1, 64) step follows. Last: the whole
B = 64 keypoint step (forward + decode with the refinement, fp16x2 blob, 240 x 384 frames) with the tracker off and on
(T = 1, S = 64), interleaved. The measurements are the constant-rate trajectory of tests/track_inputs.py with its noise
(every stream a copy). SPEF_LIB selects an A/B build (tools/build_variant.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'spacecraft-pose-estimation-framework_amd'), os.path.join(ROOT, 'tests')]
import numpy as np
import torch

import track_inputs as TI
from spef_amd import blob as Bl
from spef_amd.arch import mobilenet_v2
from spef_amd.data.synthetic import synth_frames
from spef_amd.engine import Engine
from spef_amd.weights import plant_keypoint_head, synthetic_state_dict

REPS = 50

g = np.load(os.path.join(ROOT, 'tests', 'golden', 'keypoints.npz'))
arch = mobilenet_v2('keypoints')
i = int(np.argmin(np.abs(g['t'][:, 2] - np.median(g['t'][:, 2]))))
sd = plant_keypoint_head(synthetic_state_dict(arch, seed=1001, head_std=2e-4), g['kp2d'][i])
eng = Engine(Bl.pack(sd, arch, dtype='fp16x2'), 'cuda:0')
eng.set_keypoints(g['kp3d'], g['K'], float(g['nu']), float(g['nv']))

kp = torch.from_numpy(np.ascontiguousarray(g['kp2d'][:64], np.float32)).cuda()
for _ in range(5):
    eng.decode_keypoints(kp, apply_sigmoid=False)
eng.profile_begin()
for _ in range(REPS):
    eng.decode_keypoints(kp, apply_sigmoid=False)
prof = eng.profile_end()
print(f'epnp_kernel B=64: {prof["epnp_kernel"][1] / prof["epnp_kernel"][0] * 1e3:.1f} us per launch', flush=True)

qm, tm, cov, st = TI.standard()
for T, S in ((1, 64), (8, 8), (64, 1)):
    rows = np.repeat(np.arange(T), S)
    dec = {'ori': torch.from_numpy(qm[rows].astype(np.float32)).cuda(),
           'pos': torch.from_numpy(tm[rows].astype(np.float32)).cuda(),
           'status': torch.from_numpy(st[rows].astype(np.int32)).cuda()}
    for with_cov in (False, True):
        d = dict(dec, cov=torch.from_numpy(cov[rows].astype(np.float32)).cuda()) if with_cov else dec
        trk = eng.tracker(S, **(TI.PARAMS if with_cov else dict(TI.PARAMS, r=(1e-4, 1e-2))))
        for _ in range(5):
            trk.step(d, T, want_cov=with_cov)
        eng.profile_begin()
        for _ in range(REPS):
            out = trk.step(d, T, want_cov=with_cov)
        prof = eng.profile_end()
        n, ms = prof['track_step_kernel'][:2]
        flags = sorted(set(out['track_status'].cpu().numpy().tolist()))
        print(f'track_step_kernel T={T} S={S} cov/cov_out {"on" if with_cov else "off"}: {ms / n * 1e3:.1f} us per launch, '
              f'{ms / n * 1e3 / T:.2f} us per frame of the serial chain; track status {flags}', flush=True)
        trk.close()

# the whole B = 64 keypoint step with the refinement, tracker off / on, interleaved
eng.set_keypoint_refine(50, 4.0)
frames = torch.from_numpy(synth_frames(64, 240, 384, 20_000)).cuda()
eng.reserve(64, 240, 384)
trk = eng.tracker(64, gate_chi2=TI.GATE, max_coast=3)
ms = {False: [], True: []}
for rep in range(12):
    for on in (False, True):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        raw, _ = eng.forward(frames)
        dec = eng.decode_keypoints(raw, want_cov=on)
        if on:
            out = trk.step(dec, 1)
        b.record()
        b.synchronize()
        if rep >= 2:
            ms[on].append(a.elapsed_time(b))
print(f'B=64 keypoint step (forward + decode + refinement, fp16x2, one stream): tracker off '
      f'{np.median(ms[False]) * 1e3:.0f} us, on {np.median(ms[True]) * 1e3:.0f} us (median of {len(ms[True])}); track '
      f'status {sorted(set(out["track_status"].cpu().numpy().tolist()))}')
trk.close()
eng.close()
