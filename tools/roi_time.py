"""ROI crop-and-resize kernels: time per launch (GPU box).

HIP-event time per launch (the engine's profiler) of spef_preprocess_roi's two kernels -- the per-frame coefficient
tables and the fused two-pass resample -- at S = 64 frames 1200 x 1920 -> 240 x 384, for full-frame boxes and for
quarter-area boxes (600 x 960, scattered over the frame), next to spef_preprocess' two kernels on the same frames, all
in one process, interleaved. Also the small kernels of the loop (prediction, boxes, un-mapping) at S = 64.
DESIGN.md section 3 "ROI path" records the output. SPEF_LIB selects an A/B build (tools/build_variant.py)."""
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
from spef_amd.weights import synthetic_state_dict

S, HIN, WIN, H, W, REPS, ROUNDS = 64, 1200, 1920, 240, 384, 20, 3

arch = mobilenet_v2('keypoints')
eng = Engine(Bl.pack(synthetic_state_dict(arch, seed=1001, head_std=0.002), arch, dtype='fp32'), 'cuda:0')
g = np.load(os.path.join(ROOT, 'tests', 'golden', 'keypoints.npz'))
eng.set_keypoints(g['kp3d'], g['K'], float(g['nu']), float(g['nv']))
base = synth_frames(8, HIN, WIN, 50_000)
frames = torch.from_numpy(np.concatenate([base] * (S // 8))).cuda()
rng = np.random.default_rng(64)
full = torch.tensor([[0, 0, WIN, HIN]] * S, dtype=torch.int32, device='cuda')
x0, y0 = rng.integers(0, WIN - 960 + 1, S), rng.integers(0, HIN - 600 + 1, S)
quarter = torch.from_numpy(np.stack([x0, y0, x0 + 960, y0 + 600], 1).astype(np.int32)).cuda()
out = torch.empty((S, H, W, 3), dtype=torch.uint8, device='cuda')


def us(prof, *keys):
    return sum(prof[k][1] / prof[k][0] * 1e3 for k in keys)


for _ in range(3):
    eng.preprocess(frames, (H, W), out=out)
    eng.preprocess_roi(frames, full, (H, W), out=out)
    eng.preprocess_roi(frames, quarter, (H, W), out=out)
torch.cuda.synchronize()
assert torch.equal(eng.preprocess_roi(frames, full, (H, W)), eng.preprocess(frames, (H, W)))
print(f'S = {S}, {HIN} x {WIN} -> {H} x {W}, {REPS} launches per round, us per launch')
print('| round | resize_h + resize_v (spef_preprocess) | roi_coeffs | roi_resample, full-frame boxes | roi_coeffs | '
      'roi_resample, quarter-area boxes |')
for rnd in range(ROUNDS):
    row = []
    for box in (None, full, quarter):
        eng.profile_begin()
        for _ in range(REPS):
            if box is None:
                eng.preprocess(frames, (H, W), out=out)
            else:
                eng.preprocess_roi(frames, box, (H, W), out=out)
        prof = eng.profile_end()
        if box is None:
            row.append(f'{us(prof, "resize_h_kernel"):.1f} + {us(prof, "resize_v_kernel"):.1f} = '
                       f'{us(prof, "resize_h_kernel", "resize_v_kernel"):.1f}')
        else:
            row += [f'{us(prof, "roi_coeffs_kernel"):.1f}', f'{us(prof, "roi_resample_kernel"):.1f}']
    print(f'| {rnd} | ' + ' | '.join(row) + ' |', flush=True)

# the small kernels of the loop
trk = eng.tracker(S)
st = np.zeros((S, 160))
st[:, 0] = 1.0
st[:, 3:7] = g['q'][:S]
st[:, 7:10] = g['t'][:S]
st[:, 10:13] = 0.01
trk.set_state(st)
raw = torch.zeros((S, 24), device='cuda')
for rnd in range(2):
    eng.profile_begin()
    for _ in range(REPS):
        p = trk.predict()
        box, _ = eng.roi_boxes(p['ori'], p['pos'], (HIN, WIN), (H, W), have=p['have'])
        eng.unmap_keypoints(raw, box)
    prof = eng.profile_end()
    print(f'round {rnd}: track_predict {us(prof, "track_predict_kernel"):.1f} us, roi_box '
          f'{us(prof, "roi_box_kernel"):.1f} us, roi_unmap {us(prof, "roi_unmap_kernel"):.1f} us per launch', flush=True)
trk.close()
eng.close()
