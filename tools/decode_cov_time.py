"""Covariance-path timing (GPU box): HIP-event microseconds per call of spef_decode alone and of spef_decode +
spef_decode_cov, interleaved in one process, at B = 64 and B = 1 with 1728 orientation / 1000 position bins (median of
50 each after warm-up), and the per-kernel split of the engine's HIP-event profiler next to it; then the covariance
kernel alone at 256, 1728 and 8192 orientation bins (1, 7 and 32 bins per thread: what a bin costs). Last: the whole
predict_tracked step at B = 64 (T = 1, S = 64; forward + decode + tracker, fp16mx blob, 512 x 512 frames) with pdf_cov
off and on, interleaved. The logits are the planted T = 0.2 rows of tests/golden/decode_ori.npz and encoded SPEED
positions. SPEF_LIB selects an A/B build (tools/build_variant.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'spacecraft-pose-estimation-framework_amd')]
import numpy as np
import torch

from spef_amd import _lib as L
from spef_amd import blob as Bl
from spef_amd.arch import mobilenet_v2
from spef_amd.data.synthetic import synth_frames
from spef_amd.engine import Engine
from spef_amd.spe.spe_utils import SPEUtils
from spef_amd.spe_mi355x import SPEMi355x
from spef_amd.weights import synthetic_state_dict

REPS = 50
CLS = L.CLASSIFICATION

go = np.load(os.path.join(ROOT, 'tests', 'golden', 'decode_ori.npz'))
gp = np.load(os.path.join(ROOT, 'tests', 'golden', 'decode_pos.npz'))
eng = Engine(None, 'cuda:0')
eng.set_decode_tables(go['hist'], gp['grid'])
with np.errstate(divide='ignore'):
    pos_logits = np.maximum(np.log(gp['enc']), -80.0).astype(np.float32)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


for B in (64, 1):
    rows = np.arange(B) % 32
    lo = torch.from_numpy(np.ascontiguousarray(go['planted_logits'][2, rows])).cuda()
    lp = torch.from_numpy(np.ascontiguousarray(pos_logits[rows])).cuda()
    us = {False: [], True: []}
    for rep in range(REPS + 5):
        for on in (False, True):
            t = timed(lambda: eng.decode(CLS, CLS, lo, lp, want_cov=on))
            if rep >= 5:
                us[on].append(t)
    eng.profile_begin()
    for _ in range(REPS):
        dec = eng.decode(CLS, CLS, lo, lp, want_cov=True, want_hinv=True)
    prof = eng.profile_end()
    per = {k: prof[k][1] / prof[k][0] * 1e3 for k in ('decode_ori_kernel', 'decode_cov_kernel')}
    sig = np.degrees(np.sqrt(np.trace(dec['cov'][0, :3, :3].cpu().numpy())))
    print(f'B={B}: spef_decode {np.median(us[False]):.1f} us per call, spef_decode + spef_decode_cov '
          f'{np.median(us[True]):.1f} us (median of {REPS}, HIP events around the call, output allocation included); '
          f'profiler: decode_ori_kernel {per["decode_ori_kernel"]:.1f} us, decode_cov_kernel '
          f'{per["decode_cov_kernel"]:.1f} us per launch; cov_status {sorted(set(dec["cov_status"].cpu().numpy().tolist()))}, '
          f'row 0 sigma {sig:.1f} deg', flush=True)
eng.close()

# where the kernel's time goes: its launches at B = 64 against the bins one thread walks (1, 7 and 32 of them)
for n in (256, 1728, 8192):
    rng = np.random.Generator(np.random.PCG64(n))
    h = rng.standard_normal((n, 4))
    h /= np.linalg.norm(h, axis=1, keepdims=True)
    e = Engine(None, 'cuda:0')
    e.set_decode_tables(h, gp['grid'])
    lo = torch.from_numpy((30.0 * (h[:64] @ h.T) ** 2).astype(np.float32)).cuda()
    lp = torch.from_numpy(np.ascontiguousarray(pos_logits[np.arange(64) % 32])).cuda()
    dec = e.decode(CLS, CLS, lo, lp)
    for _ in range(5):
        e.decode_cov(dec, CLS, CLS, want_hinv=True)
    e.profile_begin()
    for _ in range(REPS):
        e.decode_cov(dec, CLS, CLS, want_hinv=True)
    k = e.profile_end()['decode_cov_kernel']
    print(f'decode_cov_kernel B=64, {n} orientation bins ({(n + 255) // 256} per thread): {k[1] / k[0] * 1e3:.1f} us '
          f'per launch', flush=True)
    e.close()

# the whole B = 64 predict_tracked step, pdf_cov off / on, interleaved
su = SPEUtils(None, 'classification', 12, 3, False, 'classification')
sd = synthetic_state_dict(mobilenet_v2('ursonet', su.orientation.n_bins, su.position.n_bins), seed=1001)
spe = SPEMi355x(Bl.pack(sd, dtype='fp16mx'), 'cuda:0', su)
frames = torch.from_numpy(synth_frames(64, 512, 512, 20_000)).cuda()
ms = {False: [], True: []}
for rep in range(12):
    for on in (False, True):
        _, tracked, lat = spe.predict_tracked(frames, n_streams=64, pdf_cov=on, gate_chi2=16.81)
        if rep >= 2:
            ms[on].append(lat)
print(f'B=64 predict_tracked step (forward + decode + tracker, fp16mx, 512 x 512, one stream): pdf_cov off '
      f'{np.median(ms[False]) * 1e3:.0f} us, on {np.median(ms[True]) * 1e3:.0f} us (median of {len(ms[True])}); track '
      f'status {sorted(set(tracked["track_status"].tolist()))}')
spe.close()
