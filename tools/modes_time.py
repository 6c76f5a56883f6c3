"""Modes-path timing (GPU box): microseconds per B = 64 launch of decode_modes_kernel (1728 orientation bins; k_max 1, 2
and 4, rounds 0 and 3) on two-peaked PDFs, next to decode_cov_kernel on the same rows, and of the tracker step with one
measurement (track_step_kernel) and with K = 2 and 4 candidates (track_step_modes_kernel) at (T, S) = (1, 64). Every
figure comes twice: the median of 50 launches timed one by one with HIP events around the C entry point (outputs
allocated beforehand; warm-up first), and the mean per launch of the engine's HIP-event profiler over the same 50.
SPEF_LIB selects an A/B build (tools/build_variant.py)."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'spacecraft-pose-estimation-framework_amd'), os.path.join(ROOT, 'tests')]
import numpy as np
import torch

import modes_inputs as MI
from spef_amd import _lib as L
from spef_amd.engine import Engine, _ptr, _stream

REPS, WARM, B = 50, 10, 64
CLS, REG = L.CLASSIFICATION, L.REGRESSION


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def measure(eng, kernel, fn):
    """-> (median us of REPS single launches, profiler's mean us per launch)."""
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    us = [timed(fn) for _ in range(REPS)]
    eng.profile_begin()
    for _ in range(REPS):
        fn()
    k = eng.profile_end()[kernel]
    return float(np.median(us)), k[1] / k[0] * 1e3


tab = MI.tables()[1728]
eng = Engine(None, 'cuda:0')
eng.set_decode_tables(tab[0], None)
st = _stream(eng.device)
rng = np.random.Generator(np.random.PCG64(64))
pdf_host = np.stack([MI.mixture_pdf(q, MI.qmul(q, MI.FLIP_Z), rng.uniform(0.3, 0.7), tab)
                     for q in (MI.rand_quat(rng) for _ in range(B))])
pdf = torch.from_numpy(pdf_host).cuda()
dec = eng.decode(CLS, REG, torch.log(pdf + 1e-30), torch.zeros((B, 3), device='cuda'), want_cov=True)
med, prof = measure(eng, 'decode_cov_kernel', lambda: eng.decode_cov(dec, CLS, REG))
print(f'decode_cov_kernel B={B}, 1728 bins: median {med:.1f} us per call (output allocation included), profiler '
      f'{prof:.1f} us per launch', flush=True)
for k_max in (1, 2, 4):
    for rounds in (0, 3):
        prm = L.ModesParams(k_max, rounds, 45.0, 0.1, 0.05, 0.0)
        mq = torch.empty((B, k_max, 4), device='cuda')
        mm = torch.empty((B, k_max), device='cuda')
        mc = torch.empty((B, k_max, 9), device='cuda')
        nm, ms = (torch.empty((B,), dtype=torch.int32, device='cuda') for _ in range(2))

        def run():
            L.check(eng.lib.spef_decode_modes(eng.ctx, _ptr(pdf), 1728, B, C.byref(prm), _ptr(mq), _ptr(mm), _ptr(mc),
                                              _ptr(nm), _ptr(ms), st))
        med, prof = measure(eng, 'decode_modes_kernel', run)
        print(f'decode_modes_kernel B={B}, 1728 bins, k_max={k_max}, rounds={rounds}: median {med:.1f} us, profiler '
              f'{prof:.1f} us per launch; modes found {np.bincount(nm.cpu().numpy(), minlength=5)[1:].tolist()}',
              flush=True)

# the tracker step at (T, S) = (1, 64): one measurement against K candidates
trk_p = dict(MI.TRACK)
for K in (0, 2, 4):
    md = eng.decode_modes(dec, k_max=max(K, 1))
    trk = eng.tracker(B, **trk_p)
    row = dict(dec)
    (trk.step_modes if K else trk.step)(row, 1)           # the first frame starts the tracks: time the steps after it
    fn = (lambda: trk.step_modes(row, 1)) if K else (lambda: trk.step(row, 1))
    name = 'track_step_modes_kernel' if K else 'track_step_kernel'
    med, prof = measure(eng, name, fn)
    print(f'{name} (T, S) = (1, {B})' + (f', K={K}' if K else '') + f': median {med:.1f} us per call (output allocation '
          f'included), profiler {prof:.1f} us per launch', flush=True)
    trk.close()
eng.close()
