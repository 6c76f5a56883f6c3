"""Pose-smoother kernel timing (GPU box): HIP-event microseconds per launch, 50 launches after warm-up, with the engine's
HIP-event profiler, at (T, S) = (64, 1), (8, 8) and (64, 64): the gain kernel and the chain kernel of spef_track_smooth
apart, each with and without cov_out, and next to them, in the same process, spef_track_step and spef_track_step_hist
on the same rows -- three repeats of each, so that the spread between repeats (the run-to-run noise) stands beside the
difference between the two. The measurements are the constant-rate trajectory of tests/track_inputs.py with its noise
and covariance (every stream a copy). SPEF_LIB selects an A/B build (tools/build_variant.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'spacecraft-pose-estimation-framework_amd'), os.path.join(ROOT, 'tests')]
import numpy as np
import torch

import track_inputs as TI
from spef_amd.engine import Engine

REPS, REPEATS = 50, 3

eng = Engine(None, 'cuda:0')
qm, tm, cov, st = TI.standard()


def timed(label, fn):
    """-> {kernel: us per launch} over REPS calls of fn after 5 warm-up calls."""
    for _ in range(5):
        fn()
    eng.profile_begin()
    for _ in range(REPS):
        fn()
    prof = eng.profile_end()
    return {k: v[1] / v[0] * 1e3 for k, v in prof.items()}


for T, S in ((64, 1), (8, 8), (64, 64)):
    rows = np.repeat(np.arange(T), S)
    dec = {'ori': torch.from_numpy(qm[rows].astype(np.float32)).cuda(),
           'pos': torch.from_numpy(tm[rows].astype(np.float32)).cuda(),
           'status': torch.from_numpy(st[rows].astype(np.int32)).cuda(),
           'cov': torch.from_numpy(cov[rows].astype(np.float32)).cuda()}
    trk = eng.tracker(S, **TI.PARAMS)
    hist = trk.history(T)

    def plain():
        trk.reset()
        return trk.step(dec, T)

    def recorded():
        trk.reset()
        hist.reset()
        return trk.step(dec, T, history=hist)

    step, step_hist = [], []
    for _ in range(REPEATS):
        step.append(timed('step', plain)['track_step_kernel'])
        step_hist.append(timed('step_hist', recorded)['track_step_hist_kernel'])
    out = recorded()
    line = f'T={T} S={S}: track_step_kernel ' + ' / '.join(f'{x:.1f}' for x in step) + ' us, track_step_hist_kernel ' + \
        ' / '.join(f'{x:.1f}' for x in step_hist) + f' us per launch ({REPEATS} repeats of {REPS}); filter chain ' \
        f'{np.median(step) / T:.2f} us per frame'
    print(line, flush=True)
    for want_cov in (False, True):
        t = timed('smooth', lambda: hist.smooth(out, want_cov=want_cov))
        res = hist.smooth(out, want_cov=want_cov)
        flags = sorted(set(res['smooth_status'].cpu().numpy().tolist()))
        print(f'T={T} S={S} cov_out {"on" if want_cov else "off"}: smooth_gain_kernel {t["smooth_gain_kernel"]:.1f} us, '
              f'smooth_chain_kernel {t["smooth_chain_kernel"]:.1f} us per launch, '
              f'{t["smooth_chain_kernel"] / T:.2f} us per frame of the serial chain; smooth status {flags}', flush=True)
    hist.close()
    trk.close()
eng.close()
