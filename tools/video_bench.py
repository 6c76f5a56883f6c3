#!/usr/bin/env python3
"""Timing of the video path ("Video path"): 64 frames of 512 x 512, fp16mx, synthetic weights.

    python tools/video_bench.py [--frames 64] [--size 512] [--dtype fp16mx] [--reps 7]

runs four measurements, each in a fresh child process under its own time limit, and prints one JSON line per
measurement:

    loop      64 calls of Inference.predict(x, 'Adaptative'): the per-frame path (B = 1 forward, host NumPy filter,
              a second decode on log(pdf)) -- the baseline; this code path is the same before and after the video
              kernels were added
    sequence  Inference.predict_sequence(x[64]): T = 64, S = 1 -- one forward, one decode, one video step
    cameras   SPEMi355x.predict_video(x[64], n_streams=64): T = 1, S = 64
    scan      the video kernels alone, from the library's per-launch HIP-event profile (spef_profile_*): time per
              launch, and per time step for T = 64, S = 1

Times are host wall-clock around calls that end in a device synchronise (median of --reps after 2 warm-up runs);
frames are resident on the device.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'spacecraft-pose-estimation-framework_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

MODES = ('loop', 'sequence', 'cameras', 'scan')
LIMIT_S = {'loop': 240, 'sequence': 180, 'cameras': 180, 'scan': 180}


def _setup(args):
    import numpy as np
    import torch
    from spef_amd import blob as Bl
    from spef_amd.arch import mobilenet_v2
    from spef_amd.spe.spe_utils import SPEUtils
    from spef_amd.weights import synthetic_state_dict
    su = SPEUtils(None, 'classification', 12, 3, False, 'classification')
    sd = synthetic_state_dict(mobilenet_v2('ursonet', su.orientation.n_bins, su.position.n_bins), seed=1001,
                              head_std=0.3)
    blob = Bl.pack(sd, dtype=args.dtype)
    rng = np.random.Generator(np.random.PCG64(5))
    x = torch.from_numpy(rng.random((args.frames, 3, args.size, args.size), dtype=np.float32)).cuda()
    return su, blob, x


def _timed(fn, reps):
    import torch
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def run_mode(args):
    import torch
    from spef_amd.inference import Inference
    su, blob, x = _setup(args)
    n = args.frames
    rec = {'mode': args.mode, 'frames': n, 'size': args.size, 'dtype': args.dtype, 'reps': args.reps,
           'gpu': torch.cuda.get_device_name(0)}
    inf = Inference(blob, 'gpu_mi355x', su)
    if args.mode == 'loop':
        def fn():
            inf.reset()
            for t in range(n):
                inf.predict(x[t:t + 1], 'Adaptative')
    elif args.mode == 'sequence':
        def fn():
            inf.reset()
            inf.predict_sequence(x)
    elif args.mode == 'cameras':
        spe = inf.inference_engine

        def fn():
            spe.video_filter(n).reset()
            spe.predict_video(x, n_streams=n)
    else:
        spe = inf.inference_engine
        eng = spe.engine
        for label, streams in (('T64_S1', 1), ('T1_S64', n)):
            spe.video_filter(streams).reset()
            spe.predict_video(x, n_streams=streams)               # warm
            eng.profile_begin()
            for _ in range(args.reps):
                spe.video_filter(streams).reset()
                spe.predict_video(x, n_streams=streams)
            prof = eng.profile_end()
            for key in ('video_scan_kernel', 'decode_pdf_kernels', 'video_pole_kernel', 'decode_ori_kernel'):
                launches, ms = prof[key][0], prof[key][1]
                rec[f'{label}_{key}_us_per_launch'] = round(1e3 * ms / launches, 2)
            rec[f'{label}_scan_us_per_time_step'] = round(
                1e3 * prof['video_scan_kernel'][1] / prof['video_scan_kernel'][0] / (n // streams), 3)
            rec[f'{label}_all_kernels_ms'] = round(sum(v[1] for v in prof.values()) / args.reps, 3)
        inf.close()
        print(json.dumps(rec), flush=True)
        return
    med, lo, hi = _timed(fn, args.reps)
    rec.update(ms_per_64=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
               frames_per_s=round(n / med * 1e3, 1))
    inf.close()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--mode', choices=MODES, help='run one measurement in this process (default: all, one child each)')
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--dtype', default='fp16mx')
    ap.add_argument('--reps', type=int, default=7)
    args = ap.parse_args()
    if args.mode:
        return run_mode(args)
    for mode in MODES:       # a fresh process per measurement; stop at the first that fails or runs out of time
        cmd = [sys.executable, os.path.abspath(__file__), '--mode', mode, '--frames', str(args.frames), '--size',
               str(args.size), '--dtype', args.dtype, '--reps', str(args.reps)]
        try:
            r = subprocess.run(cmd, timeout=LIMIT_S[mode])
        except subprocess.TimeoutExpired:
            print(f'video_bench: {mode} ran out of time ({LIMIT_S[mode]} s); stopping', file=sys.stderr)
            return 124
        if r.returncode != 0:
            print(f'video_bench: {mode} failed with status {r.returncode}; stopping', file=sys.stderr)
            return r.returncode
    return 0


if __name__ == '__main__':
    sys.exit(main())
