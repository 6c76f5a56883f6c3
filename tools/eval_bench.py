#!/usr/bin/env python3
"""Timing of an evaluation run ("Scoring path"): 1,800 frames of 512 x 512 (the size of the SPEED
validation split), fp16mx, synthetic weights, batches resident on the device.

    python tools/eval_bench.py [--frames 1800] [--batch 32] [--size 512] [--dtype fp16mx] [--reps 7]

runs three measurements, each in a fresh child process under its own time limit, and prints one JSON line per
measurement:

    host      evaluation(): per batch SPEMi355x.predict (synchronises, copies the pose and the soft outputs to the
              host), SPEUtils.get_score and the error lists in NumPy -- the baseline; this code path is the same
              before and after the scoring kernels were added
    device    evaluation_device(): a depth-3 StreamPipeline, a scoring step per batch on its stream, one result()
    kernels   the scoring kernels alone, from the library's per-launch HIP-event profile (spef_profile_*): time per
              launch of the step (scoring + count advance) and of the statistics kernel

Times are host wall-clock around calls that end in a device synchronise (median of --reps after 2 warm-up runs).
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

MODES = ('host', 'device', 'kernels')
LIMIT_S = {'host': 300, 'device': 240, 'kernels': 240}


def _setup(args):
    import torch
    from spef_amd import blob as Bl
    from spef_amd.arch import mobilenet_v2
    from spef_amd.data.synthetic import synth_frames, synth_poses
    from spef_amd.spe.spe_utils import SPEUtils
    from spef_amd.spe_mi355x import SPEMi355x
    from spef_amd.weights import synthetic_state_dict
    su = SPEUtils(None, 'classification', 12, 3, False, 'classification')
    sd = synthetic_state_dict(mobilenet_v2('ursonet', su.orientation.n_bins, su.position.n_bins), seed=1001,
                              head_std=0.3)
    spe = SPEMi355x(Bl.pack(sd, dtype=args.dtype), 'cuda:0', su)
    # four distinct resident batches, cycled; every image has its own target pose
    pool = [torch.from_numpy(synth_frames(args.batch, args.size, args.size, k * args.batch)).cuda() for k in range(4)]
    batches = []
    for k, a in enumerate(range(0, args.frames, args.batch)):
        b = min(args.batch, args.frames - a)
        ori, pos = synth_poses(b, a)
        batches.append(({'torch': pool[k % 4][:b]}, {'ori': torch.from_numpy(ori), 'pos': torch.from_numpy(pos)}))
    return su, spe, batches


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
    from spef_amd.tools.evaluation import evaluation, evaluation_device
    su, spe, batches = _setup(args)
    rec = {'mode': args.mode, 'frames': args.frames, 'batch': args.batch, 'size': args.size, 'dtype': args.dtype,
           'reps': args.reps, 'gpu': torch.cuda.get_device_name(0)}
    loaders = {'valid': batches}

    def evaluation_dev(*a):
        return evaluation_device(*a, capacity=args.frames)
    if args.mode == 'kernels':
        evaluation_dev(spe, loaders, su, ('valid',))               # warm
        eng = spe.eval_pipeline().engine                           # the context the scorer launches through
        eng.profile_begin()
        for _ in range(args.reps):
            evaluation_dev(spe, loaders, su, ('valid',))
        prof = eng.profile_end()
        for key in ('score_step_kernel', 'score_finalize_kernel'):
            launches, ms = prof[key][0], prof[key][1]
            rec[f'{key}_launches'] = launches
            rec[f'{key}_us_per_launch'] = round(1e3 * ms / launches, 2)
    else:
        fn = evaluation if args.mode == 'host' else evaluation_dev
        out = {}

        def run():
            out['score'], out['error'] = fn(spe, loaders, su, ('valid',))
        med, lo, hi = _timed(run, args.reps)
        rec.update(ms_per_run=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
                   images_per_s=round(args.frames / med * 1e3, 1), esa_score=out['score']['valid']['esa'][0],
                   ori_mad=out['error']['valid']['ori_mad'][0])
    spe.close()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--mode', choices=MODES, help='run one measurement in this process (default: all, one child each)')
    ap.add_argument('--frames', type=int, default=1800)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--dtype', default='fp16mx')
    ap.add_argument('--reps', type=int, default=7)
    args = ap.parse_args()
    if args.mode:
        return run_mode(args)
    for mode in MODES:       # a fresh process per measurement; stop at the first that fails or runs out of time
        cmd = [sys.executable, os.path.abspath(__file__), '--mode', mode, '--frames', str(args.frames), '--batch',
               str(args.batch), '--size', str(args.size), '--dtype', args.dtype, '--reps', str(args.reps)]
        try:
            r = subprocess.run(cmd, timeout=LIMIT_S[mode])
        except subprocess.TimeoutExpired:
            print(f'eval_bench: {mode} ran out of time ({LIMIT_S[mode]} s); stopping', file=sys.stderr)
            return 124
        if r.returncode != 0:
            print(f'eval_bench: {mode} failed with status {r.returncode}; stopping', file=sys.stderr)
            return r.returncode
    return 0


if __name__ == '__main__':
    sys.exit(main())
