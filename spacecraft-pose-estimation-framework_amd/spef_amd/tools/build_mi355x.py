"""Build an experiment for the MI355X target (the analogue of build_nvidia.py / build_tvm.py).

    python -m spef_amd.tools.build_mi355x --experiment experiments/train/<name> [--dtype fp16mx|fp16x2|fp16|bf16|int8|fp32]
        [--eval-variants fp32,fp16mx,fp16x2,fp16,bf16,int8 | none] [--eval-batches N]
        [--calib host|device] [--calib-method percentile|mse|max] [--calib-frames N]
    python -m spef_amd.tools.build_mi355x --synthetic --out experiments/build/mi355x/synthetic

Reads ``config.yaml`` + ``model/parameters.pt`` (+ ``model/bit_width.json`` for quantized models) of a
reference training experiment (eval.py:20-27 layout; the checkpoint is loaded with ``weights_only=True``),
folds BN and packs the weight blob (fp16/bf16, or int8 with activation scales calibrated on frames), and writes
``experiments/build/mi355x/<name>/{model.spef, config.yaml, build.json}``.

int8 calibration (``MI355X.CALIB_*``): ``--calib host`` (the default) runs the float model in torch on the CPU over the
raw activations (``quant.calibrate``); ``--calib device`` streams the frames through the fp32 schedule on the GPU
with a histogram observer behind every quantizer (``quant.calibrate_device``: any number of frames, percentile, MSE
or max clips as build_nvidia.py:86-127 offers) and is an error when no GPU is visible. ``build.json`` records where
the calibration ran, the method, the frame count and the seconds.

Then, like build_nvidia.py:331-343 / build_tvm.py:219-231 (every lowering variant evaluated on the host with the same
``evaluation()``), each precision variant of the experiment -- fp32 (the reference's arithmetic), fp16mx (the default:
fp16x2 weights with fp16 storage of the early activations only, within ~5e-4 of fp32 at a trained-scale head), fp16x2
(fp32 activations, hi + lo fp16 MFMA operands: within ~2e-5 of fp32 at any head scale), fp16, bf16 and int8 -- is
built in memory and evaluated on the same frames (``eval_host/eval_<variant>.json``), and
``eval_host/variants.json`` compares every variant's head outputs and poses with the fp32 variant's (the
spe_finn.py:116-149 statistics, tools/compare.py) and, when the caller passes the reference model
(``build(..., reference=callable)``: float32 NCHW images -> (ori, pos) raw head outputs), with the reference's.
Needs a GPU; skipped (with a note in build.json) when none is visible. Keypoint experiments asking for fp16 or
fp16mx (the default) get the fp16x2 blob: EPnP amplifies keypoint error (test_gpu_keypoints.py), and the fp16
keypoint head exceeds the 1e-3 output bound.

The build refuses to ship a floating-point blob that misses the north star's bound (raw head outputs 1e-3, pose
0.1 deg / 1 mm) against the fp32 variant on the evaluation frames: it rebuilds as fp16x2 when that variant is within
the bound (``build.json`` records the ``fallback``), and otherwise exits with status 3 -- unless
``--allow-out-of-bound`` is given, which keeps the requested blob with a warning (int8 has its own, wider bound).
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time


def calibrate_frames(sd, cfg, calib_frames, bit_width=None, info=None):
    """The int8 activation scales on ``calib_frames``, on the host or on the device as ``cfg.MI355X.CALIB_*`` says.
    ``info`` (a dict) receives where it ran, the method, the frame count and the seconds."""
    from ..quant import calibrate, calibrate_device
    m = cfg.MI355X
    t0 = time.time()
    if m.CALIB_ON_DEVICE:
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError('the calibration was asked to run on the device (--calib device / '
                               'MI355X.CALIB_ON_DEVICE) and no GPU is visible; --calib host runs it on the CPU')
        qp = calibrate_device(sd, calib_frames, device=m.DEVICE, batch=min(m.BATCH_SIZE, 64), bw=bit_width,
                              method=m.CALIB_METHOD, percentile=m.CALIB_PERCENTILE,
                              residual=cfg.MODEL.BACKBONE.RESIDUAL)
    else:
        if m.CALIB_METHOD == 'max':
            raise ValueError("the host calibration offers 'percentile' and 'mse'; 'max' needs --calib device")
        qp = calibrate(sd, calib_frames, percentile=m.CALIB_PERCENTILE, residual=cfg.MODEL.BACKBONE.RESIDUAL,
                       bw=bit_width, method=m.CALIB_METHOD)
    if info is not None:
        info.update({'where': 'device' if m.CALIB_ON_DEVICE else 'host', 'method': m.CALIB_METHOD,
                     'percentile': m.CALIB_PERCENTILE, 'frames': int(len(calib_frames)),
                     'seconds': round(time.time() - t0, 3)})
    return qp


def pack_variant(sd, cfg, arch, dtype: str, calib_frames=None, bit_width=None, calib_info=None):
    """-> (blob bytes, int8 quantisation parameters or None)."""
    from .. import blob as Bl
    if dtype == 'int8':
        from ..blob_q8 import pack_int8
        assert calib_frames is not None, 'int8 builds calibrate activation scales on frames'
        qp = calibrate_frames(sd, cfg, calib_frames, bit_width, calib_info)
        return pack_int8(sd, qp, arch), qp
    return Bl.pack(sd, arch, dtype=dtype), None


def evaluate_variants(sd, cfg, arch, out_dir: str, variants, calib_frames=None, bit_width=None, reference=None,
                      n_batches: int = 2, camera=None) -> dict:
    """Host evaluation of every precision variant on the same synthetic SPEED-style batches (build_nvidia.py:331-343).
    Writes eval_host/eval_<variant>.json ({score, error} of evaluation()) and eval_host/variants.json; returns the
    latter. ``reference``: optional callable, float32 NCHW [0,1] images -> (ori, pos) raw head outputs."""
    import numpy as np
    import torch
    from ..config import keypoint_consensus, keypoint_refine, to_spe_utils
    from ..data.synthetic import speed_like_loader
    from ..spe_mi355x import SPEMi355x
    from .compare import feature_stats
    from .evaluation import evaluation
    dev = torch.device(f'cuda:{cfg.MI355X.DEVICE}')
    su = to_spe_utils(cfg, camera)
    size, B = tuple(cfg.DATA.IMG_SIZE), cfg.MI355X.BATCH_SIZE
    batches = list(speed_like_loader(n_batches, B, size))
    x0 = batches[0][0]['torch']
    xf = x0.permute(0, 3, 1, 2).float().div(255.0)        # ToTensor() of the same frames (the reference's input)
    ed = os.path.join(out_dir, 'eval_host')
    os.makedirs(ed, exist_ok=True)
    outs, poses, summary = {}, {}, {'frames': int(B * n_batches), 'img_size': list(size), 'variants': {}}
    for v in variants:
        blob, _ = pack_variant(sd, cfg, arch, v, calib_frames, bit_width)
        spe = SPEMi355x(blob, dev, su, keypoint_refine=keypoint_refine(cfg),
                        keypoint_consensus=keypoint_consensus(cfg))
        try:
            score, error = evaluation(spe, {'synthetic': batches}, su, ('synthetic',))
            with open(os.path.join(ed, f'eval_{v}.json'), 'w') as f:
                json.dump({'score': score, 'error': error}, f, indent=1)
            o, p = spe.engine.forward(x0.to(dev))
            outs[v] = np.concatenate([o.cpu().numpy()] + ([p.cpu().numpy()] if p is not None else []), axis=1)
            poses[v], _ = spe.predict(x0)
            summary['variants'][v] = {'esa_score': score['synthetic']['esa'][0], 'blob_bytes': len(blob)}
        finally:
            spe.close()
    ref_out = None
    if reference is not None:
        with torch.no_grad():
            ro, rp = reference(xf)
        ref_out = np.concatenate([np.asarray(ro, np.float32), np.asarray(rp, np.float32)] if rp is not None and
                                 np.asarray(rp).size else [np.asarray(ro, np.float32)], axis=1)
    base = 'fp32' if 'fp32' in outs else None
    for v in outs:
        rec = summary['variants'][v]
        if base and v != base:
            rec['vs_fp32_variant'] = feature_stats(outs[v], outs[base])
            qa, qb = poses[v]['ori'].astype(np.float64), poses[base]['ori'].astype(np.float64)
            d = np.abs(np.sum(qa * qb, axis=1)) / (np.linalg.norm(qa, axis=1) * np.linalg.norm(qb, axis=1))
            rec['vs_fp32_variant']['ori_max_deg'] = float(np.degrees(2 * np.arccos(np.clip(d, 0, 1))).max())
            rec['vs_fp32_variant']['pos_max_m'] = float(np.linalg.norm(poses[v]['pos'] - poses[base]['pos'], axis=1).max())
            # the north star's bound (raw outputs 1e-3, pose 0.1 deg / 1 mm) against the fp32 variant on these frames:
            # fp16 storage error scales with the output range, so a trained head may fail it
            vs = rec['vs_fp32_variant']
            rec['within_north_star'] = bool(vs['max_abs'] < 1e-3 and vs['ori_max_deg'] < 0.1 and vs['pos_max_m'] < 1e-3)
        if ref_out is not None:
            rec['vs_reference'] = feature_stats(outs[v], ref_out)
    if base:
        summary['within_north_star'] = [base] + [v for v in outs if summary['variants'][v].get('within_north_star')]
    with open(os.path.join(ed, 'variants.json'), 'w') as f:
        json.dump(summary, f, indent=1)
    return summary


def build(sd, cfg, out_dir: str, dtype: str, calib_frames=None, bit_width=None) -> dict:
    """``bit_width``: the experiment's bit_width.json as quant.BitWidths (int8 only; None = all 8 bits)."""
    from ..arch import arch_from_state_dict
    os.makedirs(out_dir, exist_ok=True)
    arch = arch_from_state_dict(sd, residual=cfg.MODEL.BACKBONE.RESIDUAL)
    t0 = time.time()
    calib_info = {}
    blob, qp = pack_variant(sd, cfg, arch, dtype, calib_frames, bit_width, calib_info)
    if qp is not None:
        import dataclasses
        with open(os.path.join(out_dir, 'qparams.json'), 'w') as f:
            json.dump(dict(qp, bits=dataclasses.asdict(qp['bits'])), f, indent=1)
    with open(os.path.join(out_dir, 'model.spef'), 'wb') as f:
        f.write(blob)
    cfg.MI355X.DTYPE = dtype
    from ..config import save_config
    save_config(cfg, os.path.join(out_dir, 'config.yaml'))
    info = {'dtype': dtype, 'bytes': len(blob), 'sha256': hashlib.sha256(blob).hexdigest(), 'head': arch.head,
            'n_ori': arch.n_ori, 'n_pos': arch.n_pos, 'pack_seconds': round(time.time() - t0, 3)}
    if qp is not None:
        info['calibration'] = calib_info
    with open(os.path.join(out_dir, 'build.json'), 'w') as f:
        json.dump(info, f, indent=1)
    return info


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--experiment', help='reference experiment dir with config.yaml and model/parameters.pt')
    ap.add_argument('--synthetic', action='store_true', help='seeded synthetic weights (no checkpoint offline)')
    ap.add_argument('--dtype', choices=['fp16mx', 'fp16x2', 'fp16', 'bf16', 'int8', 'fp32'])
    ap.add_argument('--out')
    ap.add_argument('--eval-variants', default='auto',
                    help="comma list of fp32,fp16mx,fp16x2,fp16,bf16,int8 to evaluate on the host after the build, 'none', or "
                         "'auto' (all that apply, when a GPU is visible)")
    ap.add_argument('--eval-batches', type=int, default=2)
    ap.add_argument('--allow-out-of-bound', action='store_true',
                    help='keep the requested floating-point blob even when it misses the 1e-3 / 0.1 deg / 1 mm bound '
                         'against the fp32 variant (default: fall back to fp16x2, or fail)')
    ap.add_argument('--calib', choices=['host', 'device'],
                    help='int8: where the activation scales are calibrated (default: MI355X.CALIB_ON_DEVICE, host); '
                         'device needs a GPU')
    ap.add_argument('--calib-method', choices=['percentile', 'mse', 'max'], help='default: MI355X.CALIB_METHOD')
    ap.add_argument('--calib-frames', type=int, help='default: MI355X.CALIB_FRAMES')
    ap.add_argument('--synthetic-head-std', type=float, default=None,
                    help='--synthetic: orientation Linear init std (default: the reference init, 0.01); 0.3 gives the '
                         'trained-scale heads of the reference-generated predict fixtures')
    a = ap.parse_args(argv)
    import torch
    from ..config import load_config
    from ..data.synthetic import synth_frames
    if a.experiment:
        cfg = load_config(os.path.join(a.experiment, 'config.yaml'))
        sd = torch.load(os.path.join(a.experiment, 'model', 'parameters.pt'), map_location='cpu', weights_only=True)
        bit_width = None
        bw_path = os.path.join(a.experiment, 'model', 'bit_width.json')
        if os.path.exists(bw_path):
            from ..quant import parse_bit_width
            bit_width = parse_bit_width(bw_path)
        name = os.path.basename(os.path.normpath(a.experiment))
    elif a.synthetic:
        bit_width = None
        from ..arch import mobilenet_v2
        from ..weights import synthetic_state_dict
        cfg = load_config(None)
        h = cfg.MODEL.HEAD
        from ..spe.spe_utils import SPEUtils
        su = SPEUtils(None, h.ORI, h.N_ORI_BINS_PER_DIM, cfg.DATA.ORI_SMOOTH_FACTOR, h.ORI_DELETE_UNUSED_BINS, h.POS,
                      h.N_POS_BINS_PER_DIM, cfg.DATA.POS_SMOOTH_FACTOR)
        n_ori = su.orientation.n_bins if h.ORI == 'classification' else 4
        n_pos = su.position.n_bins if h.POS == 'classification' else 3
        sd = synthetic_state_dict(mobilenet_v2('ursonet', n_ori, n_pos), seed=1001,
                                  **({} if a.synthetic_head_std is None else
                                     {'head_std': a.synthetic_head_std, 'pos_std': 0.01, 'pos_bias': (0.3, -0.2, 12.0)}))
        name = 'synthetic'
    else:
        ap.error('--experiment or --synthetic')
    keypoints = cfg.MODEL.HEAD.ORI == 'keypoints'
    dtype = a.dtype or ('fp16x2' if keypoints and cfg.MI355X.DTYPE in ('fp16', 'fp16mx') else cfg.MI355X.DTYPE)
    out = a.out or os.path.join('experiments', 'build', 'mi355x', name)
    if a.calib:
        cfg.MI355X.CALIB_ON_DEVICE = a.calib == 'device'
    if a.calib_method:
        cfg.MI355X.CALIB_METHOD = a.calib_method
    if a.calib_frames:
        cfg.MI355X.CALIB_FRAMES = a.calib_frames
    if dtype == 'int8' and cfg.MI355X.CALIB_ON_DEVICE and not torch.cuda.is_available():
        ap.error('--calib device: no GPU is visible (--calib host calibrates on the CPU)')
    calib = synth_frames(cfg.MI355X.CALIB_FRAMES, *cfg.DATA.IMG_SIZE, 900)
    info = build(sd, cfg, out, dtype, calib if dtype == 'int8' else None, bit_width)
    rc = 0
    if a.eval_variants != 'none':
        variants = (['fp32', 'fp16mx', 'fp16x2', 'fp16', 'bf16'] + ([] if keypoints else ['int8'])) if a.eval_variants == 'auto' else \
            [v for v in a.eval_variants.split(',') if v]
        if dtype not in ('int8', 'fp32'):   # the bound check needs the fp32 reference, the built dtype and the fallback
            variants += [v for v in ('fp32', dtype, 'fp16x2') if v not in variants]
        if torch.cuda.is_available():
            from ..arch import arch_from_state_dict
            from ..spe.camera import CAMERAS
            camera = CAMERAS['speed_plus' if 'plus' in cfg.DATA.PATH else 'speed']
            info['eval_host'] = evaluate_variants(sd, cfg, arch_from_state_dict(sd, residual=cfg.MODEL.BACKBONE.RESIDUAL),
                                                  out, variants, calib, bit_width, n_batches=a.eval_batches,
                                                  camera=camera)
            ok = info['eval_host'].get('within_north_star')
            if ok is not None and dtype not in ok and dtype != 'int8':
                miss = (f'the built {dtype} blob exceeds the 1e-3 / 0.1 deg / 1 mm bound against the fp32 variant on the '
                        f'evaluation frames ({info["eval_host"]["variants"][dtype]["vs_fp32_variant"]["max_abs"]:.2e} max '
                        f'|d raw output|); variants within it: {ok}')
                if a.allow_out_of_bound:
                    info['warning'] = miss + '; kept (--allow-out-of-bound)'
                    print('warning:', info['warning'], file=sys.stderr)
                elif 'fp16x2' in ok:
                    requested = dtype
                    info = dict(build(sd, cfg, out, 'fp16x2', None, bit_width), eval_host=info['eval_host'])
                    info['fallback'] = {'requested': requested, 'built': 'fp16x2', 'reason': miss}
                    print(f'note: {miss}; rebuilt as fp16x2', file=sys.stderr)
                else:
                    info['error'] = miss + '; no variant to fall back to (pass --allow-out-of-bound to keep it)'
                    print('error:', info['error'], file=sys.stderr)
                    rc = 3
        else:
            info['eval_host'] = 'skipped: no GPU visible (run the build on the MI355X box to evaluate the variants)'
        with open(os.path.join(out, 'build.json'), 'w') as f:
            json.dump(info, f, indent=1)
    print(json.dumps(info))
    return rc


if __name__ == '__main__':
    sys.exit(main())
