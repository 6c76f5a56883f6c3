#!/usr/bin/env python3
"""Timing and accuracy of the INT8 calibration paths ("Calibration path"), synthetic weights and
frames. One measurement per run, one JSON line:

    python tools/calib_bench.py --mode compare  [--frames 16] [--height 512] [--width 512]
        quant.calibrate (host: torch CPU forward, np.percentile on the raw activations) against
        quant.calibrate_device (fp32 schedule + histogram observers) on the same frames: seconds of each and the
        largest relative difference between their scales
    python tools/calib_bench.py --mode stream   [--frames 1024] [--batch 64]
        calibrate_device alone over many frames (batches resident on the device), percentile and MSE
    python tools/calib_bench.py --mode kernel   [--batch 64]
        the observer kernel alone on the largest tap (block 2's expand output at --batch x 512 x 512: 96 channels at
        256 x 256, 1.6 GB at batch 64): GB/s for ReLU-like data (half zeros), all zeros (no LDS traffic) and one
        repeated value (every lane on one LDS address), next to the read peak spef_measure_peaks finds on this GPU
    python tools/calib_bench.py --mode accuracy [--frames 16,1024] [--eval-frames 64]
        int8 engine against the fp32 engine on held-out frames (largest |d orientation logit|, |d position|, angle
        between the decoded orientations) for scales from the percentile and MSE clips at each frame count, and for the
        host calibration on 4 frames of 128 x 128 (what bench.py and the tests use)

Times are host wall-clock around calls that end in a device synchronise.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'spacecraft-pose-estimation-framework_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def _sd():
    from spef_amd.arch import mobilenet_v2
    from spef_amd.spe.spe_utils import SPEUtils
    from spef_amd.weights import synthetic_state_dict
    su = SPEUtils(None, 'classification', 12, 3, False, 'regression')
    return su, synthetic_state_dict(mobilenet_v2('ursonet', su.orientation.n_bins, 3), seed=1001)   # bench.py's model


def _scales(qp):
    v = [qp['image'], qp['stem'], qp['final'], qp['last']]
    for b in qp['blocks']:
        v += [b[k] for k in ('quant', 'expand', 'dw') if b[k] is not None]
    return v


def _device_batches(n, batch, h, w, first=900):
    """n frames as device batches: up to 256 distinct synthetic frames, further batches spatially rolled copies made on
    the device (distinct bytes, same statistics), as bench.py's device_batches."""
    import torch
    from spef_amd.data.synthetic import synth_frames
    base = torch.from_numpy(synth_frames(min(n, 256), h, w, first)).cuda()
    out, k = [], 0
    while sum(b.shape[0] for b in out) < n:
        src = base if k == 0 else torch.roll(base, shifts=(37 * k, 53 * k), dims=(1, 2))
        for a in range(0, src.shape[0], batch):
            if sum(b.shape[0] for b in out) >= n:
                break
            out.append(src[a:a + min(batch, n - sum(b.shape[0] for b in out))].contiguous())
        k += 1
    return out


def mode_compare(a, rec):
    import numpy as np
    import torch
    from spef_amd import quant as Qt
    from spef_amd.data.synthetic import synth_frames
    _, sd = _sd()
    fr = synth_frames(a.frames, a.height, a.width, 900)
    t0 = time.perf_counter()
    host = Qt.calibrate(sd, fr)
    rec['host_seconds'] = round(time.perf_counter() - t0, 3)
    Qt.calibrate_device(sd, fr[:1], batch=a.batch)   # library load, first launches
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev = Qt.calibrate_device(sd, fr, batch=a.batch)
        ts.append(time.perf_counter() - t0)
    rec['device_seconds'] = round(statistics.median(ts), 4)
    rec['device_includes'] = 'fp32 blob pack, context, upload, observed forward, read, scales'
    rel = np.array(_scales(dev)) / np.array(_scales(host)) - 1
    rec['scale_rel_diff_min'], rec['scale_rel_diff_max'] = float(rel.min()), float(rel.max())


def mode_stream(a, rec):
    import torch
    from spef_amd import quant as Qt
    _, sd = _sd()
    batches = _device_batches(a.frames, a.batch, a.height, a.width)
    Qt.calibrate_device(sd, batches[:1])
    for method in ('percentile', 'mse'):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        Qt.calibrate_device(sd, batches, method=method)
        dt = time.perf_counter() - t0
        rec[f'{method}_seconds'] = round(dt, 3)
        rec[f'{method}_images_per_s'] = round(a.frames / dt, 1)


def mode_kernel(a, rec):
    import ctypes as C
    import torch
    from spef_amd import blob as Bl
    from spef_amd.engine import Engine
    _, sd = _sd()
    eng = Engine(Bl.pack(sd, dtype='fp32'), 'cuda:0')
    obs = eng.observer()
    n = a.batch * (a.height // 2) * (a.width // 2) * 96
    x = torch.randn(n, device='cuda:0').clamp_(min=0)
    data = {'relu': x, 'zeros': torch.zeros_like(x), 'repeated': torch.full_like(x, 1.2345)}
    rec['values'], rec['gbytes'] = n, round(n * 4 / 1e9, 3)
    for name, t in data.items():
        obs.update(3, t)
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            obs.update(3, t)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        rec[f'{name}_ms'] = round(statistics.median(ms), 4)
        rec[f'{name}_gb_per_s'] = round(n * 4 / statistics.median(ms) / 1e6, 1)
    obs.close()
    del data, x
    torch.cuda.empty_cache()
    peaks = (C.c_double * 8)()
    if eng.lib.spef_measure_peaks(0, 3, peaks) == 0:
        rec['read_peak_gb_per_s'] = round(peaks[3], 1)
    eng.close()


def mode_accuracy(a, rec):
    import numpy as np
    import torch
    from oracle import decode_ref as D
    from spef_amd import blob as Bl
    from spef_amd import quant as Qt
    from spef_amd.blob_q8 import pack_int8
    from spef_amd.data.synthetic import synth_frames
    from spef_amd.engine import Engine
    su, sd = _sd()
    ev = torch.from_numpy(synth_frames(a.eval_frames, a.height, a.width, 50000)).cuda()

    def run(blob):
        e = Engine(blob, 'cuda:0')
        e.set_decode_tables(su.orientation.histogram, None)
        o, p = e.forward(ev)
        q = e.decode(1, 0, o, p, want_soft=False)['ori']
        out = o.cpu().numpy(), p.cpu().numpy(), q.cpu().numpy().astype(np.float64)
        e.close()
        return out
    o0, p0, q0 = run(Bl.pack(sd, dtype='fp32'))

    def err(qp):
        o, p, q = run(pack_int8(sd, qp))
        return {'ori_logit_max_abs': float(np.abs(o - o0).max()), 'pos_max_abs_m': float(np.abs(p - p0).max()),
                'ori_max_deg': float(D.angle_deg_stable(q, q0).max()),
                'ori_mean_deg': float(D.angle_deg_stable(q, q0).mean())}
    rec['eval_frames'] = a.eval_frames
    rec['host_4x128_percentile'] = err(Qt.calibrate(sd, synth_frames(4, 128, 128, 900)))
    for n in [int(v) for v in str(a.frames).split(',')]:
        batches = _device_batches(n, a.batch, a.height, a.width)
        for method in ('percentile', 'mse'):
            rec[f'device_{n}_{method}'] = err(Qt.calibrate_device(sd, batches, method=method))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--mode', choices=['compare', 'stream', 'kernel', 'accuracy'], required=True)
    ap.add_argument('--frames', default=None, help='frame count (accuracy: a comma list)')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--height', type=int, default=512)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--eval-frames', type=int, default=64)
    ap.add_argument('--reps', type=int, default=7)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print('calib_bench: no GPU visible', file=sys.stderr)
        return 2
    default = {'compare': 16, 'stream': 1024, 'kernel': 0, 'accuracy': '16,1024'}[a.mode]
    if a.mode != 'accuracy':
        a.frames = int(a.frames) if a.frames is not None else default
    elif a.frames is None:
        a.frames = default
    rec = {'mode': a.mode, 'frames': a.frames, 'batch': a.batch, 'size': [a.height, a.width],
           'gpu': torch.cuda.get_device_name(0)}
    {'compare': mode_compare, 'stream': mode_stream, 'kernel': mode_kernel, 'accuracy': mode_accuracy}[a.mode](a, rec)
    print(json.dumps(rec), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
