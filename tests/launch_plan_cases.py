"""The launch-plan cases: which kernel runs for every block of every schedule, under every schedule option.

tools/record_launch_plan.py records them into tests/golden/launch_plan.json and tests/test_gpu_launch_plan.py replays
them. A case is one entry point of one engine on one input under one option set; its fingerprint is what the profiler
keeps per kernel key without any timing -- the launch count and the algorithmic bytes and flops -- plus the output
shapes and a SHA-256 of the raw output bytes. The shapes are the smallest at which each branch of the schedulers is
taken:

  * ``u8_96x160``   B = 2 uint8 NHWC, final map 3 x 5: no multiple of 64 pixels, the unfused last conv + mean_hw
  * ``u8_256x256``  B = 1 uint8 NHWC, final map 8 x 8: x2_pw_pool and pool_gemm
  * ``f32_96x160``  B = 2 float32 NCHW: no fused front kernel
  * ``kp_240x384``  B = 1 uint8 NHWC at the keypoint head's own size
"""
import functools
import hashlib

import numpy as np
import torch

from spef_amd import _lib as L
from spef_amd import blob as Bl
from spef_amd.arch import mobilenet_v2
from spef_amd.blob_q8 import pack_int8
from spef_amd.data.synthetic import synth_frames
from spef_amd.engine import Engine
from spef_amd.quant import calibrate
from spef_amd.weights import synthetic_state_dict

INPUTS = {'u8_96x160': (2, 96, 160, 'u8'), 'u8_256x256': (1, 256, 256, 'u8'), 'f32_96x160': (2, 96, 160, 'f32'),
          'kp_240x384': (1, 240, 384, 'u8')}
LAST_BLOCK = 17   # op index of the last inverted residual (op 0 is the stem)

# every schedule option at the library's default; a case overrides some
DEFAULTS = {'fuse': 1, 'fuse_min_hw': 0, 'gemm': 1, 'wavespec': 2, 'q8_rolesplit': 0, 'mx_kernels': 1,
            'trim': L.OPT_TRIM_DEFAULT}
OPTION_IDS = {'fuse': L.OPT_FUSE_BLOCKS, 'fuse_min_hw': L.OPT_FUSE_MIN_HW, 'gemm': L.OPT_PW_GEMM,
              'wavespec': L.OPT_WAVESPEC, 'q8_rolesplit': L.OPT_Q8_ROLESPLIT, 'mx_kernels': L.OPT_MX_KERNELS,
              'trim': L.OPT_TRIM}


def _cases():
    """-> {case id: (engine, input, entry, options)}; entry: 'forward', 'backbone', 'observe', 'observe_feat' or
    ('probe', stop_op). The observe entries' outputs include the observer's records of that one run."""
    out = {}

    def add(engine, inp, entry, **opts):
        tag = entry if isinstance(entry, str) else f'probe{entry[1]}'
        name = '-'.join([engine, inp, tag] + [f'{k}{v}' for k, v in opts.items()])
        assert name not in out, name
        out[name] = (engine, inp, entry, opts)

    for inp in ('u8_96x160', 'u8_256x256', 'f32_96x160'):
        add('fp32', inp, 'forward')
        add('fp16x2', inp, 'forward')
        add('fp16x2', inp, 'backbone')
    add('fp32', 'u8_96x160', 'backbone')
    for inp in ('u8_96x160', 'f32_96x160'):
        add('fp32', inp, 'observe')        # last conv into a workspace buffer
        add('fp32', inp, 'observe_feat')   # last conv straight into the caller's feature map
    for dt in ('fp16', 'bf16'):
        for fuse, gemm, wavespec in ((1, 1, 2), (1, 1, 1), (1, 1, 0), (0, 1, 2), (0, 0, 2)):
            for inp in ('u8_96x160', 'u8_256x256'):
                add(dt, inp, 'forward', fuse=fuse, gemm=gemm, wavespec=wavespec)
        add(dt, 'f32_96x160', 'forward')
        add(dt, 'f32_96x160', 'forward', fuse=0)
        # 48 x 80 and 24 x 40 maps fuse, 12 x 20 and smaller do not
        add(dt, 'u8_96x160', 'forward', fuse_min_hw=400)
        add(dt, 'u8_96x160', 'backbone')
    for mx_kernels, trim in ((1, 3), (1, 1), (1, 0), (0, 3)):
        for inp in ('u8_96x160', 'u8_256x256'):
            add('fp16mx', inp, 'forward', mx_kernels=mx_kernels, trim=trim)
    add('fp16mx', 'f32_96x160', 'forward')
    for fuse in (1, 0):
        for rolesplit in (0, 1):
            for inp in ('u8_96x160', 'u8_256x256'):
                add('int8', inp, 'forward', fuse=fuse, q8_rolesplit=rolesplit)
    add('int8', 'f32_96x160', 'forward')
    add('int8', 'u8_96x160', 'backbone')
    for eng in ('fp16', 'fp16mx', 'int8'):
        for stop in (0, 1, 4, LAST_BLOCK):
            add(eng, 'u8_96x160', ('probe', stop))
    add('kp_fp16x2', 'kp_240x384', 'forward')
    add('kp_fp32', 'kp_240x384', 'forward')
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def _ursonet_sd():
    return synthetic_state_dict(mobilenet_v2('ursonet', 1728, 3), seed=1001)


@functools.lru_cache(maxsize=None)
def engine(name):
    """One engine per schedule, kept for the process."""
    if name.startswith('kp_'):
        arch = mobilenet_v2('keypoints')
        sd = synthetic_state_dict(arch, seed=1001, head_std=0.002)
        return Engine(Bl.pack(sd, arch, dtype=name[3:]), 'cuda:0')
    sd = _ursonet_sd()
    if name == 'int8':
        return Engine(pack_int8(sd, calibrate(sd, synth_frames(4, 128, 128, 900))), 'cuda:0')
    return Engine(Bl.pack(sd, mobilenet_v2('ursonet', 1728, 3), dtype=name), 'cuda:0')


@functools.lru_cache(maxsize=None)
def frames(name):
    b, h, w, kind = INPUTS[name]
    fr = torch.from_numpy(synth_frames(b, h, w, 7))
    if kind == 'f32':
        fr = (fr.permute(0, 3, 1, 2).to(torch.float32) / 255.0).contiguous()
    return fr.cuda()


@functools.lru_cache(maxsize=None)
def _observer(name):
    return engine(name).observer()


def _call(eng_name, inp, entry):
    eng, x = engine(eng_name), frames(inp)
    if entry == 'forward':
        return [t for t in eng.forward(x) if t is not None]
    if entry == 'backbone':
        return [eng.backbone(x)]
    if entry in ('observe', 'observe_feat'):
        b, h, w, _ = INPUTS[inp]
        f = torch.zeros((b, -(-h // 32), -(-w // 32), 1280), dtype=torch.float32, device=eng.device)
        obs = _observer(eng_name)
        obs.reset()
        obs.observe(x, f if entry == 'observe_feat' else None)
        counters, hist = obs.read()   # integer records: part of the output
        return ([f] if entry == 'observe_feat' else []) + [torch.from_numpy(a.view(np.int64)) for a in (counters, hist)]
    return [eng.probe(x, entry[1])]


def _digest(outs):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in outs:
        h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
    return h.hexdigest()


def run_case(case_id):
    """One unprofiled and one profiled run of the case -> (plan {key: [n, bytes, flops]} with bytes and flops as the
    profiler prints them, output shapes, [SHA-256 of each run's output bytes])."""
    eng_name, inp, entry, opts = CASES[case_id]
    eng = engine(eng_name)
    for k, v in {**DEFAULTS, **opts}.items():
        eng.set_option(OPTION_IDS[k], v)
    try:
        first = _call(eng_name, inp, entry)
        hashes = [_digest(first)]
        eng.profile_begin()
        try:
            outs = _call(eng_name, inp, entry)
        finally:
            prof = eng.profile_end()
        hashes.append(_digest(outs))
    finally:
        for k, v in DEFAULTS.items():
            eng.set_option(OPTION_IDS[k], v)
    plan = {k: [int(v[0]), '%.1f' % v[2], '%.1f' % v[3]] for k, v in prof.items()}
    return plan, [list(t.shape) for t in outs], hashes


def compute_units():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)
