"""Seeded inputs for the forward tests that leave the two habits of every other forward test (grey frames, one decade
of activation magnitudes): tests/test_gpu_colour_frames.py and tests/test_gpu_channel_range.py on the GPU,
tests/test_input_sensitivity.py and tests/test_channel_range_host.py for what those inputs must themselves show, which
needs no GPU. No fixtures; the float64 restatement of the schedules' roundings lives here too, because the CPU test
that chooses the held channel-scale range and the GPU test that uses it must agree on it.

  * ``colour_frames``         uint8 NHWC, R, G and B independent ``blob_frames`` planes (bright borders kept)
  * ``float_frames``          float32 NCHW, uniform, not multiples of 1 / 255, optionally past [0, 1]
  * ``channel_fault``         the six channel faults a stem can have that grey frames cannot show
  * ``rescaled_state_dict``   a function-preserving re-parametrisation: every internal channel scaled by its own power
                              of two at its BatchNorm and unscaled at its one consumer
  * ``restated_block_errors`` a schedule's rounding points per block in float64, against the exact block
"""
import functools
import importlib.util
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle.block_ref import blob_frames
from spef_amd.arch import mobilenet_v2
from spef_amd.blob import fold_bn
from spef_amd.weights import synthetic_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (b, h, w) of tests/test_gpu_colour_frames.py: an odd byte count per image that reaches the stem's bottom and right
# padding, and the ragged even shape of the older tests
COLOUR_SHAPES = ((2, 33, 35), (1, 100, 136))
RANGE_SHAPE = (1, 100, 136)   # tests/test_gpu_channel_range.py
RANGE_SEED = 7                # of the drawn channel scales

# the six planted channel faults: source channel of (R, G, B) as the stem sees them
CHANNEL_FAULTS = {
    'swap_rg': (1, 0, 2), 'swap_rb': (2, 1, 0), 'swap_gb': (0, 2, 1),   # a wrong channel order in a packed operand
    'rotate': (1, 2, 0),                                                # an off-by-one channel index
    'r_three_times': (0, 0, 0), 'g_three_times': (1, 1, 1),             # a zero plane stride / a grey shortcut
}

# The channel-scale range [kmin, kmax] (a_c = 2^k) the GPU tests hold: the widest integer range in which the float64
# restatement of every hi + lo / fp16 schedule stays at or below a quarter of that schedule's block bound on every
# block. tests/test_channel_range_host.py asserts exactly that for the draw over [KMIN, KMAX], and that the one-sided
# draws over [KMIN - 1, 0] and [0, KMAX + 1] exceed the quarter (one-sided, because a wider two-sided draw puts fewer
# channels at either end and can pass where a narrower one does not).
# The stem's channels draw from [STEM_KMIN, KMAX] only. The fused front kernels take the stem weights with ToTensor's
# / 255 folded in, split hi + lo (spef_amd/blob.py x0 / x1): eight binades nearer the fp16 subnormal floor than any
# other operand, so that block 1 of fp16x2 through the front kernel sits at 0.27 of its bound on the unscaled weights
# already (restated 1.35e-5 of the map's max) and no stem channel can be scaled down within the quarter.
KMIN, KMAX = -6, 6
STEM_KMIN = 0

# block bounds of the existing suite (tests/test_gpu_odd_frames.py restates them with their sources)
X2_BLOCK_TOL = 5e-5
MX_F16_OUT_TOL, MX_F16_HIDDEN_TOL, MX_F32_TOL = 1.2e-3, 2e-4, 5e-5
MX_F16_BLOCKS, MX_F16_HIDDEN = range(1, 4), range(2, 5)
FP16_BLOCK_TOL = 2e-2
RESTATED_SHARE = 0.25   # of the bound: the rest is for fp32 accumulation order and the GPU's own rounding


def base_state_dict():
    return synthetic_state_dict(mobilenet_v2('ursonet', 1728, 3), seed=1001)


def colour_frames(b, h, w, seed):
    """uint8 NHWC colour frames: each channel is the grey plane of its own ``blob_frames`` draw (seeds 3 seed + c), so
    R, G and B are independent and the border pixels stay as bright as the interior."""
    return np.ascontiguousarray(np.stack([blob_frames(b, h, w, 3 * seed + c)[..., 0] for c in range(3)], axis=3))


def float_frames(b, h, w, seed, lo=0.0, hi=1.0):
    """float32 NCHW frames uniform in [lo, hi): independent channels, values that are no multiple of 1 / 255."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(rng.uniform(lo, hi, (b, 3, h, w)).astype(np.float32))


def channel_fault(x, fault):
    """NCHW float32 frames as a stem with the named channel fault would read them, in the strides of ``x`` (the
    oracle's convs sum in another order on another memory format, which is no effect of the fault)."""
    out = torch.empty_like(x)
    out.copy_(x[:, list(CHANNEL_FAULTS[fault])])
    assert out.stride() == x.stride()
    return out


def _scale_bn(sd, prefix, a):
    for nm in ('weight', 'bias'):
        sd[f'{prefix}.1.{nm}'] = (sd[f'{prefix}.1.{nm}'].astype(np.float32) * a).astype(np.float32)


def rescaled_state_dict(sd, arch, kmin, kmax, seed, stem_kmin=None):
    """-> (state_dict, {conv prefix: int k per output channel}). For every channel c of the stem output, every expand
    output, every depthwise output and the last conv's output, a_c = 2^k with k an integer uniform in [kmin, kmax]:
    that conv's BN weight and bias are multiplied by a_c and its one consumer's weights on input channel c divided by
    a_c (the depthwise filter c behind the stem and behind an expand, the project column c behind a depthwise, the head
    Linears' column c behind the last conv). ReLU commutes with a positive scale, so the network computes the same
    function; the scales are powers of two, so every float32 product and sum of the oracle keeps its significand.
    Block outputs (project convs, the residual stream) are left alone. ``stem_kmin`` raises the lower end for the stem's
    channels alone (STEM_KMIN above)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {k: np.array(v, copy=True) for k, v in sd.items()}
    ks = {}

    def draw(spec):
        lo, hi = kmin, kmax
        if spec is arch.stem and stem_kmin is not None:
            lo, hi = max(kmin, stem_kmin), max(kmax, stem_kmin)
        k = rng.integers(lo, hi + 1, spec.cout)
        ks[spec.prefix] = k
        a = np.exp2(k).astype(np.float32)
        _scale_bn(out, spec.prefix, a)
        return a

    def consume_dw(spec, a):      # depthwise [C, 1, 3, 3]: filter c reads channel c
        key = f'{spec.prefix}.0.weight'
        out[key] = (out[key] / a[:, None, None, None]).astype(np.float32)

    def consume_cols(key, a):     # 1x1 conv [N, C, 1, 1] or Linear [N, C]: column c reads channel c
        w = out[key]
        out[key] = (w / a.reshape((1, -1) + (1,) * (w.ndim - 2))).astype(np.float32)

    a = draw(arch.stem)
    for blk in arch.blocks:
        convs = list(blk.convs)
        if blk.expand != 1:
            a = draw(convs.pop(0))
        consume_dw(convs[0], a)             # block 1 (t = 1): the stem's consumer
        a = draw(convs[0])
        consume_cols(f'{convs[1].prefix}.0.weight', a)
    a = draw(arch.last)
    for key in ('head.ori.1.weight', 'head.pos.0.weight'):
        consume_cols(key, a)
    return out, ks


@functools.lru_cache(maxsize=None)
def rescaled(kmin=KMIN, kmax=KMAX, seed=RANGE_SEED, stem_kmin=STEM_KMIN):
    """The rescaled seed-1001 weights of the channel-range tests, computed once per process."""
    return rescaled_state_dict(base_state_dict(), mobilenet_v2('ursonet', 1728, 3), kmin, kmax, seed, stem_kmin)


# ------------------------------------------------------------------------- float64 restatement of the schedules
@functools.lru_cache(maxsize=None)
def _budget():
    """tools/precision_budget.py (the rounding rules r16 / r32 / hilo and the packed-fp16 depthwise accumulation)."""
    path = os.path.join(ROOT, 'tools', 'precision_budget.py')
    spec = importlib.util.spec_from_file_location('precision_budget', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SCHEDULES = ('fp16x2', 'fp16mx', 'fp16mx_fallback', 'fp16')


def schedule_bound(schedule, idx):
    """The existing suite's bound on block ``idx``'s output under ``schedule``, of the map's max."""
    if schedule == 'fp16x2':
        return X2_BLOCK_TOL
    if schedule == 'fp16':
        return FP16_BLOCK_TOL
    hidden = MX_F16_HIDDEN if schedule == 'fp16mx' else ()
    return MX_F16_OUT_TOL if idx in MX_F16_BLOCKS else MX_F16_HIDDEN_TOL if idx in hidden else MX_F32_TOL


class Restated:
    """One network's folded weights in float64 and its blocks under a schedule's rounding points.

    A 1x1 conv of the hi + lo schedules is the kernels' three-MFMA sum w_hi x_hi + w_lo x_hi + w_hi x_lo with
    hi = fp16(v), lo = fp16(f32(v) - hi) for weight and activation alike (csrc/x2_common.hpp split8 / mfma_x2), the
    lo lo term dropped, accumulated exactly here (the GPU accumulates in fp32: the quarter of the bound that the
    restatement leaves is for that). An activation the schedule stores in fp16 has no lo half. The depthwise is fp32
    arithmetic on fp32 weights: exact here up to the weights' float32 rounding."""

    def __init__(self, sd, arch):
        self.B = _budget()
        self.arch = arch
        self.w = {c.prefix: tuple(torch.from_numpy(t) for t in fold_bn(sd, c)) for c in arch.all_convs()}
        self.net16 = self.B.Net(sd, arch)

    def _conv(self, t, spec, w=None):
        w0, b = self.w[spec.prefix]
        w = w0 if w is None else w
        y = F.conv2d(t, w, b, spec.stride, (spec.k - 1) // 2, 1, spec.groups)
        return F.relu(y) if spec.relu else y

    def _pw_x2(self, t, spec, exact_in):
        """hi + lo 1x1 conv; ``exact_in``: the input is an fp16 tensor already (no lo half)."""
        r16, r32 = self.B.r16, self.B.r32
        w, b = self.w[spec.prefix]
        wh = r16(w)
        wl = r16(w - wh)                      # the packer splits the float64 folded weight (blob.split_f16)
        th = r16(t)
        y = F.conv2d(th, wh + wl)             # w_hi x_hi + w_lo x_hi
        if not exact_in:
            y = y + F.conv2d(r16(r32(t) - th), wh)   # + w_hi x_lo
        y = y + b.view(1, -1, 1, 1)
        return F.relu(y) if spec.relu else y

    def front_stem(self, frames_u8):
        """The stem as the fused front kernels compute it from u8 frames (op 1 of the GPU tests): the pixel 0..255 is an
        exact fp16 operand, ToTensor's / 255 is folded into the float32 weights and those are split hi + lo
        (spef_amd/blob.py x0 / x1) -- eight binades nearer the fp16 subnormal floor than the weights themselves."""
        r16 = self.B.r16
        w, b = self.w[self.arch.stem.prefix]
        w255 = (w.to(torch.float32) / torch.tensor(255.0, dtype=torch.float32)).to(torch.float64)
        wh = r16(w255)
        x = torch.from_numpy(frames_u8).permute(0, 3, 1, 2).to(torch.float64)
        return F.relu(F.conv2d(x, wh + r16(w255 - wh), b.to(torch.float32).to(torch.float64), 2, 1))

    def stored_input(self, x, blk, schedule):
        """The exact float64 block input ``x`` as the schedule holds it: fp16 under the fp16 schedule and where fp16mx
        stores the previous output in fp16 (blocks 2-4 read one; block 1 reads the fp16 stem map inside the fused front
        kernel), float32 otherwise."""
        if schedule == 'fp16':
            return self.B.r16(x)
        mx = schedule in ('fp16mx', 'fp16mx_fallback')
        f16_in = mx and (blk.index == 1 or (blk.index - 1) in MX_F16_BLOCKS)
        return self.B.r16(x) if f16_in else self.B.r32(x)

    def reference_block(self, x, blk, schedule, storage=True):
        """What the GPU tests compare a block with: the exact block on the input the schedule holds (the GPU's own
        previous probe) with, under ``storage``, the schedule's fp16 storage points restated -- the hidden tensors of
        blocks 2-4 under fp16mx, the outputs of blocks 1-3 under fp16mx and its fallback; nothing under fp16x2 and fp16.
        Block 1 is compared from the frames, so its reference reads the exact stem map."""
        r16 = self.B.r16
        mx = schedule in ('fp16mx', 'fp16mx_fallback')
        y = xin = x if blk.index == 1 else self.stored_input(x, blk, schedule)
        convs = list(blk.convs)
        if blk.expand != 1:
            y = self._conv(y, convs.pop(0))
            if storage and schedule == 'fp16mx' and blk.index in MX_F16_HIDDEN:
                y = r16(y)
        y = self._conv(self._conv(y, convs[0]), convs[1])
        y = y + xin if blk.residual else y
        return r16(y) if (storage and mx and blk.index in MX_F16_BLOCKS) else y

    def block(self, x, blk, schedule, storage=True):
        """Block ``blk`` on its exact float64 input ``x`` (block 1: on the front kernel's stem map, ``front_stem``)
        with every rounding point of the schedule. ``storage`` False leaves out the fp16mx storage roundings inside the
        block and at its output (the fp16 input stays: an fp16 operand has no lo half, which is arithmetic)."""
        B = self.B
        r16, r32 = B.r16, B.r32
        i = blk.index
        convs = list(blk.convs)
        xin = self.stored_input(x, blk, schedule)
        if i == 1 and not storage and schedule != 'fp16':
            xin = r32(x)     # t = 1: the stem map feeds the fp32 depthwise, no matrix operand; its fp16 form is storage
        if schedule == 'fp16':   # tools/precision_budget.py's own block under its fp16 rule
            return self.net16.block(xin, blk, B.sched_fp16)
        mx = schedule in ('fp16mx', 'fp16mx_fallback')
        f16_in = mx and (i == 1 or (i - 1) in MX_F16_BLOCKS)
        y = xin
        if blk.expand != 1:
            y = self._pw_x2(y, convs.pop(0), f16_in)
            y = r16(y) if (storage and schedule == 'fp16mx' and i in MX_F16_HIDDEN) else r32(y)
        y = r32(self._conv(y, convs[0], r32(self.w[convs[0].prefix][0])))
        y = self._pw_x2(y, convs[1], False)
        y = y + xin if blk.residual else y
        return r16(y) if (storage and mx and i in MX_F16_BLOCKS) else r32(y)


@torch.no_grad()
def restated_block_errors(sd, arch, frames_u8, schedules=SCHEDULES, storage=False):
    """{schedule: {block: max |restated - reference| / max |reference|}} for blocks 1..17, each on the exact float64
    output of the block before it -- block 1 from the u8 frames through the fused front kernel's stem operand, as
    the GPU tests compare it; inf where the restated block is not finite (an fp16 overflow).

    ``storage`` False (what the held range is chosen by) leaves the fp16mx storage roundings out of both sides. With
    them in, two tensors that were each rounded to fp16 are compared, and wherever the arithmetic error moves a value
    across a rounding boundary they differ by a whole fp16 step: 2^-11 to 2^-10 of the map's max for its largest
    values, at any channel scale and however small the arithmetic error is -- the reason the fp16-output bound is one
    step (1.2e-3) and not an arithmetic bound. A fp16 rounding commutes with a power-of-two scale short of overflow and
    of the subnormal range, which test_channel_range_host.py checks on the stored tensors themselves."""
    net = Restated(sd, arch)
    x = torch.from_numpy(frames_u8).permute(0, 3, 1, 2).to(torch.float64) / 255.0
    y = net._conv(x, arch.stem)
    out = {s: {} for s in schedules}
    front = net.front_stem(frames_u8)
    for blk in arch.blocks:
        for s in schedules:
            want = net.reference_block(y, blk, s, storage)
            got = net.block(front if blk.index == 1 else y, blk, s, storage)
            ok = bool(torch.isfinite(got).all())
            out[s][blk.index] = float((got - want).abs().max() / want.abs().max()) if ok else float('inf')
        y = net.reference_block(y, blk, 'fp16x2')
    return out
