"""INT8 quantisation parameters of the Brevitas-mirroring path.

The reference's quantized model (``QMobileNetV2`` + ``QURSONetHead``; src/modeling/backbone/mobilenet_v2.py:
119-229, common/brevitas_layers.py:10-136, head/ursonet.py:36-93) carries one learned scale per activation
quantizer; weight scales are statistics of the weights (per output channel, quantizers.py:16-20) and are
recomputed at pack time. ``QParams`` holds the activation scales in the reference graph's order:

    image              input QuantIdentity (signed 8-bit)                     mobilenet_v2.py:177-178
    stem               stem QuantReLU (unsigned)                                               :179-182
    blocks[i].quant    shared signed quantizer of block i (None for block 1)   brevitas_layers.py:126-136
    blocks[i].expand   expand QuantReLU (None when t == 1)                                      :103-111
    blocks[i].dw       depthwise QuantReLU                                                      :113-119
    final              signed QuantIdentity after the last block               mobilenet_v2.py:208-211
    last               last conv QuantReLU                                                      :213-217

There is no QAT checkpoint in this environment (the reference's trained models are remote downloads), so
``calibrate`` sets the scales from activation statistics of the float model on calibration frames --
Brevitas' own initialisation of ``ParameterFromRuntimeStats`` scales (a high percentile of |x|) -- which
stands in for QAT.

Bit widths (``BitWidths``, parsed from the reference's ``bit_width.json``, model.py:16-45): every quantizer
keeps its own width from 3 to 8 bits, held in int8 containers -- weights per output channel in
[-(2^(b-1) - 1), 2^(b-1) - 1] (narrow range), unsigned ReLU quantizers in [0, 2^b - 1], the signed shared /
input quantizers in [-2^(b-1), 2^(b-1) - 1]. The reference's ``QMobileNetV2`` default is 3-bit weights and
activations with a 4-bit shared quantizer (mobilenet_v2.py:140-167, ``BitWidths.qmobilenet_default()``);
``config/train/exp_1/bit_width.json`` is all 8 (``BitWidths()``). Widths 1 and 2 select Brevitas' binary /
ternary quantizers (quantizers.py:78-96), a different arithmetic, and are rejected.
"""
from __future__ import annotations

import ast
import json
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from .arch import IR_SETTINGS, mobilenet_v2

FP = 'features.features'


N_BLOCKS = 17


@dataclass(frozen=True)
class BitWidths:
    """Quantizer bit widths of the reference's quantized model, in ``bit_width.json`` terms (model.py:16-45):
    ``inverted_residual[i] = ((expand_w, expand_act), (dw_w, dw_act), (project_w,))``, ``(None, None)`` for the
    expand of t == 1 blocks. Defaults: all 8 (``config/train/exp_1/bit_width.json``)."""
    image: int = 8
    first_conv: Tuple[int, int] = (8, 8)
    last_conv: Tuple[int, int] = (8, 8)
    fully_connected: Tuple[int, int] = (8, 8)
    shared_act: int = 8
    pooling: int = 8
    inverted_residual: Tuple = tuple(((8, 8), (8, 8), (8,)) for _ in range(N_BLOCKS))

    @staticmethod
    def qmobilenet_default() -> 'BitWidths':
        """QMobileNetV2's built-in default (mobilenet_v2.py:140-167) + QURSONetHead's 8-bit head."""
        ir = (((None, None), (3, 3), (3,)),) + tuple(((3, 3), (3, 3), (3,)) for _ in range(N_BLOCKS - 1))
        return BitWidths(8, (3, 3), (3, 3), (8, 8), 4, 8, ir)

    def block(self, i: int):
        """-> (expand_w, expand_act, dw_w, dw_act, project_w) of inverted residual i (0-based)."""
        (ew, ea), (dw, da), (pw,) = self.inverted_residual[i]
        return ew, ea, dw, da, pw

    def all_widths(self) -> List[int]:
        v = [self.image, *self.first_conv, *self.last_conv, *self.fully_connected, self.shared_act, self.pooling]
        for b in self.inverted_residual:
            v += [x for t in b for x in t if x is not None]
        return v


def parse_bit_width(path_or_dict) -> BitWidths:
    """A reference ``bit_width.json`` (path, or the dict ``load_bit_width`` returns; string values are parsed with
    ``ast.literal_eval`` like model.py:33-38) -> ``BitWidths``. Missing keys keep their 8-bit default."""
    d = path_or_dict
    if not isinstance(d, dict):
        with open(d) as f:
            d = json.load(f)
    lit = lambda x: ast.literal_eval(x) if isinstance(x, str) else x   # noqa: E731
    kw = {}
    for k in ('image', 'shared_act', 'pooling'):
        if k in d:
            kw[k] = int(lit(d[k]))
    for k in ('first_conv', 'last_conv', 'fully_connected'):
        if k in d:
            kw[k] = tuple(int(x) for x in lit(d[k]))
    if 'inverted_residual' in d:
        ir = [tuple(tuple(t) for t in lit(b)) for b in d['inverted_residual']]
        if len(ir) != N_BLOCKS:
            raise ValueError(f'inverted_residual needs {N_BLOCKS} entries, got {len(ir)}')
        kw['inverted_residual'] = tuple(ir)
    bw = BitWidths(**kw)
    check_bit_width(bw)
    return bw


def check_bit_width(path_or_dict_or_widths) -> BitWidths:
    """Validate a bit-width configuration for the int8 path: every width 3..8 (-> the parsed ``BitWidths``)."""
    bw = path_or_dict_or_widths
    if not isinstance(bw, BitWidths):
        return parse_bit_width(bw)
    bad = sorted({v for v in bw.all_widths() if not (3 <= int(v) <= 8)})
    if bad:
        raise NotImplementedError(f'bit widths {bad}: the int8 MFMA path holds 3..8-bit quantizers (1 and 2 bits '
                                  f'are Brevitas binary / ternary quantizers, quantizers.py:78-96)')
    return bw


def uint_levels(bits: int) -> int:
    """Top code of an unsigned b-bit quantizer."""
    return (1 << bits) - 1


def int_levels(bits: int) -> int:
    """Top code of a signed b-bit quantizer (the scale unit of the signed activation quantizers)."""
    return (1 << (bits - 1)) - 1


def _bn(sd, p, x):
    t = lambda n: torch.as_tensor(np.asarray(sd[f'{p}.1.{n}']), dtype=torch.float32)
    return F.batch_norm(x, t('running_mean'), t('running_var'), t('weight'), t('bias'), False, 0.1, 1e-5)


def _cbn(sd, p, x, stride, groups):
    w = torch.as_tensor(np.asarray(sd[f'{p}.0.weight']), dtype=torch.float32)
    k = w.shape[-1]
    return _bn(sd, p, F.conv2d(x, w, None, stride, (k - 1) // 2, 1, groups))


def _mse_clip(v: np.ndarray, levels: int, signed: bool) -> float:
    """The clip value c minimising the mean squared quantisation error of the values ``v`` for a quantizer with
    ``levels`` top code (scale c / levels; signed: codes down to -levels - 1), searched over c = f max|v|."""
    a = np.abs(v).max()
    if a <= 0:
        return 1e-8
    lo = -levels - 1 if signed else 0
    best, best_c = np.inf, a
    for f in np.linspace(0.05, 1.0, 96):
        sc = f * a / levels
        e = np.mean((np.clip(np.rint(v / sc), lo, levels) * sc - v) ** 2)
        if e < best:
            best, best_c = e, f * a
    return float(best_c)


def tap_ids(n_blocks: int = N_BLOCKS) -> Dict[str, int]:
    """Quantizer name -> observer tap id (include/spef.h): 0 image, 1 stem, 2 + 3 (i - 1) + {0, 1, 2} = quant /
    expand / dw of block i (1-based), then final and last."""
    ids = {'image': 0, 'stem': 1, 'final': 2 + 3 * n_blocks, 'last': 3 + 3 * n_blocks}
    for i in range(1, n_blocks + 1):
        for k, part in enumerate(('quant', 'expand', 'dw')):
            ids[f'blocks.{i}.{part}'] = 2 + 3 * (i - 1) + k
    return ids


def _quantizer(bw: BitWidths, name: str) -> Tuple[int, bool]:
    """-> (top code, signed) of the quantizer behind the tap ``name``."""
    if name == 'image':
        return int_levels(bw.image), True
    if name == 'stem':
        return uint_levels(bw.first_conv[1]), False
    if name == 'final':
        return int_levels(bw.shared_act), True
    if name == 'last':
        return uint_levels(bw.last_conv[1]), False
    _, i, part = name.split('.')
    if part == 'quant':
        return int_levels(bw.shared_act), True
    return uint_levels(bw.block(int(i) - 1)[1 if part == 'expand' else 3]), False


@torch.no_grad()
def taps(sd: Dict, frames_u8: np.ndarray, residual: bool = True):
    """The quantizer inputs of the float model on ``frames_u8`` (B x H x W x 3 uint8): yields ``(tap id, name,
    [float32 tensors])`` per quantizer in the reference graph's order -- image, stem, then per block expand (t != 1),
    dw and quant (blocks >= 2: the block input and, for a residual block, the project output before the add), final,
    last. These are the tensors ``calibrate`` takes its statistics from and the device observers see (spef_observe)."""
    ids = tap_ids()
    x = torch.from_numpy(frames_u8).permute(0, 3, 1, 2).float() / 255.0
    yield ids['image'], 'image', [x]
    x = F.relu(_cbn(sd, f'{FP}.0', x, 2, 1))
    yield ids['stem'], 'stem', [x]
    cin, idx = 32, 1
    for t, c, n, s in IR_SETTINGS:
        for i in range(n):
            stride = s if i == 0 else 1
            res = stride == 1 and cin == c and residual
            y, j = x, 0
            if t != 1:
                y = F.relu(_cbn(sd, f'{FP}.{idx}.conv.0', y, 1, 1))
                yield ids[f'blocks.{idx}.expand'], f'blocks.{idx}.expand', [y]
                j = 1
            y = F.relu(_cbn(sd, f'{FP}.{idx}.conv.{j}', y, stride, y.shape[1]))
            yield ids[f'blocks.{idx}.dw'], f'blocks.{idx}.dw', [y]
            y = _cbn(sd, f'{FP}.{idx}.conv.{j + 1}', y, 1, 1)
            if idx > 1:
                yield ids[f'blocks.{idx}.quant'], f'blocks.{idx}.quant', [x, y] if res else [x]
            x = x + y if res else y
            cin, idx = c, idx + 1
    yield ids['final'], 'final', [x]
    x = F.relu(_cbn(sd, f'{FP}.{idx}', x, 1, 1))
    yield ids['last'], 'last', [x]


def _qp_from_clips(clip, bw: BitWidths) -> Dict:
    """``clip``: quantizer name -> clip value (missing: the quantizer does not exist) -> the ``qp`` dict."""
    def scale(name):
        return None if name not in clip else clip[name] / _quantizer(bw, name)[0]
    qp: Dict = {'image': scale('image'), 'blocks': [], 'stem': scale('stem')}
    for i in range(1, N_BLOCKS + 1):
        qp['blocks'].append({'quant': scale(f'blocks.{i}.quant'), 'expand': scale(f'blocks.{i}.expand'),
                             'dw': scale(f'blocks.{i}.dw')})
    qp['final'] = scale('final')
    qp['last'] = scale('last')
    qp['bits'] = bw
    return qp


def calibrate(sd: Dict, frames_u8: np.ndarray, percentile: float = 99.999, residual: bool = True,
              bw: Optional[BitWidths] = None, method: str = 'percentile') -> Dict:
    """Activation scales from the float model's statistics on ``frames_u8`` (B x H x W x 3 uint8), one per
    quantizer (per tensor, as Brevitas), over the top code of its bit width (``bw``, default all 8):
    ``method='percentile'`` clips at the ``percentile`` of |x|; ``'mse'`` picks the clip that minimises the
    quantisation MSE of the observed values (a common PTQ initialisation; QAT refines the scales further).
    Runs on the host over the raw activations (``taps``); ``calibrate_device`` is the streamed device form."""
    bw = bw or BitWidths()
    assert method in ('percentile', 'mse')
    rng = np.random.default_rng(0)
    clip = {}
    for _, name, ts in taps(sd, frames_u8, residual):
        levels, signed = _quantizer(bw, name)
        v = torch.cat([t.flatten() for t in ts]).numpy().astype(np.float64)
        if method == 'mse':
            if v.size > 1 << 20:
                v = rng.choice(v, 1 << 20, replace=False)
            clip[name] = _mse_clip(v, levels, signed)
        else:
            clip[name] = float(max(np.percentile(np.abs(v), percentile), 1e-8))
    return _qp_from_clips(clip, bw)


# ---------------------------------------------------------------------------------------------- histogram observers
# The statistic the device observers keep (csrc/k_observe.hip, include/spef.h): a histogram of |x| keyed by the
# float32 bit pattern b = bits(|x|), 32 binades x 256 sub-bins from 2^-24 up to 2^8, plus exact counters.
OBS_BINS = 8192
OBS_COUNTERS = 8
N_TOTAL, N_UNDER, N_OVER, N_NONFINITE, MAX_BITS = range(5)   # the counters of a tap's record
_OBS_LO = 103 << 23   # bits(2^-24)
_OBS_HI = 135 << 23   # bits(2^8)


def observe_host(tensors):
    """The NumPy twin of the observer kernel: ``tensors`` (one float32 array / tensor or several) -> (counters
    uint64 [8], hist uint64 [8192]). Non-finite values count in n_nonfinite only; |x| < 2^-24 (zeros, denormals) in
    n_under; |x| >= 2^8 in n_over; everything else in bin ``(b - (103 << 23)) >> 15``; max_bits is the max of b over
    the finite values."""
    if isinstance(tensors, (np.ndarray, torch.Tensor)):
        tensors = [tensors]
    counters = np.zeros(OBS_COUNTERS, np.uint64)
    hist = np.zeros(OBS_BINS, np.uint64)
    for t in tensors:
        a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        assert a.dtype == np.float32, 'the observers see float32 values'
        b = np.ascontiguousarray(a).reshape(-1).view(np.uint32) & np.uint32(0x7fffffff)
        finite = b < np.uint32(0x7f800000)
        fb = b[finite]
        binned = fb[(fb >= _OBS_LO) & (fb < _OBS_HI)]
        counters[N_TOTAL] += np.uint64(b.size)
        counters[N_UNDER] += np.uint64(np.count_nonzero(fb < _OBS_LO))
        counters[N_OVER] += np.uint64(np.count_nonzero(fb >= _OBS_HI))
        counters[N_NONFINITE] += np.uint64(b.size - fb.size)
        if fb.size:
            counters[MAX_BITS] = max(counters[MAX_BITS], np.uint64(fb.max()))
        hist += np.bincount((binned - np.uint32(_OBS_LO)) >> np.uint32(15), minlength=OBS_BINS).astype(np.uint64)
    return counters, hist


def bin_edges() -> np.ndarray:
    """float32 [8193]: edge k is the lower edge of bin k and the (exclusive) upper edge of bin k - 1."""
    return ((np.arange(OBS_BINS + 1, dtype=np.uint32) << np.uint32(15)) + np.uint32(_OBS_LO)).view(np.float32)


def _bits_to_float(b) -> float:
    return float(np.array([int(b)], np.uint32).view(np.float32)[0])


def _hist_percentile(counters, hist, percentile: float) -> float:
    """The upper edge of the bin holding the order statistic of rank ceil(p / 100 (n - 1)) of the finite |x|, capped
    at the tap's max: at least the exact order statistic and at most (1 + 2^-8) times it. 0 when the rank falls in
    the underflow, the max when it falls in the overflow."""
    n_fin = int(counters[N_TOTAL]) - int(counters[N_NONFINITE])
    if n_fin <= 0:
        return 0.0
    mx = _bits_to_float(counters[MAX_BITS])
    r = int(np.ceil(percentile / 100.0 * (n_fin - 1)))
    r -= int(counters[N_UNDER])
    if r < 0:
        return 0.0
    cum = np.cumsum(hist.astype(np.uint64))
    k = int(np.searchsorted(cum, np.uint64(r), side='right'))   # first bin whose cumulative count exceeds r
    if k >= OBS_BINS:
        return mx
    return min(float(bin_edges()[k + 1]), mx)


def _hist_mse_clip(counters, hist, levels: int) -> float:
    """``_mse_clip`` over the histogram: the same grid of clips f max|x|, the error evaluated at the bin midpoints
    (capped at the max) weighted by the counts, the underflow counted as 0 and the overflow as the max. The histogram
    holds |x|, so a signed quantizer is searched over its positive codes [0, levels]."""
    n_fin = int(counters[N_TOTAL]) - int(counters[N_NONFINITE])
    a = _bits_to_float(counters[MAX_BITS])
    if n_fin <= 0 or a <= 0:
        return 1e-8
    e = bin_edges().astype(np.float64)
    nz = np.nonzero(hist)[0]
    v = np.minimum(0.5 * (e[nz] + e[nz + 1]), a)
    w = hist[nz].astype(np.float64)
    if int(counters[N_OVER]):
        v, w = np.append(v, a), np.append(w, float(counters[N_OVER]))
    best, best_c = np.inf, a
    for f in np.linspace(0.05, 1.0, 96):
        sc = f * a / levels
        err = float(np.sum(w * (np.clip(np.rint(v / sc), 0, levels) * sc - v) ** 2)) / n_fin
        if err < best:
            best, best_c = err, f * a
    return float(best_c)


def scales_from_stats(counters: np.ndarray, hist: np.ndarray, bw: Optional[BitWidths] = None,
                      method: str = 'percentile', percentile: float = 99.999, residual: bool = True) -> Dict:
    """Observer statistics (``counters`` [taps x 8], ``hist`` [taps x 8192]: ``ActivationObserver.read`` or
    ``observe_host`` per tap) -> the ``qp`` dict ``calibrate`` returns. Host fp64 over the integer counts.
    ``method``: 'max' (the tap's max), 'percentile' (``_hist_percentile``, floored at 1e-8) or 'mse'
    (``_hist_mse_clip``)."""
    bw = bw or BitWidths()
    assert method in ('max', 'percentile', 'mse')
    counters, hist = np.asarray(counters, np.uint64), np.asarray(hist, np.uint64)
    ids = tap_ids()
    assert counters.shape == (len(ids), OBS_COUNTERS) and hist.shape == (len(ids), OBS_BINS), 'one record per tap'
    arch = mobilenet_v2(residual=residual)
    clip = {}
    for name, t in ids.items():
        if '.' in name:
            i, part = int(name.split('.')[1]), name.split('.')[2]
            if (part == 'quant' and i == 1) or (part == 'expand' and arch.blocks[i - 1].expand == 1):
                continue
        c, h = counters[t], hist[t]
        if method == 'max':
            v = _bits_to_float(c[MAX_BITS])
        elif method == 'percentile':
            v = _hist_percentile(c, h, percentile)
        else:
            v = _hist_mse_clip(c, h, _quantizer(bw, name)[0])
        clip[name] = float(max(v, 1e-8))
    return _qp_from_clips(clip, bw)


def calibrate_device(sd: Dict, frames, device=0, batch: int = 16, bw: Optional[BitWidths] = None,
                     method: str = 'percentile', percentile: float = 99.999, residual: bool = True) -> Dict:
    """``calibrate`` on the device: the exact fp32 schedule (one kernel per conv) runs over the frames with a
    histogram observer behind every quantizer input, and the scales come from the integer counts
    (``scales_from_stats``). ``frames``: a uint8 array [N x H x W x 3], cut into batches of ``batch``, or an iterable
    of such batches (arrays or tensors of one frame size); they are streamed through the observers on a side stream
    and the statistics are read once at the end, so any number of frames costs one record per quantizer."""
    from . import blob as Bl
    from .arch import arch_from_state_dict
    from .engine import Engine
    if not torch.cuda.is_available():
        raise RuntimeError('calibrate_device needs a HIP device (quant.calibrate is the host path)')
    dev = torch.device(device if not isinstance(device, int) else f'cuda:{device}')
    if isinstance(frames, np.ndarray):
        assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[3] == 3, 'N x H x W x 3 uint8 frames'
        frames = [frames[i:i + batch] for i in range(0, frames.shape[0], batch)]   # views
    eng = Engine(Bl.pack(sd, arch_from_state_dict(sd, residual=residual), dtype='fp32'), dev)
    obs = None
    try:
        obs = eng.observer()
        stream = torch.cuda.Stream(dev)
        stream.wait_stream(torch.cuda.current_stream(dev))   # device batches made on the caller's stream
        with torch.cuda.stream(stream):
            for fr in frames:
                x = fr if isinstance(fr, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(fr))
                x = x.to(dev, non_blocking=True).contiguous()
                obs.observe(x)
            counters, hist = obs.read()
    finally:
        if obs is not None:
            obs.close()
        eng.close()
    return scales_from_stats(counters, hist, bw, method, percentile, residual)


def validate(qp: Dict, residual: bool = True) -> None:
    arch = mobilenet_v2(residual=residual)
    assert len(qp['blocks']) == len(arch.blocks), 'one entry per inverted residual'
    for i, (b, blk) in enumerate(zip(qp['blocks'], arch.blocks)):
        assert (b['quant'] is None) == (i == 0), 'block 1 has no shared quantizer (mobilenet_v2.py:189-197)'
        assert (b['expand'] is None) == (blk.expand == 1)
    for k in ('image', 'stem', 'final', 'last'):
        assert qp[k] > 0
    if qp.get('bits') is not None:
        check_bit_width(qp['bits'])
