"""Per-block pieces of the float32 oracle (ORACLE -- test infrastructure only), shared by the GPU tests that check
one kernel at a time and by the CPU test that shows what those tests can see:

  * ``oracle_block``    one ``features.features[idx]`` of oracle/model_ref.py on its own input, optionally with the
                        fp16mx schedule's fp16 hidden storage restated, optionally with a padding fault planted in
                        its 3x3 conv;
  * ``conv_bn_act``     model_ref._conv_bn_act with the padding written out, so that one side of it can be made wrong;
  * ``blob_frames``     the parity tests' frame generator (bright 4x4 blobs over noise, bright borders) at any size.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from . import model_ref as M

FAULTS = ('bottom', 'right')

# (b, h, w) of tests/test_gpu_odd_frames.py, with what each adds; tests/test_edge_sensitivity.py holds the list to
# reaching every padding side. b >= 2: a read past a row or an image lands in real pixels, not in allocation slack.
ODD_FRAME_SHAPES = (
    (2, 98, 134),    # W % 4 = 2; stem map 49 x 67 (odd x odd): block 2's bottom and right padding
    (2, 99, 135),    # W % 4 = 3; the stem's bottom and right padding
    (2, 101, 137),   # W % 4 = 1; stem map 51 x 69, level 2 26 x 35 (odd width), level 3 13 x 18
    (2, 33, 35),     # odd image byte count: image 1 starts on an odd address
    (3, 37, 50),     # stem map 19 x 25
    (2, 32, 205),    # 1 x 7 final map; 7 stem tiles per row
    (2, 32, 32),     # 1 x 1 final map
)


def reachable_sides(h, w):
    """Which padding sides a frame of h x w reads: {(conv, side)} with conv 'stem' (3x3 stride 2 on the frame) or
    'dw2' (block 2's depthwise, 3x3 stride 2 on the stem map). Pad 1, stride 2: the last output row's bottom tap is row
    2 ((n - 1) // 2) + 1 = n exactly when n is odd."""
    sh, sw = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out = set()
    for conv, (nh, nw) in (('stem', (h, w)), ('dw2', (sh, sw))):
        if nh % 2:
            out.add((conv, 'bottom'))
        if nw % 2:
            out.add((conv, 'right'))
    return out


def conv_bn_act(x, sd, prefix, stride, groups, act, fault=None):
    """model_ref._conv_bn_act with the zero padding applied by hand. ``fault`` = 'bottom' / 'right' replaces the bottom
    row / right column of the padding by the last real row / column (what a kernel that clamps its address, or reads
    one row or column too far into a tile with a replicated edge, would see) -- a 3x3 stride-2 conv reads that side
    only when the map's height / width is odd. None / 'none' = the correct conv."""
    w = M._t(sd, f'{prefix}.0.weight')
    p = (w.shape[-1] - 1) // 2
    xp = F.pad(x, (p, p, p, p))
    if fault == 'bottom':
        xp[:, :, -p:, :] = xp[:, :, -p - 1:-p, :]
    elif fault == 'right':
        xp[:, :, :, -p:] = xp[:, :, :, -p - 1:-p]
    elif fault not in (None, 'none'):
        raise ValueError(fault)
    y = F.conv2d(xp, w, None, stride, 0, 1, groups)
    y = F.batch_norm(y, M._t(sd, f'{prefix}.1.running_mean'), M._t(sd, f'{prefix}.1.running_var'),
                     M._t(sd, f'{prefix}.1.weight'), M._t(sd, f'{prefix}.1.bias'), False, 0.1, 1e-5)
    return F.relu(y) if act else y


def oracle_block(x, sd, idx, f16_hidden=(), fault=None):
    """features.features[idx] of the oracle (oracle/model_ref.py: the reference's float32 arithmetic, op for op) on
    the activation x (NCHW fp32); idx 0 = the stem. Blocks listed in ``f16_hidden`` round their expand output to fp16
    before the depthwise (the fp16mx schedule's hidden storage, csrc/k_mx.hip). ``fault`` plants a padding fault
    (``conv_bn_act``) in the block's 3x3 conv: the stem's, or the block's depthwise; 'none' runs that conv with the
    padding written out and no fault, the like-for-like baseline of a faulted run."""
    fp = 'features.features'
    if idx == 0:
        if fault is None:
            return M._conv_bn_act(x, sd, f'{fp}.0', 2, 1, True)
        return conv_bn_act(x, sd, f'{fp}.0', 2, 1, True, fault)
    cin, i = 32, 1
    for t, c, n, s in M._IR:
        for k in range(n):
            if i == idx:
                stride = s if k == 0 else 1
                y, j = x, 0
                if t != 1:
                    y = M._conv_bn_act(y, sd, f'{fp}.{idx}.conv.{j}', 1, 1, True)
                    if idx in f16_hidden:
                        y = y.half().float()
                    j += 1
                if fault is None:
                    y = M._conv_bn_act(y, sd, f'{fp}.{idx}.conv.{j}', stride, int(round(cin * t)), True)
                else:
                    y = conv_bn_act(y, sd, f'{fp}.{idx}.conv.{j}', stride, int(round(cin * t)), True, fault)
                y = M._conv_bn_act(y, sd, f'{fp}.{idx}.conv.{j + 1}', 1, 1, False)
                return x + y if (stride == 1 and cin == c) else y
            cin, i = c, i + 1
    raise ValueError(idx)


def blob_frames(b, h, w, seed):
    """uint8 NHWC grey frames: noise 0..39 plus a 4x4-blocked pattern 0..214. For h, w multiples of 4 this is the
    generator of test_gpu_parity.py / test_gpu_x2.py / test_gpu_mx.py (``_frames``), value for value; any other size is
    generated at h, w rounded up to 4 and cropped to [:h, :w], which keeps the statistics and keeps the border pixels
    as bright as the interior (a padding fault at the border changes the map; with a dark border it would not)."""
    hp, wp = (h + 3) // 4 * 4, (w + 3) // 4 * 4
    rng = np.random.Generator(np.random.PCG64(seed))
    base = rng.integers(0, 40, (b, hp, wp, 1), dtype=np.uint8)
    blob = rng.integers(0, 215, (b, hp // 4, wp // 4, 1), dtype=np.uint8).repeat(4, 1).repeat(4, 2)
    fr = np.repeat(np.clip(base.astype(np.int32) + blob, 0, 255).astype(np.uint8), 3, axis=3)
    return np.ascontiguousarray(fr[:, :h, :w])


def odd_frames(b, h, w):
    """The frames of tests/test_gpu_odd_frames.py and tests/test_edge_sensitivity.py for one of ODD_FRAME_SHAPES. How
    far a padding fault moves the map depends on what the border pixels hold: with these seeds every reachable fault
    moves it by at least 0.266 of its max (block 2's right padding at 101 x 137 is the smallest); seeds 5 + h give
    0.245 for block 2's right padding at 32 x 205, under the 0.25 floor that test_edge_sensitivity.py holds."""
    return blob_frames(b, h, w, 1000 * h + w)
