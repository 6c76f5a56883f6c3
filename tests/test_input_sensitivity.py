"""CPU: what the colour-frame GPU tests (tests/test_gpu_colour_frames.py) can see that no grey frame can -- the oracle
only, no kernel.

Every other frame of the suite replicates one grey plane into R, G and B, and with identical channels a 3 -> 32 stem
only sees sum_c w[:, c]: a stem that permutes its input channels, reads one plane three times, strides the planes of the
float32 NCHW layout wrongly or packs its operand in another channel order computes the same map. Here the six such
faults (tests/forward_inputs.py CHANNEL_FAULTS) are planted in the oracle's input and the change is measured where the
GPU tests look -- the maps after op 0 and op 1 and the head outputs: exactly nothing on ``blob_frames``, at least a
quarter of the map's max on ``colour_frames`` and on ``float_frames`` at every shape the GPU module uses, so a kernel
with one of these faults cannot pass the schedules' bounds there (the widest is 5e-2).
"""
import os
import sys

import pytest
import torch

from oracle import model_ref as M
from oracle.block_ref import blob_frames, oracle_block

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forward_inputs as FI  # noqa: E402

FLOOR = 0.25   # of the map's max, the floor of tests/test_edge_sensitivity.py; measured 0.52 .. 1.15 (printed below)
HEAD_FLOOR = 6e-3   # absolute: test_gpu_parity.py LOGIT_TOL_BF16, the widest head bound; measured 9.6e-3 .. 3.2e-2
SEED = 11      # tests/test_gpu_colour_frames.py uses the same frames: colour_frames(b, h, w, SEED + h)


@pytest.fixture(scope='module')
def sd():
    return FI.base_state_dict()


def _seen(x, sd):
    """What the GPU tests compare: the maps after op 0 and op 1, and the head outputs."""
    with torch.no_grad():
        m0 = oracle_block(x, sd, 0)
        m1 = oracle_block(m0, sd, 1)
        ori, pos = M.forward(x, sd)
    return {'op0': m0, 'op1': m1, 'ori': ori, 'pos': pos}


def _changes(x, sd):
    """{fault: {what: max |faulted - correct| / max |correct|}}"""
    good = _seen(x, sd)
    out = {}
    for fault in FI.CHANNEL_FAULTS:
        bad = _seen(FI.channel_fault(x, fault), sd)
        out[fault] = {k: float((bad[k] - good[k]).abs().max() / good[k].abs().max()) for k in good}
        out[fault]['head_abs'] = max(float((bad[k] - good[k]).abs().max()) for k in ('ori', 'pos'))
    return out


def test_the_six_faults_are_six_different_readings():
    x = FI.float_frames(1, 4, 4, 0)
    seen = [FI.channel_fault(x, f) for f in FI.CHANNEL_FAULTS]
    assert len(FI.CHANNEL_FAULTS) == 6
    for i, a in enumerate(seen):
        assert not torch.equal(a, x)
        for b in seen[i + 1:]:
            assert not torch.equal(a, b)


@pytest.mark.parametrize('b,h,w', FI.COLOUR_SHAPES)
def test_grey_frames_cannot_see_channel_faults(sd, b, h, w):
    """R = G = B: every fault leaves the op-0 and op-1 maps and the head outputs exactly as they were."""
    fr = blob_frames(b, h, w, SEED + h)
    assert (fr[..., 0] == fr[..., 1]).all() and (fr[..., 0] == fr[..., 2]).all()
    ch = _changes(M.u8_nhwc_to_nchw_f32(fr), sd)
    for fault, c in ch.items():
        assert all(v == 0.0 for v in c.values()), (fault, c)


@pytest.mark.parametrize('kind', ['colour_u8', 'float'])
@pytest.mark.parametrize('b,h,w', FI.COLOUR_SHAPES)
def test_colour_frames_see_every_channel_fault(sd, b, h, w, kind):
    """Independent channels: every fault moves the op-0 and the op-1 map by at least FLOOR of its max, and the head
    outputs by more than any head bound lets pass."""
    if kind == 'colour_u8':
        fr = FI.colour_frames(b, h, w, SEED + h)
        assert fr.shape == (b, h, w, 3) and fr.dtype.name == 'uint8'
        x = M.u8_nhwc_to_nchw_f32(fr)
    else:
        x = FI.float_frames(b, h, w, SEED + h)
    ch = _changes(x, sd)
    for fault, c in ch.items():
        print((b, h, w), kind, fault, {k: f'{v:.3g}' for k, v in c.items()})
    for fault, c in ch.items():
        assert c['op0'] >= FLOOR and c['op1'] >= FLOOR, (fault, c)
        # the mean-pooled head of the seed-1001 net (Linear std 0.01, outputs to 0.3) moves far less than a map does:
        # it is held to the widest absolute bound a GPU test puts on a head output (bf16, 6e-3), not to the maps' floor
        assert c['head_abs'] > HEAD_FLOOR, (fault, c)


def test_colour_frames_keep_bright_borders_and_independent_channels():
    """The generator itself: each plane is a blob_frames plane (so the borders are as bright as the interior and a
    padding fault still shows), and no two planes are correlated."""
    import numpy as np
    fr = FI.colour_frames(2, 33, 35, SEED + 33).astype(np.float64)
    border = np.concatenate([fr[:, 0].ravel(), fr[:, -1].ravel(), fr[:, :, 0].ravel(), fr[:, :, -1].ravel()])
    assert border.mean() > 0.8 * fr.mean()
    for a, b in ((0, 1), (0, 2), (1, 2)):
        r = np.corrcoef(fr[..., a].ravel(), fr[..., b].ravel())[0, 1]
        assert abs(r) < 0.1, (a, b, r)
    x = FI.float_frames(2, 33, 35, 3, -0.1, 1.1).numpy()
    assert x.min() < 0 and x.max() > 1 and x.shape == (2, 3, 33, 35)
    assert np.abs(x * 255 - np.rint(x * 255)).mean() > 0.2   # not on the uint8 grid
