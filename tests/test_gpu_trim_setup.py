"""GPU: SPEF_OPT_TRIM bit 1 (csrc/spef_tuning.hpp) -- the lean tile set-up of k_mx.hip's mx_irb_kernel (fp16mx blocks
2-4: scalar image bases, 32-bit per-lane offsets, incremental tile pixels, interior workgroups without bounds checks)
must compute exactly what the kernels with 64-bit per-pixel addresses compute. Every comparison is np.array_equal
between option 1 (the earlier block kernels) and the library default, on one engine and the same frames: the head
outputs of Engine.forward and the block outputs of blocks 1-7 through Engine.probe.

Shapes, the smallest at which each path can go wrong:
  (2, 192, 384)  the smallest frame with an interior workgroup in blocks 2, 3 and 4 (3 x 3 tiles of 8 x 16, 16 x 16 and
                 8 x 16 at H/4, H/4 and H/8), with tiles on all four edges;
  (3, 101, 137), (2, 100, 136)  odd maps, ragged last tiles, the bottom / right padding that test_edge_sensitivity.py
                 shows is reached; B = 3 checks the image index;
  (2, 32, 32)    maps smaller than one tile: every pixel tile is partly padding;
  (2, 64, 208)   W/4 is no multiple of 16 and the map is one tile high.
Bits 2 (x2_irb_kernel) and 3 (front_mx_kernel) of the option are not built, so the fp16x2 schedule runs no changed
kernel and has no case here.

The 32-bit offsets: at every size of this suite each launch takes the lean kernels; a map beyond the launcher's bound
(csrc/k_mx.hip mx_irb_lean_fits: an image's input or output map of 2^31 bytes or more, or an input row pitch or height
of 2^24 or more) runs the earlier kernel under the profile key mx_irb_kernel_wide<...>, which must not appear.
"""
import numpy as np
import pytest
import torch

from oracle.block_ref import odd_frames
from spef_amd import _lib as L
from spef_amd import blob as Bl
from spef_amd.arch import mobilenet_v2
from spef_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

SHAPES = [(2, 192, 384), (3, 101, 137), (2, 100, 136), (2, 32, 32), (2, 64, 208)]
BLOCK_OPS = range(1, 8)   # probe stop_op of blocks 1-7 (op 0 is the stem)


@pytest.fixture(scope='module')
def mx():
    from spef_amd.engine import Engine
    sd = synthetic_state_dict(mobilenet_v2('ursonet', 1728, 3), seed=1001)
    eng = Engine(Bl.pack(sd, dtype='fp16mx'), 'cuda:0')
    yield eng
    eng.close()


def _both(eng, run):
    """run() with the library default (a fresh engine's), then with SPEF_OPT_TRIM = 1: bit 0 alone, the early kernels
    as they were (the default restored whatever happens)."""
    new = run()
    try:
        eng.set_option(L.OPT_TRIM, 1)
        old = run()
    finally:
        eng.set_option(L.OPT_TRIM, L.OPT_TRIM_DEFAULT)
    return old, new


@pytest.mark.parametrize('b,h,w', SHAPES)
def test_heads_and_blocks_bit_identical(mx, b, h, w):
    x = torch.from_numpy(odd_frames(b, h, w)).cuda()

    def run():
        outs = [t.cpu().numpy() for t in mx.forward(x)]
        return outs + [mx.probe(x, op).cpu().numpy() for op in BLOCK_OPS]
    old, new = _both(mx, run)
    for i, (o, n) in enumerate(zip(old, new)):
        name = ('logits', 'position')[i] if i < 2 else f'block {BLOCK_OPS[i - 2]}'
        assert np.isfinite(n).all() and np.abs(n).max() > 0, name
        assert o.shape == n.shape and np.array_equal(o, n), (name, float(np.abs(o - n).max()))


@pytest.mark.parametrize('b,h,w', SHAPES)
def test_every_launch_takes_the_lean_kernels(mx, b, h, w):
    x = torch.from_numpy(odd_frames(b, h, w)).cuda()
    mx.forward(x)
    torch.cuda.synchronize()
    mx.profile_begin()
    mx.forward(x)
    keys = set(mx.profile_end())
    assert {'mx_irb_kernel<16,96,24,s2>', 'mx_irb_kernel<24,144,24,s1>', 'mx_irb_kernel<24,144,32,s2>'} <= keys, keys
    assert not [k for k in keys if k.startswith('mx_irb_kernel_wide')], keys
