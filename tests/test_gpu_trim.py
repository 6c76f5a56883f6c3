"""GPU: SPEF_OPT_TRIM (csrc/spef_tuning.hpp) -- kernels that drop work the result does not need must compute exactly
what the kernels they replace compute. Every comparison is np.array_equal between option 0 (the earlier kernels) and
the library default, on the same engine and the same frames.

Bit 0, the last conv's 128-pixel x 320-channel staged tile (k_x2_pw.hip x2_pws_kernel<POOL, X2PwsWide>): the pool form
through Engine.forward at M = 192 (a ragged last tile: 64 of its 128 pixels exist), at HW = 192 (128-pixel tiles straddle
two images) and at HW = 256; the non-pool form through a keypoint-head blob at 240 x 384 (HW = 96, M = 288: the last
tile has 32 pixels).
"""
import os

import numpy as np
import pytest
import torch

from spef_amd import _lib as L
from spef_amd import blob as Bl
from spef_amd.arch import mobilenet_v2
from spef_amd.data.synthetic import synth_frames
from spef_amd.weights import plant_keypoint_head, synthetic_state_dict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def engines():
    from spef_amd.engine import Engine
    sd = synthetic_state_dict(mobilenet_v2('ursonet', 1728, 3), seed=1001)
    es = {dt: Engine(Bl.pack(sd, dtype=dt), 'cuda:0') for dt in ('fp16mx', 'fp16x2')}
    yield es
    for e in es.values():
        e.close()


def _both(eng, run):
    """run() with SPEF_OPT_TRIM = 0, then with the library default (restored whatever happens)."""
    default = 1
    try:
        eng.set_option(L.OPT_TRIM, 0)
        base = run()
    finally:
        eng.set_option(L.OPT_TRIM, default)
    return base, run()


@pytest.mark.parametrize('dtype', ['fp16mx', 'fp16x2'])
@pytest.mark.parametrize('b,h,w', [(3, 256, 256), (3, 384, 512), (1, 512, 512)])
def test_last_conv_pool_bit_identical(engines, dtype, b, h, w):
    eng = engines[dtype]
    x = torch.from_numpy(synth_frames(b, h, w, 300 + h)).cuda()

    def run():
        return [t.cpu().numpy() for t in eng.forward(x)]
    (o0, p0), (o1, p1) = _both(eng, run)
    assert np.isfinite(o1).all() and np.abs(o1).max() > 0
    assert np.array_equal(o0, o1), float(np.abs(o0 - o1).max())
    assert np.array_equal(p0, p1), float(np.abs(p0 - p1).max())


def test_last_conv_map_bit_identical():
    """The non-pool form: the keypoint head reads the full 1280-channel map (weights as bench.py's run_keypoint)."""
    from spef_amd.engine import Engine
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'keypoints.npz'))
    arch = mobilenet_v2('keypoints')
    ip = int(np.argmin(np.abs(g['t'][:, 2] - np.median(g['t'][:, 2]))))
    sd = plant_keypoint_head(synthetic_state_dict(arch, seed=1001, head_std=2e-4), g['kp2d'][ip])
    eng = Engine(Bl.pack(sd, arch, dtype='fp16x2'), 'cuda:0')
    try:
        x = torch.from_numpy(synth_frames(3, 240, 384, 20_000)).cuda()
        r0, r1 = _both(eng, lambda: eng.forward(x)[0].cpu().numpy())
    finally:
        eng.close()
    assert np.isfinite(r1).all() and np.abs(r1).max() > 0
    assert np.array_equal(r0, r1), float(np.abs(r0 - r1).max())

