"""GPU: SPEF_OPT_X2_STAGE (csrc/spef_tuning.hpp) -- the persistent role-split rows of the fp16x2 / fp16mx schedules
(blocks 8-10 and 14) on x2_irw_st_kernel (1, the default: every chunk stage by LDS-DMA into static double buffers, kept
in flight across the chunk barrier) against x2_irw_kernel (0). The arithmetic is the same in the same order, so every
comparison is np.array_equal between the two option values, on one engine per schedule and the same frames: the
forward's outputs and the outputs of blocks 8-14 (Engine.probe; blocks 11-13 run the three-stage kernel on what blocks
8-10 wrote).

Shapes, the smallest at which each path of the new pipeline runs (CUs from the device; a 100 x 136 frame gives blocks
8-13 a 7 x 9 map, one ragged 8 x 16 tile):
  (2, 100, 136), (3, 101, 137)  fewer tiles than CUs: every workgroup runs one tile -- prologue, steady state and
                                drain with no tile transition; B = 3 checks the image index
  (2, 32, 32)                   maps smaller than a tile: most expand pixel tiles are padding
  (CUs + 1, 100, 136)           persistent tiles with an uneven split: the last workgroup has a single tile
  (2 CUs + 1, 100, 136)         three tiles in one workgroup: a parity or release error that shows only at the
                                second transition
  (2, 192, 384)                 several tiles per image, interior and edge; block 14's stride-2 tiles on all four edges
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from launch_plan_cases import compute_units  # noqa: E402
from oracle.block_ref import odd_frames
from spef_amd import _lib as L
from spef_amd import blob as Bl
from spef_amd.arch import mobilenet_v2
from spef_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

KEYS = ('x2_irw_kernel<64,384,64,s1>', 'x2_irw_kernel<96,576,160,s2>')
SHAPES = [(2, 100, 136), (3, 101, 137), (2, 32, 32), ('cu+1', 100, 136), ('2cu+1', 100, 136), (2, 192, 384)]


@pytest.fixture(scope='module')
def engines():
    from spef_amd.engine import Engine
    sd = synthetic_state_dict(mobilenet_v2('ursonet', 1728, 3), seed=1001)
    es = {dt: Engine(Bl.pack(sd, dtype=dt), 'cuda:0') for dt in ('fp16mx', 'fp16x2')}
    yield es
    for e in es.values():
        e.close()


def _both(eng, run):
    """run() with SPEF_OPT_X2_STAGE = 0, then with the library default (restored whatever happens)."""
    try:
        eng.set_option(L.OPT_X2_STAGE, 0)
        base = run()
    finally:
        eng.set_option(L.OPT_X2_STAGE, L.OPT_X2_STAGE_DEFAULT)
    return base, run()


@pytest.mark.parametrize('dtype', ['fp16mx', 'fp16x2'])
@pytest.mark.parametrize('b,h,w', SHAPES, ids=lambda v: str(v))
def test_bit_identical_to_option_0(engines, dtype, b, h, w):
    eng = engines[dtype]
    cus = compute_units()
    b = {'cu+1': cus + 1, '2cu+1': 2 * cus + 1}.get(b, b)
    x = torch.from_numpy(odd_frames(b, h, w)).cuda()

    def run():
        maps = {f'out{i}': t.cpu().numpy() for i, t in enumerate(eng.forward(x))}
        maps.update({f'block{op}': eng.probe(x, op).cpu().numpy() for op in range(8, 15)})
        return maps
    old, new = _both(eng, run)
    assert sorted(old) == sorted(new) and len(new) == 9
    for k in new:
        assert np.isfinite(new[k]).all() and np.abs(new[k]).max() > 0, k
        assert old[k].shape == new[k].shape, k
        assert np.array_equal(old[k], new[k]), (k, float(np.abs(old[k] - new[k]).max()))


@pytest.mark.parametrize('dtype', ['fp16mx', 'fp16x2'])
def test_profile_keys_unchanged(engines, dtype):
    """Both option values launch under the plan's labels (tests/test_gpu_profile_labels.py pins them)."""
    eng = engines[dtype]
    x = torch.from_numpy(odd_frames(2, 100, 136)).cuda()

    def run():
        eng.profile_begin()
        eng.forward(x)
        return set(eng.profile_end())
    old, new = _both(eng, run)
    assert set(KEYS) <= new, sorted(new)
    assert old == new, sorted(old ^ new)


def test_option_range(engines):
    eng = engines['fp16x2']
    try:
        with pytest.raises(AssertionError):
            eng.set_option(L.OPT_X2_STAGE, 2)
    finally:
        eng.set_option(L.OPT_X2_STAGE, L.OPT_X2_STAGE_DEFAULT)
