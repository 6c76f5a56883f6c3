"""CPU: what the odd-frame GPU tests (tests/test_gpu_odd_frames.py) can see -- the oracle only, no kernel.

The stem (3x3, stride 2, pad 1) reads its bottom row / right column of zero padding only when the frame's H / W is
odd, and block 2's depthwise (the same geometry on the stem map) only when the stem map's is. Here one of those four
padding sides is made wrong in the oracle (the last real row / column replicated into it, oracle/block_ref.py) and the
change is measured where the GPU tests look: at op 1 for the stem, at op 2 for block 2's depthwise, as max |d| over
the map's max, on the GPU tests' own frames. It must be large where the geometry reaches the side (so a kernel with
that fault cannot pass a 5e-2 bound, let alone the schedules' own), every side must be reached by some shape, and at
the even shapes the suite used before the change is exactly zero: those shapes could not see it.
"""
import pytest
import torch

from oracle import model_ref as M
from oracle.block_ref import FAULTS, ODD_FRAME_SHAPES, blob_frames, odd_frames, oracle_block, reachable_sides
from spef_amd.arch import mobilenet_v2
from spef_amd.weights import synthetic_state_dict

FLOOR = 0.25   # of the map's max; measured 0.266 .. 0.69 on odd_frames (printed by the `effects` fixture)
EVEN_SHAPES = ((1, 100, 136), (2, 96, 128))   # the most ragged and the most used frame size of the earlier tests
CONVS = ('stem', 'dw2')


@pytest.fixture(scope='module')
def sd():
    return synthetic_state_dict(mobilenet_v2('ursonet', 1728, 3), seed=1001)


def _seen(x, sd, conv, fault):
    """The map the GPU tests compare for ``conv``: op 1 (stem fault) or op 2 (block 2 depthwise fault)."""
    with torch.no_grad():
        if conv == 'stem':
            return oracle_block(oracle_block(x, sd, 0, fault=fault), sd, 1)
        return oracle_block(M.backbone(x, sd, upto=1), sd, 2, fault=fault)


@pytest.fixture(scope='module')
def effects(sd):
    """{(b, h, w): {(conv, side): max |faulted - correct| / max |correct|}}, computed once."""
    out = {}
    for b, h, w in ODD_FRAME_SHAPES + EVEN_SHAPES:
        x = M.u8_nhwc_to_nchw_f32(odd_frames(b, h, w) if (b, h, w) in ODD_FRAME_SHAPES else blob_frames(b, h, w, 5 + h))
        eff = {}
        for conv in CONVS:
            good = _seen(x, sd, conv, 'none')   # the same conv call as the faulted run: only the padding differs
            for side in FAULTS:
                bad = _seen(x, sd, conv, side)
                eff[(conv, side)] = float((bad - good).abs().max() / good.abs().max())
        out[(b, h, w)] = eff
        print((b, h, w), {f'{c}/{s}': f'{v:.3f}' for (c, s), v in eff.items()})
    return out


def test_written_out_padding_is_the_oracles_conv(sd):
    """The conv with the padding applied by hand (no fault) is the oracle's conv, so a planted fault is the only
    difference between the two maps that are compared."""
    x = M.u8_nhwc_to_nchw_f32(blob_frames(2, 33, 35, 5 + 33))
    with torch.no_grad():
        from oracle.block_ref import conv_bn_act
        a = conv_bn_act(x, sd, 'features.features.0', 2, 1, True)
        ref = M.backbone(x, sd, upto=0)
        assert a.shape == ref.shape == (2, 32, 17, 18)
        assert float((a - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
        assert torch.equal(_seen(x, sd, 'dw2', None), M.backbone(x, sd, upto=2))


@pytest.mark.parametrize('b,h,w', ODD_FRAME_SHAPES)
def test_reachable_padding_faults_change_the_map(effects, b, h, w):
    """(a) every side the geometry reaches changes the compared map by at least FLOOR of its max; a side it does not
    reach changes nothing at all."""
    reach = reachable_sides(h, w)
    for key, v in effects[(b, h, w)].items():
        if key in reach:
            assert v >= FLOOR, ((b, h, w), key, v)
        else:
            assert v == 0.0, ((b, h, w), key, v)


def test_every_padding_side_is_reached(effects):
    """(b) across the shape list both sides of both convs are reached -- by geometry and by effect."""
    for conv in CONVS:
        for side in FAULTS:
            hit = [s for s in ODD_FRAME_SHAPES if (conv, side) in reachable_sides(s[1], s[2])]
            assert hit, (conv, side)
            assert max(effects[s][(conv, side)] for s in hit) >= FLOOR, (conv, side)


def test_expected_reachability_table():
    """The geometry, written out: which shape reaches what (the list the GPU module's coverage rests on)."""
    want = {(98, 134): {('dw2', 'bottom'), ('dw2', 'right')},
            (99, 135): {('stem', 'bottom'), ('stem', 'right')},
            (101, 137): {('stem', 'bottom'), ('stem', 'right'), ('dw2', 'bottom'), ('dw2', 'right')},
            (33, 35): {('stem', 'bottom'), ('stem', 'right'), ('dw2', 'bottom')},
            (37, 50): {('stem', 'bottom'), ('dw2', 'bottom'), ('dw2', 'right')},
            (32, 205): {('stem', 'right'), ('dw2', 'right')},
            (32, 32): set()}
    assert {(h, w) for _, h, w in ODD_FRAME_SHAPES} == set(want)
    for (h, w), sides in want.items():
        assert reachable_sides(h, w) == sides, (h, w)


@pytest.mark.parametrize('b,h,w', EVEN_SHAPES)
def test_even_shapes_cannot_see_padding_faults(effects, b, h, w):
    """(c) at 100 x 136 and 96 x 128 no conv reads its bottom or right padding: the change is exactly 0."""
    assert reachable_sides(h, w) == set()
    assert all(v == 0.0 for v in effects[(b, h, w)].values()), effects[(b, h, w)]
