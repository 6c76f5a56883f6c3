"""CPU: the rescaled weights of tests/test_gpu_channel_range.py, and the channel-scale range they may span -- the
oracle and a float64 restatement only, no kernel.

With the synthetic weights every stem, expand, depthwise and block output peaks between 2.5 and 10.1, so the fp16
storage points and the hi + lo fp16 operand splits have only ever seen one decade. ``rescaled_state_dict`` scales every
internal channel by its own power of two at its BatchNorm and unscales it at its one consumer, the freedom a trained
checkpoint has. Checked here:

  * the oracle computes the same function on the rescaled weights (the GPU tests' references stay what they were);
  * the rescaled net's channel maxima really moved by the drawn 2^k, both ends of the range are drawn, nothing is near
    65504 and no tensor an fp16 storage point holds sinks into the fp16 subnormal range;
  * the held range [KMIN, KMAX] = [-6, 6] is the widest in which each schedule's arithmetic, restated in float64
    (tests/forward_inputs.py ``Restated``), stays within a quarter of that schedule's existing block bound on every
    block. The hi + lo split is what limits it: lo = fp16(v - hi) is exact to 2^-22 |v| only while it is a normal
    fp16; below 2^-14 it is kept to an absolute 2^-25. Small activations (k < 0) lose their lo half that way, and so do
    the consumer's weights, divided by 2^k, for k > 0;
  * the stem's channels cannot be scaled down at all (STEM_KMIN = 0): the fused front kernels' stem operand carries
    ToTensor's / 255 and is the operand nearest the fp16 subnormal floor on the unscaled weights already.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import model_ref as M
from oracle.block_ref import oracle_block
from spef_amd.arch import mobilenet_v2
from spef_amd.quant import taps

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forward_inputs as FI  # noqa: E402

F16_MAX, F16_MIN_NORMAL = 65504.0, 2.0 ** -14
# the rescaled tensors that fp16mx stores in fp16 and whose rounding the restatement leaves out of both sides (the fp16
# schedule's storage roundings are all in its restatement)
MX_F16_STORED = ('stem',) + tuple(f'blocks.{i}.expand' for i in FI.MX_F16_HIDDEN)


@pytest.fixture(scope='module')
def arch():
    return mobilenet_v2('ursonet', 1728, 3)


@pytest.fixture(scope='module')
def frames():
    b, h, w = FI.RANGE_SHAPE
    return FI.colour_frames(b, h, w, 11 + h)


def _outputs(sd, frames):
    """The oracle's block outputs (ops 1..17) and head outputs."""
    x = M.u8_nhwc_to_nchw_f32(frames)
    with torch.no_grad():
        y = oracle_block(x, sd, 0)
        outs = []
        for op in range(1, 18):
            y = oracle_block(y, sd, op)
            outs.append(y)
        outs.extend(M.forward(x, sd))
    return outs


def test_rescaling_preserves_the_function(frames):
    """Block outputs and head outputs of the oracle on the rescaled weights equal those on the base weights: powers of
    two move exponents only, so every float32 product and sum keeps its significand."""
    base = _outputs(FI.base_state_dict(), frames)
    resc = _outputs(FI.rescaled()[0], frames)
    worst, identical = 0.0, True
    for a, b in zip(base, resc):
        worst = max(worst, float((a - b).abs().max() / a.abs().max()))
        identical = identical and torch.equal(a, b)
    print(f'rescaled [{FI.KMIN}, {FI.KMAX}] vs base: max |d| / map max {worst:.2e}; bit-identical: {identical}')
    assert worst <= 1e-6


def test_channel_maxima_span_the_drawn_range(arch, frames):
    """Every scaled channel's maximum moved by exactly its drawn 2^k; both ends of the range are drawn in the stem
    ([STEM_KMIN, KMAX]), in the expand and in the depthwise family; the scaled tensors' channel maxima now span more
    than 2^(KMAX - KMIN)."""
    sd, ks = FI.rescaled()
    base = {name: ts[0] for _, name, ts in taps(FI.base_state_dict(), frames)}
    resc = {name: ts[0] for _, name, ts in taps(sd, frames)}
    families = {'stem': [], 'expand': [], 'dw': []}
    cmax = []
    names = {arch.stem.prefix: 'stem', arch.last.prefix: 'last'}
    for blk in arch.blocks:
        convs = list(blk.convs)
        if blk.expand != 1:
            names[convs.pop(0).prefix] = f'blocks.{blk.index}.expand'
        names[convs[0].prefix] = f'blocks.{blk.index}.dw'
    for prefix, k in ks.items():
        name = names[prefix]
        mb, mr = base[name].amax((0, 2, 3)).numpy(), resc[name].amax((0, 2, 3)).numpy()
        np.testing.assert_array_equal(mr, mb * np.exp2(k).astype(np.float32), err_msg=name)
        assert k.min() >= FI.KMIN and k.max() <= FI.KMAX
        fam = name.split('.')[-1]
        if fam in families:
            families[fam].append(k)
            cmax.append(mr[mr > 0])
    for fam, kk in families.items():
        kk = np.concatenate(kk)
        assert kk.min() == (FI.STEM_KMIN if fam == 'stem' else FI.KMIN) and kk.max() == FI.KMAX, fam
    cmax = np.concatenate(cmax)
    print(f'scaled channel maxima: {cmax.min():.3g} .. {cmax.max():.3g}')
    assert cmax.max() / cmax.min() > 2.0 ** (FI.KMAX - FI.KMIN)
    # block outputs (the residual stream) are left alone
    for i in range(2, 18):
        assert torch.equal(base[f'blocks.{i}.quant'], resc[f'blocks.{i}.quant'])


def test_nothing_near_the_ends_of_fp16(arch, frames):
    """No activation of the rescaled net, no folded weight and no hi half is non-finite or reaches 65504 (the largest
    is three binades below it), and every channel's peak in the tensors fp16mx stores in fp16 is at least 16 times the
    smallest normal fp16: values down to a sixteenth of a channel's peak keep all 11 bits when stored, and what lies
    below is kept to 2^-25 absolute, under 2^-15 of that peak -- those storage roundings act on the rescaled net as
    on the base net."""
    sd, _ = FI.rescaled()
    peak = 0.0
    for _, name, ts in taps(sd, frames):
        for t in ts:
            assert bool(torch.isfinite(t).all()), name
            peak = max(peak, float(t.abs().max()))
            if name in MX_F16_STORED:
                cm = t.abs().amax((0, 2, 3))
                assert float(cm[cm > 0].min()) > 16 * F16_MIN_NORMAL, name
    net = FI.Restated(sd, arch)
    wpeak = 0.0
    for prefix, (w, b) in net.w.items():
        assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(b).all()), prefix
        assert bool(torch.isfinite(w.to(torch.float16)).all()), prefix
        wpeak = max(wpeak, float(w.abs().max()), float(b.abs().max()))
    print(f'largest activation {peak:.4g}, largest folded weight or bias {wpeak:.4g}')
    assert peak < F16_MAX / 8 and wpeak < F16_MAX / 8


X2_LIKE = ('fp16x2', 'fp16mx', 'fp16mx_fallback')   # the hi + lo schedules
RANGES = {'held': (FI.KMIN, FI.KMAX, FI.STEM_KMIN), 'low half': (FI.KMIN, 0, FI.STEM_KMIN),
          'high half': (0, FI.KMAX, FI.STEM_KMIN), 'one lower': (FI.KMIN - 1, 0, FI.STEM_KMIN),
          'one higher': (0, FI.KMAX + 1, FI.STEM_KMIN), 'unscaled': (0, 0, 0)}


@pytest.fixture(scope='module')
def restated(arch, frames):
    """{range name: {schedule: {block: error / map max}}}, computed once: the held range, its two one-sided halves, the
    two one-sided ranges one step wider, and the unscaled weights."""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    out = {}
    for name, (kmin, kmax, stem) in RANGES.items():
        sd = FI.rescaled(kmin, kmax, FI.RANGE_SEED, stem)[0]
        out[name] = FI.restated_block_errors(sd, arch, frames)
        worst = {s: max(e.values()) for s, e in out[name].items()}
        share = {s: max(v / FI.schedule_bound(s, i) for i, v in e.items()) for s, e in out[name].items()}
        print(f'restated {name} [{kmin}, {kmax}], stem from {max(kmin, stem)}: max block error / map max',
              {s: f'{v:.2e}' for s, v in worst.items()}, 'block 1', {s: f'{e[1]:.2e}' for s, e in out[name].items()},
              'largest share of the bound', {s: f'{v:.3f}' for s, v in share.items()})
    return out


def _over(errs, schedule, first=1):
    return {b: e for b, e in errs[schedule].items()
            if b >= first and e > FI.RESTATED_SHARE * FI.schedule_bound(schedule, b)}


@pytest.mark.parametrize('schedule', FI.SCHEDULES)
def test_restated_arithmetic_keeps_a_quarter_of_the_bound(restated, schedule):
    """On the weights the GPU tests use -- channels drawn over [KMIN, KMAX], the stem's over [STEM_KMIN, KMAX] -- the
    schedule's arithmetic alone stays at or below a quarter of the existing bound of every block. Blocks 2-17, which no
    stem scale reaches (each is restated on its exact input), do so in each one-sided half as well, where every
    channel sits on that side."""
    assert not _over(restated['held'], schedule), (schedule, _over(restated['held'], schedule))
    for half in ('low half', 'high half'):
        assert not _over(restated[half], schedule, first=2), (half, schedule, _over(restated[half], schedule, 2))


@pytest.mark.parametrize('side', ['one lower', 'one higher'])
def test_the_range_is_the_widest(restated, side):
    """One step further on either side the hi + lo schedules exceed the quarter on some block past the front kernel:
    [KMIN, KMAX] is where the restatement puts the limit, not a cautious choice."""
    for schedule in X2_LIKE:
        assert _over(restated[side], schedule, first=2), (side, schedule)


def test_the_stem_cannot_be_scaled_down(restated):
    """Why the stem's channels draw from [STEM_KMIN, KMAX] = [0, KMAX]: on the unscaled weights block 1 of fp16x2
    through the fused front kernel (u8 frames, the / 255-folded stem operand split hi + lo) is over the quarter already
    -- and within the bound, as the existing tests find it. Blocks 2-17 are a hundredth of the bound there."""
    e = restated['unscaled']['fp16x2']
    print(f'unscaled weights, fp16x2: block 1 through the front kernel {e[1]:.2e}, blocks 2-17 up to '
          f'{max(v for b, v in e.items() if b > 1):.2e} of the map max')
    assert FI.RESTATED_SHARE * FI.X2_BLOCK_TOL < e[1] < FI.X2_BLOCK_TOL
    assert max(v for b, v in e.items() if b > 1) < 0.05 * FI.X2_BLOCK_TOL


def test_storage_roundings_cost_one_fp16_step_at_any_scale(arch, frames):
    """Why the restatement above leaves the fp16mx storage roundings out of both sides: with them in, blocks 1-3 differ
    from the equally rounded reference by a whole fp16 step of the map's largest values (2^-11 to 2^-10 of the max)
    already on the base weights, where the arithmetic error is 1e-6 -- and by no more on the rescaled ones."""
    for kmin, kmax in ((0, 0), (FI.KMIN, FI.KMAX)):
        sd = FI.rescaled(kmin, kmax, FI.RANGE_SEED, FI.STEM_KMIN)[0]
        e = FI.restated_block_errors(sd, arch, frames, ('fp16mx',), storage=True)['fp16mx']
        print(f'fp16mx with storage roundings, [{kmin}, {kmax}]:', {b: f'{v:.1e}' for b, v in e.items() if b < 5})
        for blk in FI.MX_F16_BLOCKS:
            assert e[blk] < FI.MX_F16_OUT_TOL, (blk, e[blk])
        assert max(e[b] for b in FI.MX_F16_BLOCKS) > FI.RESTATED_SHARE * FI.MX_F16_OUT_TOL
