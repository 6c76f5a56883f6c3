"""GPU: every schedule on weights whose internal channels span 2^KMIN .. 2^KMAX instead of one decade.

With the synthetic weights every stem, expand, depthwise and block output peaks between 2.5 and 10.1, so the fp16
storage points (fp16, fp16mx) and the hi + lo fp16 operand splits (spef_amd/blob.py split_f16, csrc/x2_common.hpp
relu_split8 / split8 / lo_pair) have never seen another magnitude. tests/forward_inputs.py ``rescaled_state_dict``
scales every internal channel by its own power of two and unscales it at its consumer -- the same function, bit for
bit in the oracle (tests/test_channel_range_host.py), and the freedom a trained checkpoint has between a BatchNorm
channel's scale and its consumer's weights. [KMIN, KMAX] is the widest range in which the float64 restatement of each
schedule's arithmetic keeps within a quarter of the schedule's block bound (same CPU module); the kernels are held to
the whole, unchanged bound here.

Each block is compared with the oracle's block applied to the GPU's own previous probe, so each kernel is checked on
its own (the pattern and the fp16 restatements of test_gpu_mx.py::test_block_outputs_vs_oracle); ops 0 and 1 are
compared from the frames (u8 input: block 1 runs fused with the stem). Colour frames at the ragged (1, 100, 136).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import int8_ref as Q
from oracle import model_ref as M
from oracle.block_ref import oracle_block
from spef_amd import _lib as L
from spef_amd import blob as Bl
from spef_amd.blob_q8 import pack_int8
from spef_amd.data.synthetic import synth_frames
from spef_amd.quant import calibrate, validate

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forward_inputs as FI  # noqa: E402

pytestmark = pytest.mark.gpu

# the constants of tests/test_gpu_odd_frames.py, with their sources
LOGIT_TOL = 1e-3          # north star, absolute
X2_BLOCK_TOL = 5e-5       # test_gpu_x2.py::test_block_outputs_vs_oracle, of the map's max
MX_F16_OUT_TOL, MX_F16_HIDDEN_TOL, MX_F32_TOL = 1.2e-3, 2e-4, 5e-5   # test_gpu_mx.py::test_block_outputs_vs_oracle
MX_F16_BLOCKS, MX_F16_HIDDEN = range(1, 4), range(2, 5)
F32_BLOCK_TOL, F32_HEAD_TOL = 1e-5, 1e-4   # test_gpu_parity.py::test_fp32_variant_vs_reference_golden
FP16_BLOCK_TOL = 2e-2     # test_gpu_parity.py::test_block_activations_vs_oracle
BF16_BLOCK_TOL = 5e-2     # test_gpu_odd_frames.py BF16_PAD_TOL, the one block bound bf16 has
LOGIT_TOL_BF16 = 6e-3     # test_gpu_parity.py LOGIT_TOL_BF16
Q8_OPS = (0, 1, 2, 3, 5, 8, 12, 16, 17)   # test_gpu_int8.py::test_int8_activations_bit_exact


@functools.lru_cache(maxsize=None)
def _frames():
    b, h, w = FI.RANGE_SHAPE
    return FI.colour_frames(b, h, w, 11 + h)   # the frames of tests/test_channel_range_host.py


@functools.lru_cache(maxsize=None)
def _head_ref():
    with torch.no_grad():
        o, p = M.forward(M.u8_nhwc_to_nchw_f32(_frames()), FI.rescaled()[0])
    return o.numpy(), p.numpy()


def _blocks_vs_oracle(eng, f16_out=(), f16_hidden=()):
    """{op: max |GPU - oracle| / max |oracle|} for ops 0..17 on the rescaled weights, and the head outputs' max
    absolute error."""
    sd = FI.rescaled()[0]
    fr = _frames()
    x = M.u8_nhwc_to_nchw_f32(fr)
    xg = torch.from_numpy(fr).cuda()
    errs, prev = {}, None
    with torch.no_grad():
        for op in range(18):
            got = eng.probe(xg, op).cpu()
            if op == 0:
                ref = oracle_block(x, sd, 0)
            elif op == 1:
                ref = oracle_block(oracle_block(x, sd, 0), sd, 1)
            else:
                ref = oracle_block(prev.permute(0, 3, 1, 2).contiguous(), sd, op, f16_hidden)
            if op in f16_out:
                ref = ref.half().float()
            ref = ref.permute(0, 2, 3, 1).numpy()
            assert got.shape == ref.shape, (op, got.shape, ref.shape)
            assert np.isfinite(got.numpy()).all(), op
            errs[op] = float(np.abs(got.numpy() - ref).max() / max(1e-6, np.abs(ref).max()))
            prev = got
    o, p = eng.forward(xg)
    ro, rp = _head_ref()
    he = max(float(np.abs(o.cpu().numpy() - ro).max()), float(np.abs(p.cpu().numpy() - rp).max()))
    return errs, he


def _report(what, errs, he):
    print(f'{what}, channel scales 2^[{FI.KMIN}, {FI.KMAX}]: block err / map max',
          {k: f'{v:.1e}' for k, v in errs.items()}, f'max {max(errs.values()):.2e}; head {he:.2e}')


@pytest.fixture(scope='module')
def engines():
    from spef_amd.engine import Engine
    made = {}

    def get(dtype):
        if dtype not in made:
            made[dtype] = Engine(Bl.pack(FI.rescaled()[0], dtype=dtype), 'cuda:0')
        return made[dtype]
    yield get
    for e in made.values():
        e.close()


@pytest.mark.parametrize('dtype,block_tol,head_tol', [('fp32', F32_BLOCK_TOL, F32_HEAD_TOL),
                                                      ('fp16x2', X2_BLOCK_TOL, LOGIT_TOL),
                                                      ('fp16', FP16_BLOCK_TOL, LOGIT_TOL),
                                                      ('bf16', BF16_BLOCK_TOL, LOGIT_TOL_BF16)])
def test_blocks_and_heads_on_rescaled_weights(engines, dtype, block_tol, head_tol):
    """fp32, fp16x2, fp16, bf16: every op within the schedule's block bound of the oracle block on the GPU's own
    previous probe, head outputs within the schedule's absolute bound of the oracle's."""
    errs, he = _blocks_vs_oracle(engines(dtype))
    _report(dtype, errs, he)
    for op, err in errs.items():
        assert err < block_tol, (dtype, op, err)
    assert he < head_tol, (dtype, he)


@pytest.mark.parametrize('mx_kernels', [1, 0])
def test_fp16mx_blocks_and_heads_on_rescaled_weights(engines, mx_kernels):
    """fp16mx on k_mx.hip (1) and on the fp16x2 kernels' fp16-I/O variants (0), with the bounds and the restated fp16
    storage points of test_gpu_mx.py::test_block_outputs_vs_oracle: fp16 outputs of blocks 1-3 1.2e-3, fp16 hidden
    tensors (blocks 2-4 under mx_kernels = 1) 2e-4, the rest 5e-5 of the map's max; head outputs 1e-3 absolute."""
    mx = engines('fp16mx')
    f16_hidden = MX_F16_HIDDEN if mx_kernels else ()
    mx.set_option(L.OPT_MX_KERNELS, mx_kernels)
    try:
        errs, he = _blocks_vs_oracle(mx, MX_F16_BLOCKS, f16_hidden)
    finally:
        mx.set_option(L.OPT_MX_KERNELS, 1)
    _report(f'fp16mx mx_kernels={mx_kernels}', errs, he)
    for op, err in errs.items():
        tol = MX_F16_OUT_TOL if op in MX_F16_BLOCKS else MX_F16_HIDDEN_TOL if op in f16_hidden else MX_F32_TOL
        assert err < tol, (op, err, tol)
    assert he < LOGIT_TOL, he


# ----------------------------------------------------------------------------------------------------------- int8
@functools.lru_cache(maxsize=None)
def _q8(percentile):
    """Activation scales calibrated on the rescaled weights (test_gpu_int8.py's frames), and the integer oracle on the
    test's frames: ({op: NHWC float32 codes}, ori, pos, {conv: (clipped below, clipped above)})."""
    sd = FI.rescaled()[0]
    qp = calibrate(sd, synth_frames(4, 128, 128, 900), percentile=percentile)
    validate(qp)
    fr = _frames()
    acts = {op: np.ascontiguousarray(Q.int8_forward(fr, sd, qp, upto=op).transpose(0, 2, 3, 1)).astype(np.float32)
            for op in Q8_OPS}
    clips = {}
    ro, rp = Q.int8_forward(fr, sd, qp, clips=clips)
    return qp, acts, ro, rp, {k: v[0] for k, v in clips.items()}


@pytest.mark.parametrize('percentile', [99.999, 99.0])
def test_int8_bit_exact_on_rescaled_weights(percentile):
    """INT8 calibrated on the rescaled weights: per-tensor activation scales over channels that span 2^12 put the
    large channels at the top of the code range and the small ones in its lowest codes. Ops Q8_OPS and the head outputs
    equal the integer oracle bit for bit, late blocks as slab (SPEF_OPT_Q8_ROLESPLIT 0) and role-split (1) kernels.

    The case must drive the requant clamps or it adds nothing, so the oracle's own values before the clip are counted:
    the unsigned quantizers (stem, expand, depthwise, last conv) clip below zero and above their top code, 2.1e3 values
    above at the default percentile (99.999) and 2.1e4 with the scales calibrated at the 99th percentile, the second
    case; the stem's codes, which the probe at op 0 sees, hold both 0 and 255. The signed block-output quantizers see
    the residual stream, which the rescaling leaves alone, and clip nothing in either case: their clamps are not what
    this test adds."""
    from spef_amd.engine import Engine
    qp, acts, ro, rp, clips = _q8(percentile)
    unsigned = [v for k, v in clips.items() if not k.endswith('.project')]
    signed = [v for k, v in clips.items() if k.endswith('.project')]
    print(f'int8 percentile {percentile}: unsigned quantizers clipped below / above',
          sum(v[0] for v in unsigned), sum(v[1] for v in unsigned), '; signed', sum(v[0] for v in signed),
          sum(v[1] for v in signed))
    assert sum(v[0] for v in unsigned) > 0 and sum(v[1] for v in unsigned) > 1000
    assert clips['stem'][0] > 0 and clips['stem'][1] > 0 and acts[0].min() == 0 and acts[0].max() == 255
    x = torch.from_numpy(_frames()).cuda()
    eng = Engine(pack_int8(FI.rescaled()[0], qp), 'cuda:0')
    try:
        for rolesplit in (0, 1):
            eng.set_option(L.OPT_Q8_ROLESPLIT, rolesplit)
            for op, ref in acts.items():
                got = eng.probe(x, op).cpu().numpy()
                assert got.shape == ref.shape, (rolesplit, op, got.shape, ref.shape)
                np.testing.assert_array_equal(got, ref, err_msg=f'rolesplit {rolesplit}: op {op}')
            o, p = eng.forward(x)
            np.testing.assert_array_equal(o.cpu().numpy(), ro, err_msg=f'rolesplit {rolesplit}: ori')
            np.testing.assert_array_equal(p.cpu().numpy(), rp, err_msg=f'rolesplit {rolesplit}: pos')
    finally:
        eng.set_option(L.OPT_Q8_ROLESPLIT, 0)
        eng.close()
