"""GPU: colour frames and off-grid float frames through every stem path of every schedule.

Every other frame of the suite has R = G = B, and with identical channels a 3 -> 32 stem only sees sum_c w[:, c]: a
kernel that permutes its input channels, reads one plane three times, strides the float32 NCHW planes wrongly or packs
its operand in another channel order (spef_amd/blob.py x0 / x1, the int8 LUT dword) passes all of it. The float32 NCHW
inputs were always u8 / 255, 256 values inside [0, 1]. Here R, G and B are independent (tests/forward_inputs.py
``colour_frames``), the float frames are uniform off the 1 / 255 grid and, for int8, past [0, 1] on both sides;
tests/test_input_sensitivity.py (CPU) shows that each of six channel faults moves the compared maps by >= 0.25 of their
max on exactly these frames and by nothing on grey ones.

The stem paths: op 0 probes the stem kernel alone (u8 and float32 input, fp32 / fp16 / bf16 output); op 1 from u8 frames
runs the fused front kernel of the schedule (fp16 / bf16, fp16x2, fp16mx), and the stem + block 1 kernels with fusion
off; the int8 stem in both layouts. Every bound is an existing test's, restated with its source; none is widened.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import decode_ref as D
from oracle import int8_ref as Q
from oracle import model_ref as M
from oracle import resize_ref as R
from oracle.block_ref import oracle_block
from spef_amd import _lib as L
from spef_amd import blob as Bl
from spef_amd.arch import mobilenet_v2
from spef_amd.blob_q8 import pack_int8
from spef_amd.data.synthetic import synth_frames
from spef_amd.quant import BitWidths, calibrate
from spef_amd.weights import synthetic_state_dict

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forward_inputs as FI  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = pytest.mark.parametrize('b,h,w', FI.COLOUR_SHAPES)
SEED = 11   # tests/test_input_sensitivity.py measures the faults' effect on the same frames

# the constants of tests/test_gpu_odd_frames.py, with their sources
LOGIT_TOL = 1e-3          # north star, absolute (test_gpu_parity.py / test_gpu_x2.py / test_gpu_mx.py LOGIT_TOL)
X2_BLOCK_TOL = 5e-5       # test_gpu_x2.py::test_block_outputs_vs_oracle, of the map's max
MX_F16_OUT_TOL, MX_F32_TOL = 1.2e-3, 5e-5   # test_gpu_mx.py::test_block_outputs_vs_oracle (block 1 stores fp16)
F32_BLOCK_TOL, F32_HEAD_TOL = 1e-5, 1e-4    # test_gpu_parity.py::test_fp32_variant_vs_reference_golden
FP16_BLOCK_TOL = 2e-2     # test_gpu_parity.py::test_block_activations_vs_oracle
FP16_FRONT_TOL = 4e-3     # test_gpu_parity.py::test_front_kernel_vs_stem_block1 (u8, fused: the front kernel at op 1)
BF16_PAD_TOL = 5e-2       # test_gpu_odd_frames.py: a fifth of the smallest effect a wrong input has on these maps
LOGIT_TOL_BF16 = 6e-3     # test_gpu_parity.py LOGIT_TOL_BF16
POS_TOL_M, ORI_TOL_DEG = 1e-3, 0.1   # north star


@functools.lru_cache(maxsize=None)
def _sd():
    return FI.base_state_dict()


@functools.lru_cache(maxsize=None)
def _oracle(b, h, w, kind):
    """(inputs {layout: CPU tensor}, NHWC maps after op 0 and op 1, ori, pos) of the FP32 oracle, computed once.
    kind 'colour': colour_frames as u8 NHWC and as float32 NCHW (u8 / 255); 'float': float_frames, float32 NCHW only."""
    if kind == 'colour':
        fr = FI.colour_frames(b, h, w, SEED + h)
        x = M.u8_nhwc_to_nchw_f32(fr)
        inputs = {'u8': torch.from_numpy(fr), 'f32': x.contiguous()}
    else:
        x = FI.float_frames(b, h, w, SEED + h)
        inputs = {'f32': x}
    sd = _sd()
    with torch.no_grad():
        m0 = oracle_block(x, sd, 0)
        m1 = oracle_block(m0, sd, 1)
        ori, pos = M.forward(x, sd)
    maps = [m.permute(0, 2, 3, 1).contiguous().numpy() for m in (m0, m1)]
    for m in maps:
        m.setflags(write=False)
    return inputs, maps, ori.numpy(), pos.numpy()


def _rel(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(1e-6, np.abs(ref).max()))


def _check(eng, what, b, h, w, tol0, tol1, head_tol, f16_out1=False, tol1_u8=None):
    """Ops 0 and 1 and the head outputs on the colour frames in both layouts and on the float frames, against the
    oracle. ``f16_out1``: the schedule stores block 1's output in fp16 and the oracle's is rounded alike, as in
    test_gpu_mx.py."""
    for kind in ('colour', 'float'):
        inputs, maps, ro, rp = _oracle(b, h, w, kind)
        ref1 = maps[1].astype(np.float16).astype(np.float32) if f16_out1 else maps[1]
        for layout, xc in inputs.items():
            x = xc.cuda()
            e0 = _rel(eng.probe(x, 0).cpu().numpy(), maps[0])
            e1 = _rel(eng.probe(x, 1).cpu().numpy(), ref1)
            o, p = eng.forward(x)
            he = max(float(np.abs(o.cpu().numpy() - ro).max()), float(np.abs(p.cpu().numpy() - rp).max()))
            print(f'{what} {(b, h, w)} {kind} {layout}: err / map max op 0 {e0:.2e}, op 1 {e1:.2e}; head {he:.2e}')
            t1 = tol1_u8 if (tol1_u8 is not None and layout == 'u8') else tol1
            assert e0 < tol0, (what, kind, layout, 'op 0', e0)
            assert e1 < t1, (what, kind, layout, 'op 1', e1)
            assert he < head_tol, (what, kind, layout, 'head', he)


def _engine(dtype):
    from spef_amd.engine import Engine
    return Engine(Bl.pack(_sd(), dtype=dtype), 'cuda:0')


@pytest.fixture(scope='module')
def engines():
    made = {}

    def get(dtype):
        if dtype not in made:
            made[dtype] = _engine(dtype)
        return made[dtype]
    yield get
    for e in made.values():
        e.close()


# ------------------------------------------------------------------------------------------------ float schedules
@SHAPES
def test_fp32_colour(engines, b, h, w):
    _check(engines('fp32'), 'fp32', b, h, w, F32_BLOCK_TOL, F32_BLOCK_TOL, F32_HEAD_TOL)


@SHAPES
def test_fp16x2_colour(engines, b, h, w):
    """u8: stem_kernel<u8> at op 0, x2_front_kernel at op 1; float32: stem_kernel<f32> and block 1 on their own."""
    _check(engines('fp16x2'), 'fp16x2', b, h, w, X2_BLOCK_TOL, X2_BLOCK_TOL, LOGIT_TOL)


@pytest.mark.parametrize('mx_kernels', [1, 0])
@SHAPES
def test_fp16mx_colour(engines, b, h, w, mx_kernels):
    """u8 at op 1: front_mx_kernel (blob operand x1, mx_kernels = 1) or the fp16x2 front kernel's fp16-output variant
    (operand x0, 0). The op-0 probe runs the stem alone in fp32; block 1's output is stored in fp16."""
    mx = engines('fp16mx')
    mx.set_option(L.OPT_MX_KERNELS, mx_kernels)
    try:
        _check(mx, f'fp16mx mx_kernels={mx_kernels}', b, h, w, MX_F32_TOL, MX_F16_OUT_TOL, LOGIT_TOL, f16_out1=True)
    finally:
        mx.set_option(L.OPT_MX_KERNELS, 1)


@pytest.mark.parametrize('fused', [True, False])
@SHAPES
def test_fp16_colour(engines, b, h, w, fused):
    """u8 at op 1: front_vp_kernel when fused (held to the front kernel's own 4e-3), the stem and block-1 kernels
    otherwise."""
    e = engines('fp16')
    e.set_fused(fused)
    try:
        _check(e, f'fp16 fused={fused}', b, h, w, FP16_BLOCK_TOL, FP16_BLOCK_TOL, LOGIT_TOL,
               tol1_u8=FP16_FRONT_TOL if fused else None)
    finally:
        e.set_fused(True)


@SHAPES
def test_bf16_colour(engines, b, h, w):
    """bf16 (front_kernel, the non-vp front): no precision claim, a channel-order check -- 5e-2 of the map's max against
    the >= 0.25 a channel fault moves it by; head outputs at the bf16 variant's own bound."""
    _check(engines('bf16'), 'bf16', b, h, w, BF16_PAD_TOL, BF16_PAD_TOL, LOGIT_TOL_BF16)


# ----------------------------------------------------------------------------------------------------------- int8
Q8_OPS = (0, 1)


@functools.lru_cache(maxsize=None)
def _q8_sd():
    return synthetic_state_dict(mobilenet_v2(), seed=1001)


@functools.lru_cache(maxsize=None)
def _q8_params(low_bit):
    """test_gpu_int8.py's calibration (its q8 / q8low fixtures)."""
    bw = BitWidths.qmobilenet_default() if low_bit else None
    return calibrate(_q8_sd(), synth_frames(4, 128, 128, 900), **({'bw': bw} if low_bit else {}))


# float frames of the int8 float path: the issue's [-0.1, 1.1), and [-1.2, 1.2): with the calibrated image scale
# (about 1 / 127) the signed input quantizer clips below -1.008, which -0.1 does not reach
FLOAT_RANGES = ((-0.1, 1.1), (-1.2, 1.2))


@functools.lru_cache(maxsize=None)
def _q8_oracle(b, h, w, low_bit):
    """[(name, input CPU tensor, {op: NHWC float32 codes}, ori, pos)] of the integer oracle, computed once: the colour
    frames as u8 NHWC and as float32 NCHW, and the float frames of FLOAT_RANGES through the oracle's float entry."""
    sd, qp = _q8_sd(), _q8_params(low_bit)

    def run(frames):
        acts = {op: np.ascontiguousarray(Q.int8_forward(frames, sd, qp, upto=op).transpose(0, 2, 3, 1))
                .astype(np.float32) for op in Q8_OPS}
        return (acts,) + tuple(Q.int8_forward(frames, sd, qp))
    fr = FI.colour_frames(b, h, w, SEED + h)
    xf = M.u8_nhwc_to_nchw_f32(fr).contiguous()
    cases = [('colour u8', torch.from_numpy(fr)) + run(fr), ('colour f32', xf) + run(xf.numpy())]
    bits = Q._Bits(qp.get('bits')).image
    for lo, hi in FLOAT_RANGES:
        x = FI.float_frames(b, h, w, SEED + h, lo, hi)
        q = Q.input_quant_f32(x.numpy(), qp['image'], bits)
        if (lo, hi) == FLOAT_RANGES[-1]:   # the input clip is met on both sides
            assert q.min() == -(1 << (bits - 1)) and q.max() == (1 << (bits - 1)) - 1
            assert float(x.min()) / np.float32(qp['image']) < q.min() - 1
            assert float(x.max()) / np.float32(qp['image']) > q.max() + 1
        else:
            assert q.max() == (1 << (bits - 1)) - 1 and q.min() < 0
        cases.append((f'float [{lo}, {hi})', x) + run(x.numpy()))
    return cases


def _q8_check(eng, b, h, w, low_bit, what):
    for name, xc, acts, ro, rp in _q8_oracle(b, h, w, low_bit):
        x = xc.cuda()
        for op, ref in acts.items():
            got = eng.probe(x, op).cpu().numpy()
            assert got.shape == ref.shape, (what, name, op, got.shape, ref.shape)
            np.testing.assert_array_equal(got, ref, err_msg=f'{what}, {name}: op {op}')
        o, p = eng.forward(x)
        np.testing.assert_array_equal(o.cpu().numpy(), ro, err_msg=f'{what}, {name}: ori')
        np.testing.assert_array_equal(p.cpu().numpy(), rp, err_msg=f'{what}, {name}: pos')


@pytest.fixture(scope='module')
def q8_engines():
    from spef_amd.engine import Engine
    made = {}

    def get(low_bit, shift32):
        if (low_bit, shift32) not in made:
            made[(low_bit, shift32)] = Engine(pack_int8(_q8_sd(), _q8_params(low_bit), shift32=shift32), 'cuda:0')
        return made[(low_bit, shift32)]
    yield get
    for e in made.values():
        e.close()


@pytest.mark.parametrize('blob', ['default', 'general_shift', 'low_bit'])
@SHAPES
def test_int8_colour_bit_exact(q8_engines, b, h, w, blob):
    """INT8: ops 0 and 1 and the head outputs equal oracle/int8_ref.py bit for bit on the colour frames in both layouts
    (the u8 LUT dword [q_r, q_g, q_b, 0]; the float branch's three planes) and on float frames off the 1 / 255 grid
    and past [0, 1] (rintf(x / s_img) and the input clip on values no u8 frame gives) -- the default blob, a
    shift32=False blob and the reference QMobileNetV2's low-bit widths, fused and one kernel per conv."""
    low_bit, shift32 = blob == 'low_bit', blob != 'general_shift'
    eng = q8_engines(low_bit, shift32)
    try:
        for fused in (True, False):
            eng.set_fused(fused)
            _q8_check(eng, b, h, w, low_bit, f'{blob}, fused={fused}')
    finally:
        eng.set_fused(True)


# ---------------------------------------------------------------------------------------------------- predict_frames
@pytest.mark.parametrize('dtype,sharp', [('fp16mx', False), ('fp16x2', True)])
def test_predict_frames_colour_vs_resize_oracle_and_forward_oracle(dtype, sharp):
    """predict_frames on colour camera frames (2, 51, 67) -> (64, 96): the on-device resize followed by the stem against
    oracle/resize_ref.py pil_resize followed by the oracle's forward -- head outputs within the absolute 1e-3.
    (tests/test_gpu_preprocess.py compares this path with the GPU's own forward only.)

    fp16mx, the headline schedule (front_mx_kernel behind the resize), at the reference head init. fp16x2, the parity
    schedule for sharp heads, with a sharp orientation head (std 0.3) and a SPEED-range position bias, as
    test_gpu_mx.py::test_sharp_head_logits_absolute -- there the decoded pose is compared too, within 0.1 deg / 1 mm: at
    the reference init the softmax is flat and the decoded quaternion ill-conditioned for any implementation.
    (fp16mx at the sharp head is not held to 1e-3 here: the 2 x 3 final map of a 64 x 96 frame averages six pixels
    where the bench's 512 x 512 averages 256, and its logits measure 1.4e-3 from the oracle's.)"""
    from spef_amd.spe.spe_utils import SPEUtils
    from spef_amd.spe_mi355x import SPEMi355x
    arch = mobilenet_v2('ursonet', 1728, 3)
    sd = synthetic_state_dict(arch, seed=1001, head_std=0.3, pos_std=0.01, pos_bias=(0.3, -0.2, 12.0)) if sharp \
        else _sd()
    raw = FI.colour_frames(2, 51, 67, SEED)
    small = np.stack([R.pil_resize(f, 64, 96) for f in raw])
    assert small.shape == (2, 64, 96, 3)
    assert not (small[..., 0] == small[..., 1]).all() and not (small[..., 1] == small[..., 2]).all()
    ro, rp = M.forward(M.u8_nhwc_to_nchw_f32(small), sd)
    ro, rp = ro.numpy(), rp.numpy()
    hist, _ = D.orientation_histogram(12, False)
    rq = D.decode_orientation_batch(D.softmax_f32(ro), hist)
    su = SPEUtils(None, 'classification', 12, 3, False, 'regression')
    spe = SPEMi355x(Bl.pack(sd, dtype=dtype), 'cuda:0', su)
    try:
        pose, ms = spe.predict_frames(torch.from_numpy(raw), (64, 96))
        got = spe.engine.preprocess(torch.from_numpy(raw).cuda(), (64, 96))
        np.testing.assert_array_equal(got.cpu().numpy(), small)
        o, p = spe.engine.forward(got)
        lo = float(np.abs(o.cpu().numpy() - ro).max())
        po = float(np.abs(p.cpu().numpy() - rp).max())
    finally:
        spe.close()
    ao = float(D.angle_deg_stable(np.asarray(pose['ori'], np.float64), rq).max())
    pp = float(np.abs(np.asarray(pose['pos']) - rp).max())
    print(f'predict_frames colour {dtype} sharp={sharp}: max|d logit| {lo:.2e}, |d pos raw| {po:.2e}, '
          f'pose {ao:.2e} deg, {pp:.2e} m')
    assert ms > 0
    assert lo < LOGIT_TOL and po < LOGIT_TOL
    assert pp < POS_TOL_M
    if sharp:
        assert np.abs(ro).max() > 1.0 and ao < ORI_TOL_DEG
