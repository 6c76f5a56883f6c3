"""GPU: odd and non-multiple-of-4 frame sizes through every schedule.

Every other frame in the suite has even H, even W and W % 4 == 0, so three things never ran there: the bottom / right
zero padding of the stem and of block 2's depthwise (read only when the frame / the stem map is odd), the uint8 front
and stem kernels' byte-scatter staging on interior tiles with a different byte phase per row and an odd per-image base
(W % 4 != 0), and odd maps at the stem level and level 2, a 1 x 1 and a 1 x N final map. The shapes of
oracle/block_ref.py ODD_FRAME_SHAPES reach all of it; tests/test_edge_sensitivity.py (CPU) shows that a wrong padding
side moves the compared maps by >= 0.25 of their max at these shapes and frames, so nothing below passes vacuously.

Every bound is an existing test's, restated next to its use with its source; nothing is widened for these shapes. A
shape the library rejects raises in Engine (spef status != 0) and fails the test.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import int8_ref as Q
from oracle import model_ref as M
from oracle.block_ref import ODD_FRAME_SHAPES, odd_frames, oracle_block
from spef_amd import _lib as L
from spef_amd import blob as Bl
from spef_amd.arch import mobilenet_v2
from spef_amd.blob_q8 import pack_int8
from spef_amd.data.synthetic import synth_frames
from spef_amd.quant import BitWidths, calibrate
from spef_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

SHAPES = pytest.mark.parametrize('b,h,w', ODD_FRAME_SHAPES)

LOGIT_TOL = 1e-3          # north star, absolute (test_gpu_parity.py / test_gpu_x2.py / test_gpu_mx.py LOGIT_TOL)
X2_BLOCK_TOL = 5e-5       # test_gpu_x2.py::test_block_outputs_vs_oracle, of the map's max
MX_F16_OUT_TOL, MX_F16_HIDDEN_TOL, MX_F32_TOL = 1.2e-3, 2e-4, 5e-5   # test_gpu_mx.py::test_block_outputs_vs_oracle
MX_F16_BLOCKS, MX_F16_HIDDEN = range(1, 4), range(2, 5)              # test_gpu_mx.py F16_BLOCKS / F16_HIDDEN
F32_BLOCK_TOL, F32_HEAD_TOL = 1e-5, 1e-4   # test_gpu_parity.py::test_fp32_variant_vs_reference_golden
F32_OPS = (0, 1, 2, 4, 7, 17)
FP16_BLOCK_TOL = 2e-2     # test_gpu_parity.py::test_block_activations_vs_oracle
FP16_FRONT_TOL = 4e-3     # test_gpu_parity.py::test_front_kernel_vs_stem_block1, of the oracle map's max
# bf16 (the one user of the non-vp front_kernel): no precision claim -- one fifth of the smallest effect (0.25 of the
# map's max) that a wrong padding side has at these shapes, the floor tests/test_edge_sensitivity.py holds
BF16_PAD_TOL = 5e-2
Q8_OPS = (0, 1, 2, 3, 5, 8, 12, 16, 17)   # test_gpu_int8.py::test_int8_activations_bit_exact


@functools.lru_cache(maxsize=None)
def _sd():
    return synthetic_state_dict(mobilenet_v2('ursonet', 1728, 3), seed=1001)


def _u8(fr):
    return torch.from_numpy(fr).cuda()


def _f32(fr):
    return M.u8_nhwc_to_nchw_f32(fr).contiguous().cuda()


@functools.lru_cache(maxsize=None)
def _oracle(b, h, w):
    """The FP32 oracle at one shape, computed once: (frames, [NHWC map after op 0..17], ori, pos). The maps come from
    the per-block oracle chained, which is model_ref.backbone's own sequence of calls (the head outputs are checked
    against model_ref.forward)."""
    fr = odd_frames(b, h, w)
    x = M.u8_nhwc_to_nchw_f32(fr)
    sd = _sd()
    maps = []
    with torch.no_grad():
        y = x
        for op in range(18):
            y = oracle_block(y, sd, op)
            maps.append(y.permute(0, 2, 3, 1).contiguous().numpy())
        ori, pos = M.ursonet_head(M._conv_bn_act(y, sd, 'features.features.18', 1, 1, True), sd)
        ro, rp = M.forward(x, sd)
    assert torch.equal(ori, ro) and torch.equal(pos, rp)
    for m in maps:
        m.setflags(write=False)
    return fr, maps, ori.numpy(), pos.numpy()


def _rel(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(1e-6, np.abs(ref).max()))


def _head_err(eng, x, ro, rp):
    o, p = eng.forward(x)
    return max(float(np.abs(o.cpu().numpy() - ro).max()), float(np.abs(p.cpu().numpy() - rp).max()))


def _engine(dtype):
    from spef_amd.engine import Engine
    return Engine(Bl.pack(_sd(), dtype=dtype), 'cuda:0')


@pytest.fixture(scope='module')
def x2():
    e = _engine('fp16x2')
    yield e
    e.close()


@pytest.fixture(scope='module')
def mx():
    e = _engine('fp16mx')
    yield e
    e.close()


@pytest.fixture(scope='module')
def f32():
    e = _engine('fp32')
    yield e
    e.close()


@pytest.fixture(scope='module')
def fp16():
    e = _engine('fp16')
    yield e
    e.close()


@pytest.fixture(scope='module')
def bf16():
    e = _engine('bf16')
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------------- fp16x2
@SHAPES
def test_x2_blocks_and_heads_vs_oracle(x2, b, h, w):
    """fp16x2: every block output in both input layouts (u8 NHWC: the front kernel; f32 NCHW: stem + block 1 on their
    own) within 5e-5 of the oracle map's max, head outputs within the absolute 1e-3."""
    fr, maps, ro, rp = _oracle(b, h, w)
    for name, x in (('u8', _u8(fr)), ('f32', _f32(fr))):
        errs = {op: _rel(x2.probe(x, op).cpu().numpy(), maps[op]) for op in range(18)}
        he = _head_err(x2, x, ro, rp)
        print(f'fp16x2 {(b, h, w)} {name}: max block err / map max {max(errs.values()):.2e} '
              f'(op {max(errs, key=errs.get)}), head {he:.2e}')
        for op, err in errs.items():
            assert err < X2_BLOCK_TOL, (name, op, err)
        assert he < LOGIT_TOL, (name, he)


# ------------------------------------------------------------------------------------------------------- fp16mx
@pytest.mark.parametrize('mx_kernels', [1, 0])
@SHAPES
def test_mx_blocks_and_heads_vs_oracle(mx, b, h, w, mx_kernels):
    """fp16mx, on k_mx.hip (1) and on the fp16x2 kernels' fp16-I/O variants (0): the comparison and the bounds of
    test_gpu_mx.py::test_block_outputs_vs_oracle -- each block against the oracle block applied to the GPU's own
    previous probe with the schedule's fp16 storage points restated (hidden tensors of blocks 2-4 under mx_kernels = 1,
    outputs of blocks 1-3); fp16 outputs 1.2e-3, fp16 hidden 2e-4, the rest 5e-5 of the map's max. Head outputs within
    the absolute 1e-3 of the oracle's."""
    fr, _, ro, rp = _oracle(b, h, w)
    sd = _sd()
    f16_hidden = MX_F16_HIDDEN if mx_kernels else ()
    x = M.u8_nhwc_to_nchw_f32(fr)
    xg = _u8(fr)
    errs = {}
    mx.set_option(L.OPT_MX_KERNELS, mx_kernels)
    try:
        prev = None
        with torch.no_grad():
            for op in range(18):
                got = mx.probe(xg, op).cpu()
                if op == 0:
                    ref = oracle_block(x, sd, 0)
                elif op == 1:
                    ref = oracle_block(oracle_block(x, sd, 0), sd, 1)
                else:
                    ref = oracle_block(prev.permute(0, 3, 1, 2).contiguous(), sd, op, f16_hidden)
                if op in MX_F16_BLOCKS:
                    ref = ref.half().float()
                errs[op] = _rel(got.numpy(), ref.permute(0, 2, 3, 1).numpy())
                prev = got
        he = _head_err(mx, xg, ro, rp)
    finally:
        mx.set_option(L.OPT_MX_KERNELS, 1)
    print(f'fp16mx {(b, h, w)} mx_kernels={mx_kernels}: block err / map max',
          {k: f'{v:.1e}' for k, v in errs.items()}, f'head {he:.2e}')
    for op, err in errs.items():
        tol = MX_F16_OUT_TOL if op in MX_F16_BLOCKS else MX_F16_HIDDEN_TOL if op in f16_hidden else MX_F32_TOL
        assert err < tol, (op, err, tol)
    assert he < LOGIT_TOL, he


# --------------------------------------------------------------------------------------------------------- fp32
@SHAPES
def test_f32_blocks_and_heads_vs_oracle(f32, b, h, w):
    """fp32 blob (k_f32.hip, the reference's arithmetic): ops 0, 1, 2, 4, 7, 17 within 1e-5 of the map's max and the
    head outputs within 1e-4, in both input layouts."""
    fr, maps, ro, rp = _oracle(b, h, w)
    for name, x in (('u8', _u8(fr)), ('f32', _f32(fr))):
        errs = {op: _rel(f32.probe(x, op).cpu().numpy(), maps[op]) for op in F32_OPS}
        he = _head_err(f32, x, ro, rp)
        print(f'fp32 {(b, h, w)} {name}: max block err / map max {max(errs.values()):.2e}, head {he:.2e}')
        for op, err in errs.items():
            assert err < F32_BLOCK_TOL, (name, op, err)
        assert he < F32_HEAD_TOL, (name, he)


def test_f32_observed_forward_equals_backbone(f32):
    """The observed forward (spef_observe, the INT8 calibration's pass) at 101 x 137 writes the bytes Engine.backbone
    writes."""
    fr = odd_frames(2, 101, 137)
    obs = f32.observer()
    try:
        for x in (_u8(fr), _f32(fr)):
            want = f32.backbone(x)
            got = torch.full_like(want, float('nan'))
            obs.observe(x, got)
            assert want.shape == (2, 4, 5, 1280)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    finally:
        obs.close()


# --------------------------------------------------------------------------------------------------------- fp16
@SHAPES
def test_fp16_fused_bit_identical_to_unfused(fp16, b, h, w):
    """test_gpu_parity.py::test_fused_blocks_bit_identical_to_unfused at the odd shapes: ops 1-17 and the head
    outputs, float32 NCHW input."""
    x = _f32(odd_frames(b, h, w))
    try:
        for op in range(1, 18):
            fp16.set_fused(False)
            u = fp16.probe(x, op).cpu().numpy()
            fp16.set_fused(True)
            f = fp16.probe(x, op).cpu().numpy()
            assert np.array_equal(u, f), (op, float(np.abs(u - f).max()))
        fp16.set_fused(False)
        uo, up = [t.cpu().numpy() for t in fp16.forward(x)]
        fp16.set_fused(True)
        fo, fp = [t.cpu().numpy() for t in fp16.forward(x)]
        assert np.array_equal(uo, fo) and np.array_equal(up, fp)
    finally:
        fp16.set_fused(True)


@SHAPES
def test_fp16_wave_specialised_blocks_bit_identical(fp16, b, h, w):
    """test_gpu_parity.py::test_role_split_blocks_bit_identical_to_slab at the odd shapes: SPEF_OPT_WAVESPEC 0 / 1 / 2
    give the same bits at ops 8-17."""
    x = _u8(odd_frames(b, h, w))
    try:
        for op in range(8, 18):
            outs = []
            for mode in (0, 1, 2):
                fp16.set_option(L.OPT_WAVESPEC, mode)
                outs.append(fp16.probe(x, op).cpu().numpy())
            for mode in (1, 2):
                assert np.array_equal(outs[0], outs[mode]), (op, mode, float(np.abs(outs[0] - outs[mode]).max()))
    finally:
        fp16.set_option(L.OPT_WAVESPEC, 2)


@SHAPES
def test_fp16_front_kernel_and_blocks_vs_oracle(fp16, b, h, w):
    """The u8 front kernel (front_vp_kernel) against the stem + block-1 kernels of the f32 path and against the oracle
    at op 1, within 4e-3 of the oracle map's max; every block output of the u8 path within 2e-2 of the map's max."""
    fr, maps, _, _ = _oracle(b, h, w)
    x8, xf = _u8(fr), _f32(fr)
    got = fp16.probe(x8, 1).cpu().numpy()
    sep = fp16.probe(xf, 1).cpu().numpy()
    scale = float(np.abs(maps[1]).max())
    d_sep, d_ref = float(np.abs(got - sep).max() / scale), float(np.abs(got - maps[1]).max() / scale)
    errs = {op: _rel(fp16.probe(x8, op).cpu().numpy(), maps[op]) for op in range(18)}
    print(f'fp16 {(b, h, w)}: front vs separate {d_sep:.2e}, vs oracle {d_ref:.2e}; max block err / map max '
          f'{max(errs.values()):.2e} (op {max(errs, key=errs.get)})')
    assert got.shape == maps[1].shape
    assert d_sep < FP16_FRONT_TOL and d_ref < FP16_FRONT_TOL, (d_sep, d_ref)
    for op, err in errs.items():
        assert err < FP16_BLOCK_TOL, (op, err)


# --------------------------------------------------------------------------------------------------------- bf16
@SHAPES
def test_bf16_front_kernel_padding(bf16, b, h, w):
    """bf16, u8 input (front_kernel, then block 2): ops 1 and 2 within 5e-2 of the oracle map's max -- a padding check
    (BF16_PAD_TOL above), not a precision bound."""
    fr, maps, _, _ = _oracle(b, h, w)
    x = _u8(fr)
    errs = {op: _rel(bf16.probe(x, op).cpu().numpy(), maps[op]) for op in (1, 2)}
    print(f'bf16 {(b, h, w)}: err / map max at op 1 {errs[1]:.2e}, op 2 {errs[2]:.2e}')
    for op, err in errs.items():
        assert err < BF16_PAD_TOL, (op, err)


# --------------------------------------------------------------------------------------------------------- int8
@functools.lru_cache(maxsize=None)
def _q8_sd():
    return synthetic_state_dict(mobilenet_v2(), seed=1001)


@functools.lru_cache(maxsize=None)
def _q8_params(low_bit):
    """test_gpu_int8.py's calibration (its q8 / q8low fixtures)."""
    bw = BitWidths.qmobilenet_default() if low_bit else None
    return calibrate(_q8_sd(), synth_frames(4, 128, 128, 900), **({'bw': bw} if low_bit else {}))


@functools.lru_cache(maxsize=None)
def _q8_oracle(b, h, w, low_bit=False):
    """The integer oracle at one shape, computed once: (frames, {op: NHWC float32 codes}, ori, pos)."""
    fr = odd_frames(b, h, w)
    sd, qp = _q8_sd(), _q8_params(low_bit)
    acts = {op: np.ascontiguousarray(Q.int8_forward(fr, sd, qp, upto=op).transpose(0, 2, 3, 1)).astype(np.float32)
            for op in Q8_OPS}
    ro, rp = Q.int8_forward(fr, sd, qp)
    return fr, acts, ro, rp


def _q8_check(eng, x, acts, ro, rp, what):
    for op, ref in acts.items():
        got = eng.probe(x, op).cpu().numpy()
        assert got.shape == ref.shape, (what, op, got.shape, ref.shape)
        np.testing.assert_array_equal(got, ref, err_msg=f'{what}: op {op}')
    o, p = eng.forward(x)
    np.testing.assert_array_equal(o.cpu().numpy(), ro, err_msg=f'{what}: ori')
    np.testing.assert_array_equal(p.cpu().numpy(), rp, err_msg=f'{what}: pos')


def _q8_engine(low_bit, shift32):
    from spef_amd.engine import Engine
    return Engine(pack_int8(_q8_sd(), _q8_params(low_bit), shift32=shift32), 'cuda:0')


@pytest.fixture(scope='module')
def q8():
    e = _q8_engine(False, True)
    yield e
    e.close()


@pytest.fixture(scope='module')
def q8_general_shift():
    e = _q8_engine(False, False)
    yield e
    e.close()


@pytest.fixture(scope='module')
def q8low():
    e = _q8_engine(True, True)
    yield e
    e.close()


@SHAPES
def test_int8_bit_exact(q8, b, h, w):
    """INT8: activations at test_gpu_int8.py's ops and the head outputs equal oracle/int8_ref.py bit for bit, for u8 and
    float32 NCHW input, with the late blocks as slab (SPEF_OPT_Q8_ROLESPLIT 0) and role-split (1) kernels, and on the
    one-kernel-per-conv schedule (set_fused(False))."""
    fr, acts, ro, rp = _q8_oracle(b, h, w)
    x8, xf = _u8(fr), _f32(fr)
    try:
        for rolesplit in (0, 1):
            q8.set_option(L.OPT_Q8_ROLESPLIT, rolesplit)
            for name, x in (('u8', x8), ('f32', xf)):
                _q8_check(q8, x, acts, ro, rp, f'rolesplit {rolesplit}, {name}')
        q8.set_option(L.OPT_Q8_ROLESPLIT, 0)
        q8.set_fused(False)
        for name, x in (('u8', x8), ('f32', xf)):
            _q8_check(q8, x, acts, ro, rp, f'unfused, {name}')
    finally:
        q8.set_fused(True)
        q8.set_option(L.OPT_Q8_ROLESPLIT, 0)


@SHAPES
def test_int8_general_shift_bit_exact(q8_general_shift, b, h, w):
    """A shift32=False blob (the fused blocks' general-shift requant), slab and role-split late blocks."""
    fr, acts, ro, rp = _q8_oracle(b, h, w)
    x8 = _u8(fr)
    try:
        for rolesplit in (0, 1):
            q8_general_shift.set_option(L.OPT_Q8_ROLESPLIT, rolesplit)
            _q8_check(q8_general_shift, x8, acts, ro, rp, f'general shift, rolesplit {rolesplit}')
    finally:
        q8_general_shift.set_option(L.OPT_Q8_ROLESPLIT, 0)


@pytest.mark.parametrize('b,h,w', [(2, 33, 35), (2, 101, 137)])
def test_int8_low_bit_bit_exact(q8low, b, h, w):
    """The reference QMobileNetV2's default 3-bit / 4-bit-shared widths (quant.BitWidths.qmobilenet_default): the
    padding code and the quantisers' clip ranges differ from the 8-bit case."""
    fr, acts, ro, rp = _q8_oracle(b, h, w, True)
    for name, x in (('u8', _u8(fr)), ('f32', _f32(fr))):
        _q8_check(q8low, x, acts, ro, rp, f'low bit, {name}')


# --------------------------------------------------------------------------------------------------------- trim
@pytest.mark.parametrize('dtype', ['fp16mx', 'fp16x2'])
@pytest.mark.parametrize('b,h,w', [(2, 32, 32), (2, 32, 205), (3, 37, 50)])
def test_trim_bit_identical_on_nearly_empty_tiles(x2, mx, dtype, b, h, w):
    """SPEF_OPT_TRIM 0 (the earlier last-conv kernel) against the default (128-pixel x 320-channel tiles,
    tests/test_gpu_trim.py) where the one 128-pixel tile is nearly empty: HW = 1, 7, 4 and M = B HW = 2, 14, 12."""
    eng = {'fp16mx': mx, 'fp16x2': x2}[dtype]
    x = _u8(odd_frames(b, h, w))

    def run():
        return [t.cpu().numpy() for t in eng.forward(x)]
    try:
        eng.set_option(L.OPT_TRIM, 0)
        o0, p0 = run()
    finally:
        eng.set_option(L.OPT_TRIM, 1)
    o1, p1 = run()
    assert np.isfinite(o1).all() and np.abs(o1).max() > 0
    assert np.array_equal(o0, o1), float(np.abs(o0 - o1).max())
    assert np.array_equal(p0, p1), float(np.abs(p0 - p1).max())
