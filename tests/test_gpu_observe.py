"""Histogram observers on the GPU (csrc/k_observe.hip, spef_observe): every count equals the NumPy twin
``quant.observe_host`` exactly, the observed forward is the fp32 schedule bit for bit, and the scales calibrated from
the device statistics give an int8 engine that matches the integer oracle."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from bench import synth_frames
from oracle import int8_ref as Q
from oracle import model_ref as M
from spef_amd import blob as Bl
from spef_amd import quant as Qt
from spef_amd.arch import mobilenet_v2
from spef_amd.blob_q8 import pack_int8
from spef_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

N_BLOCKS = 17
TAP_FINAL, TAP_LAST = 2 + 3 * N_BLOCKS, 3 + 3 * N_BLOCKS
LO, HI = 103 << 23, 135 << 23


def f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def specials():
    """0, -0.0, denormals, the floats around 2^-24, 1.0, both sides of a bin edge, 255.999, 256.0, +-inf, NaN, and the
    negative twins (the values of test_observe_host.py's first test)."""
    edge = LO + (1000 << 15)
    pos = np.array([0.0, f32(1), f32(0x007fffff), f32(LO - 1), f32(LO), 1.0, f32(edge - 1), f32(edge), f32(edge + 1),
                    255.999, f32(HI - 1), 256.0, 3.0e38, np.inf, np.nan], np.float32)
    return np.concatenate([pos, -pos])


def values(n, seed):
    """Normal values x 2^U(-30, 10) with the special values mixed in at random places."""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal(n) * np.exp2(rng.uniform(-30, 10, n))).astype(np.float32)
    sp = rng.permutation(specials())
    k = min(n, sp.size)
    v[rng.choice(n, k, replace=False)] = sp[:k]
    return v


@pytest.fixture(scope='module')
def sd():
    return synthetic_state_dict(mobilenet_v2(), seed=1001)


@pytest.fixture(scope='module')
def eng(sd):
    from spef_amd.engine import Engine
    e = Engine(Bl.pack(sd, mobilenet_v2(), dtype='fp32'), 'cuda:0')
    yield e
    e.close()


@pytest.fixture()
def obs(eng):
    o = eng.observer()
    yield o
    o.close()


def offset_tensor(v):
    """``v`` on the device, starting one float past a 16-byte boundary."""
    buf = torch.empty(v.size + 1, dtype=torch.float32, device='cuda:0')
    assert buf.data_ptr() % 16 == 0
    t = buf[1:]
    t.copy_(torch.from_numpy(v))
    return t


def assert_tap(counters, hist, tap, want, msg=''):
    np.testing.assert_array_equal(counters[tap], want[0], err_msg=f'counters of tap {tap} {msg}')
    np.testing.assert_array_equal(hist[tap], want[1], err_msg=f'bins of tap {tap} {msg}')


def test_info(obs):
    assert obs.n_taps == 4 + 3 * N_BLOCKS and obs.n_bins == Qt.OBS_BINS
    c, h = obs.read()
    assert c.shape == (obs.n_taps, 8) and h.shape == (obs.n_taps, Qt.OBS_BINS) and not c.any() and not h.any()


@pytest.mark.parametrize('n', [1, 3, 4, 63, 4097, (1 << 20) + 5])
def test_kernel_equals_twin(obs, n):
    v = values(n, n)
    obs.update(3, offset_tensor(v))
    c, h = obs.read()
    assert_tap(c, h, 3, Qt.observe_host(v))
    assert int(c[3][Qt.N_TOTAL]) == n == int(c[3][1:4].sum() + h[3].sum())
    assert not np.delete(c, 3, 0).any() and not np.delete(h, 3, 0).any()   # no other tap was touched


@pytest.mark.parametrize('kind', ['zeros', 'repeated', 'aligned'])
def test_kernel_equals_twin_degenerate(obs, kind):
    if kind == 'zeros':
        v = np.zeros(1 << 20, np.float32)
    elif kind == 'repeated':   # every lane adds to one LDS address
        v = np.full((1 << 20) + 3, 1.2345, np.float32)
    else:
        v = values(100003, 5)
    t = torch.from_numpy(v).cuda() if kind == 'aligned' else offset_tensor(v)
    obs.update(TAP_LAST, t)
    c, h = obs.read()
    assert_tap(c, h, TAP_LAST, Qt.observe_host(v), kind)


def test_more_than_2_31_values(obs):
    """The launcher cuts a tensor into launches of 2^31 values (no LDS bin can wrap): one that needs two, from an odd
    pointer, with a value on either side of the cut. The expected statistic is known without a host pass."""
    n = (1 << 31) + 5
    buf = torch.zeros(n + 1, dtype=torch.float32, device='cuda:0')
    t = buf[1:]
    head = (16 - t.data_ptr() % 16) % 16 // 4
    t[(1 << 31) - 1] = 1.0
    t[(1 << 31) + head] = 3.0
    t[n - 1] = -2.0
    obs.update(0, t)
    c, h = obs.read()
    del buf, t
    assert [int(x) for x in c[0][:5]] == [n, n - 3, 0, 0, int(np.float32(3.0).view(np.uint32))]
    bins = {(int(np.float32(x).view(np.uint32)) - LO) >> 15 for x in (1.0, 2.0, 3.0)}
    assert set(np.nonzero(h[0])[0]) == bins and int(h[0].sum()) == 3


def test_updates_accumulate_reset_and_isolation(eng, obs):
    a, b = values(5001, 1), values(777, 2)
    obs.update(7, offset_tensor(a))
    obs.update(7, torch.from_numpy(b).cuda())
    other = eng.observer()
    try:
        other.update(7, torch.from_numpy(b).cuda())
        c, h = obs.read()
        assert_tap(c, h, 7, Qt.observe_host(np.concatenate([a, b])), 'two updates')
        assert_tap(c, h, 7, Qt.observe_host([a, b]))
        c2, h2 = other.read()
        assert_tap(c2, h2, 7, Qt.observe_host(b), 'second observer')
        obs.reset()
        c, h = obs.read()
        assert not c.any() and not h.any()
        c2, h2 = other.read()
        assert_tap(c2, h2, 7, Qt.observe_host(b), 'second observer after the first one was reset')
    finally:
        other.close()


def test_bad_arguments(sd, eng, obs):
    from spef_amd import _lib as L
    from spef_amd.engine import Engine
    t = torch.ones(8, device='cuda:0')
    for tap in (-1, obs.n_taps):
        with pytest.raises(AssertionError):
            obs.update(tap, t)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert eng.lib.spef_observer_update(obs.handle, 0, C.c_void_p(t.data_ptr()), -1, s) == L.ERR_ARG
    assert eng.lib.spef_observer_update(obs.handle, 0, C.c_void_p(t.data_ptr()), 0, s) == L.OK   # a no-op
    assert eng.lib.spef_observer_update(obs.handle, 0, None, 0, s) == L.OK
    c, h = obs.read()
    assert not c.any() and not h.any()
    x = torch.from_numpy(synth_frames(1, 64, 64, 3)).cuda()
    mx = Engine(Bl.pack(sd, mobilenet_v2(), dtype='fp16mx'), 'cuda:0')
    try:   # observe needs the fp32 schedule
        o2 = mx.observer()
        with pytest.raises(L.SpefError) as ei:
            o2.observe(x)
        assert ei.value.code == L.ERR_STATE
        o2.close()
    finally:
        mx.close()
    nores = Engine(Bl.pack(sd, mobilenet_v2(residual=False), dtype='fp32'), 'cuda:0')
    try:   # an observer of a model with another op list
        nores.reserve(1, 64, 64)
        rc = eng.lib.spef_observe(nores.ctx, obs.handle, C.c_void_p(x.data_ptr()), L.IN_U8_NHWC, 1, 64, 64, None, s)
        assert rc == L.ERR_ARG
    finally:
        nores.close()
    rc = eng.lib.spef_observe(eng.ctx, obs.handle, C.c_void_p(x.data_ptr()), L.IN_U8_NHWC, 1, 96, 96, None, s)
    assert rc == L.ERR_STATE   # spef_reserve does not cover 96 x 96


@pytest.fixture(scope='module')
def observed64(eng):
    """One observed forward of 2 x 64 x 64 uint8 frames: (frames, device frames, features, counters, hist)."""
    fr = synth_frames(2, 64, 64, 31)
    x = torch.from_numpy(fr).cuda()
    o = eng.observer()
    feat = torch.empty((2, 2, 2, 1280), dtype=torch.float32, device='cuda:0')
    o.observe(x, feat)
    c, h = o.read()
    o.close()
    return fr, x, feat, c, h


def test_observed_forward_is_the_fp32_schedule(eng, observed64):
    fr, x, feat, c, h = observed64
    assert torch.equal(feat, eng.backbone(x))


def test_observed_taps_equal_twin_of_probes(eng, observed64):
    fr, x, feat, c, h = observed64
    arch = mobilenet_v2()
    assert_tap(c, h, 0, Qt.observe_host(fr.astype(np.float32) / np.float32(255)), 'image')
    assert int(c[0][Qt.N_TOTAL]) == fr.size
    assert_tap(c, h, 1, Qt.observe_host(eng.probe(x, 0)), 'stem')
    assert not c[2].any() and not c[3].any() and not h[2].any() and not h[3].any()   # block 1: no quant, no expand
    n_res = 0
    for i in range(2, N_BLOCKS + 1):
        tap = 2 + 3 * (i - 1)
        xin = eng.probe(x, i - 1)
        if arch.blocks[i - 1].residual:
            n_res += 1
            assert int(c[tap][Qt.N_TOTAL]) == 2 * xin.numel(), f'block {i}'
        else:
            assert_tap(c, h, tap, Qt.observe_host(xin), f'quant of block {i}')
        hid = arch.blocks[i - 1].hidden
        assert int(c[tap + 1][Qt.N_TOTAL]) == xin.numel() // arch.blocks[i - 1].cin * hid, f'expand of block {i}'
        assert int(c[tap + 2][Qt.N_TOTAL]) == eng.probe(x, i).numel() // arch.blocks[i - 1].cout * hid, f'dw of block {i}'
    assert n_res == 10
    assert_tap(c, h, TAP_FINAL, Qt.observe_host(eng.probe(x, N_BLOCKS)), 'final')
    assert_tap(c, h, TAP_LAST, Qt.observe_host(eng.backbone(x)), 'last')
    # every value lands in exactly one place
    np.testing.assert_array_equal(c[:, Qt.N_TOTAL], c[:, 1:4].sum(axis=1) + h.sum(axis=1))


def test_float_layout_gives_the_same_counts(eng, observed64):
    fr, x, feat, c, h = observed64
    o = eng.observer()
    try:
        o.observe(M.u8_nhwc_to_nchw_f32(fr).contiguous().cuda())
        c2, h2 = o.read()
    finally:
        o.close()
    np.testing.assert_array_equal(c, c2)
    np.testing.assert_array_equal(h, h2)


def test_batch_cuts_and_graph_replay(eng):
    fr = synth_frames(4, 64, 64, 37)
    x = torch.from_numpy(fr).cuda()
    o = eng.observer()
    try:
        o.observe(x)
        c4, h4 = o.read()
        o.reset()
        o.observe(x[:2].contiguous())
        o.observe(x[2:].contiguous())
        c22, h22 = o.read()
        np.testing.assert_array_equal(c4, c22)
        np.testing.assert_array_equal(h4, h22)
        # no allocation and no host synchronisation inside: the same call captured and replayed twice
        feat = torch.empty((4, 2, 2, 1280), dtype=torch.float32, device='cuda:0')
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            o.observe(x, feat)
        o.reset()
        feat.zero_()
        g.replay()
        cg, hg = o.read()
        np.testing.assert_array_equal(c4, cg)
        np.testing.assert_array_equal(h4, hg)
        assert torch.equal(feat, eng.backbone(x))
        g.replay()
        cg, hg = o.read()
        np.testing.assert_array_equal(2 * c4[:, :4], cg[:, :4])
        np.testing.assert_array_equal(c4[:, Qt.MAX_BITS], cg[:, Qt.MAX_BITS])
        np.testing.assert_array_equal(2 * h4, hg)
    finally:
        o.close()


def test_hidden_taps_against_host_taps(sd, eng):
    """expand, dw and the quant taps of residual blocks are not reachable by a probe: their device percentile against
    the exact order statistic of the host's float model (``quant.taps``) on the 4 x 128 x 128 calibration frames. The
    ratio lies in [1 - 2^-9, (1 + 2^-8)(1 + 2^-9)]: 2^-8 is the bin, 2^-9 what the device and torch forwards may differ
    by (about 200 x the 1e-5 the fp32 schedule is held to in test_gpu_c2_precision.py)."""
    fr = synth_frames(4, 128, 128, 900)
    o = eng.observer()
    try:
        o.observe(torch.from_numpy(fr).cuda())
        c, h = o.read()
    finally:
        o.close()
    arch = mobilenet_v2()
    lo, hi = 1 - 2.0 ** -9, (1 + 2.0 ** -8) * (1 + 2.0 ** -9)
    worst_lo, worst_hi, checked = np.inf, 0.0, 0
    for tap, name, ts in Qt.taps(sd, fr):
        assert int(c[tap][Qt.N_TOTAL]) == sum(t.numel() for t in ts), name
        assert int(c[tap][Qt.N_OVER]) == 0 and int(c[tap][Qt.N_NONFINITE]) == 0, name
        part = name.split('.')[-1]
        if not (part in ('expand', 'dw') or (part == 'quant' and arch.blocks[int(name.split('.')[1]) - 1].residual)):
            continue
        v = np.abs(np.concatenate([t.numpy().reshape(-1) for t in ts]))
        for p in (99.0, 99.9):
            r = int(np.ceil(p / 100.0 * (v.size - 1)))
            exact = float(np.partition(v, r)[r])
            ratio = Qt._hist_percentile(c[tap], h[tap], p) / exact
            worst_lo, worst_hi, checked = min(worst_lo, ratio), max(worst_hi, ratio), checked + 1
            print(f'{name} p={p}: device percentile / exact host order statistic = {ratio:.6f}')
            assert lo <= ratio <= hi, (name, p, ratio)
    print(f'hidden taps: {checked} ratios in [{worst_lo:.6f}, {worst_hi:.6f}]')
    assert checked == 2 * (16 + 17 + 10)


def test_calibrate_device_int8_engine(sd):
    """Scales from the device statistics -> int8 blob -> engine: bit-exact against the integer oracle run with the
    same scales (test_gpu_int8.py's comparison), and as close to the fake-quant graph and to FP32 as
    test_int8_oracle.py asks of the host calibration."""
    from spef_amd.engine import Engine
    qp = Qt.calibrate_device(sd, synth_frames(4, 128, 128, 900), batch=3)   # batches of 3 + 1 frames
    Qt.validate(qp)
    e = Engine(pack_int8(sd, qp), 'cuda:0')
    try:
        fr = synth_frames(2, 64, 64, 11)
        o, p = e.forward(torch.from_numpy(fr).cuda())
        ro, rp = Q.int8_forward(fr, sd, qp)
        np.testing.assert_array_equal(o.cpu().numpy(), ro)
        np.testing.assert_array_equal(p.cpu().numpy(), rp)
        fr = synth_frames(2, 96, 96, 5)
        o, p = e.forward(torch.from_numpy(fr).cuda())
        fo, fp = Q.fake_quant_forward(fr, sd, qp)
        assert np.abs(o.cpu().numpy() - fo.numpy()).max() < 0.05 * np.abs(fo.numpy()).max()
        fr = synth_frames(2, 128, 128, 77)
        o, p = e.forward(torch.from_numpy(fr).cuda())
        ro, rp = M.forward(M.u8_nhwc_to_nchw_f32(fr), sd)
        assert np.abs(o.cpu().numpy() - ro.numpy()).max() < 0.06 * np.abs(ro.numpy()).max()
        assert np.abs(p.cpu().numpy() - rp.numpy()).max() < 0.1 * np.abs(rp.numpy()).max()
    finally:
        e.close()
    # the image tap sees the same values on both sides, so its scale is the host twin's exactly; an iterable of
    # batches (device tensors or arrays) gives the statistics of the array
    fr = synth_frames(4, 128, 128, 900)
    c, h = Qt.observe_host(fr.astype(np.float32) / np.float32(255))
    assert qp['image'] == max(Qt._hist_percentile(c, h, 99.999), 1e-8) / 127
    qp2 = Qt.calibrate_device(sd, [torch.from_numpy(fr[:1]).cuda(), fr[1:]], method='mse')
    Qt.validate(qp2)
    assert qp2['image'] == Qt._hist_mse_clip(c, h, 127) / 127
    assert Qt.calibrate_device(sd, fr, method='max')['image'] == float((fr.astype(np.float32) / np.float32(255)).max()) / 127


def test_build_tool_device_calibration(tmp_path):
    from spef_amd.tools import build_mi355x
    out = str(tmp_path / 'int8_device')
    rc = build_mi355x.main(['--synthetic', '--dtype', 'int8', '--calib', 'device', '--calib-frames', '4',
                            '--eval-variants', 'none', '--out', out])
    assert rc == 0
    with open(out + '/qparams.json') as f:
        qp = json.load(f)
    assert qp['image'] > 0 and len(qp['blocks']) == N_BLOCKS and qp['blocks'][0]['quant'] is None
    with open(out + '/build.json') as f:
        info = json.load(f)
    cal = info['calibration']
    assert cal['where'] == 'device' and cal['method'] == 'percentile' and cal['frames'] == 4 and cal['seconds'] > 0
