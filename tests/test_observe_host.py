"""Histogram observers on the host: the statistic (``quant.observe_host``, the twin of csrc/k_observe.hip), the scales
taken from it (``quant.scales_from_stats``) against the exact order statistics and ``_mse_clip`` on the raw
activations, and ``calibrate`` on top of ``quant.taps``."""
import ctypes as C

import numpy as np
import pytest

from bench import synth_frames
from spef_amd import quant as Qt
from spef_amd.arch import mobilenet_v2
from spef_amd.blob_q8 import pack_int8
from spef_amd.weights import synthetic_state_dict


def f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


LO, HI = 103 << 23, 135 << 23


def special_values():
    """-> (values float32, expectation per value: 'under' | 'over' | 'nonfinite' | bin index), positive halves only;
    the caller adds the negative twins."""
    edge = LO + (1000 << 15)   # the lower edge of bin 1000
    cases = [
        (np.float32(0.0), 'under'),
        (f32(1), 'under'),                       # the smallest denormal
        (f32(0x007fffff), 'under'),              # the largest denormal
        (f32(LO - 1), 'under'),                  # the float just below 2^-24
        (f32(LO), 0),                            # 2^-24: the first bin
        (np.float32(1.0), (127 - 103) * 256),
        (f32(edge - 1), 999),
        (f32(edge), 1000),
        (f32(edge + 1), 1000),
        (np.float32(255.999), 8191),
        (f32(HI - 1), 8191),                     # the float just below 2^8
        (np.float32(256.0), 'over'),
        (np.float32(3.0e38), 'over'),
        (np.float32(np.inf), 'nonfinite'),
        (np.float32(np.nan), 'nonfinite'),
    ]
    return cases


def test_observe_host_special_values():
    assert f32(LO) == np.float32(2.0 ** -24) and f32(HI) == np.float32(256.0)
    cases = special_values()
    for sign in (1.0, -1.0):
        for v, want in cases:
            x = np.array([np.float32(sign) * v], np.float32)
            c, h = Qt.observe_host(x)
            assert c[Qt.N_TOTAL] == 1
            got = ('under' if c[Qt.N_UNDER] else 'over' if c[Qt.N_OVER] else 'nonfinite' if c[Qt.N_NONFINITE] else
                   int(np.nonzero(h)[0][0]))
            assert got == want, (sign, v, got, want)
            assert int(c[Qt.N_UNDER] + c[Qt.N_OVER] + c[Qt.N_NONFINITE] + h.sum()) == 1
            assert int(c[Qt.MAX_BITS]) == (0 if want == 'nonfinite' else bits(v))
            assert not c[5:].any()
    # all together: -0.0 too, the max over the finite values, the total equal to the sum of the parts
    allv = np.array([s * v for s in (1, -1) for v, _ in cases] + [-0.0], np.float32)
    c, h = Qt.observe_host(allv)
    assert int(c[Qt.N_TOTAL]) == allv.size == int(c[Qt.N_UNDER] + c[Qt.N_OVER] + c[Qt.N_NONFINITE] + h.sum())
    assert int(c[Qt.N_UNDER]) == 9 and int(c[Qt.N_OVER]) == 4 and int(c[Qt.N_NONFINITE]) == 4
    assert int(c[Qt.MAX_BITS]) == bits(np.float32(3.0e38))
    assert h[1000] == 4 and h[999] == 2 and h[8191] == 4 and h[0] == 2
    # several tensors accumulate; torch tensors are taken as well
    import torch
    c2, h2 = Qt.observe_host([allv[:7], torch.from_numpy(allv[7:])])
    np.testing.assert_array_equal(c, c2)
    np.testing.assert_array_equal(h, h2)


def test_bin_edges():
    e = Qt.bin_edges()
    assert e.dtype == np.float32 and e.shape == (Qt.OBS_BINS + 1,)
    assert e[0] == np.float32(2.0 ** -24) and e[-1] == np.float32(256.0)
    k = np.arange(Qt.OBS_BINS)
    np.testing.assert_array_equal(e[1:].view(np.uint32), ((k + 1) << 15) + LO)
    assert (e[1:].astype(np.float64) / e[:-1] - 1).max() <= 2.0 ** -8


@pytest.fixture(scope='module')
def sd():
    return synthetic_state_dict(mobilenet_v2(), seed=1001)


@pytest.fixture(scope='module')
def stats128(sd):
    """Per tap of the 4 x 128 x 128 calibration frames: name, |x| (float32, all tensors of the tap), its statistic."""
    out = {}
    for tap, name, ts in Qt.taps(sd, synth_frames(4, 128, 128, 900)):
        v = np.abs(np.concatenate([t.numpy().reshape(-1) for t in ts]))
        out[tap] = (name, v, Qt.observe_host(ts))
    return out


def test_taps_cover_every_quantizer(stats128):
    ids = Qt.tap_ids()
    assert len(ids) == 4 + 3 * 17 and sorted(ids.values()) == list(range(55))
    absent = {ids['blocks.1.quant'], ids['blocks.1.expand']}
    assert set(stats128) == set(ids.values()) - absent
    for tap, (name, _, _) in stats128.items():
        assert ids[name] == tap


def test_histogram_percentile_brackets_order_statistic(stats128):
    """v = the exact order statistic of rank ceil(p / 100 (n - 1)) of |x|; the histogram percentile h is the upper edge
    of v's bin capped at the max, so v <= h <= v (1 + 2^-8)."""
    worst = 0.0
    for tap, (name, v, (c, h)) in stats128.items():
        assert int(c[Qt.N_OVER]) == 0 and int(c[Qt.N_NONFINITE]) == 0, name
        assert int(c[Qt.N_TOTAL]) == v.size
        for p in (99.0, 99.9, 99.999):
            r = int(np.ceil(p / 100.0 * (v.size - 1)))
            exact = float(np.partition(v, r)[r])
            got = Qt._hist_percentile(c, h, p)
            assert exact > 0, (name, p)
            assert exact <= got <= exact * (1 + 2.0 ** -8), (name, p, exact, got)
            worst = max(worst, got / exact)
    print(f'worst histogram percentile / exact order statistic: {worst:.6f}')


def test_histogram_mse_clip_close_to_exact(sd):
    """The clip found on the histogram costs at most 1 % more quantisation MSE, on the exact values, than the clip
    ``_mse_clip`` finds on the values themselves (unsigned quantizers of 8 and 3 bits)."""
    def mse(v, clip, levels):
        sc = clip / levels
        return float(np.mean((np.clip(np.rint(v / sc), 0, levels) * sc - v) ** 2))
    worst = 0.0
    for tap, name, ts in Qt.taps(sd, synth_frames(2, 96, 96, 900)):
        v = np.concatenate([t.numpy().reshape(-1) for t in ts]).astype(np.float64)
        v = np.abs(v)   # unsigned quantizer: every tap as magnitudes
        c, h = Qt.observe_host([np.abs(t.numpy()) for t in ts])
        for levels in (255, 7):
            ref = Qt._mse_clip(v, levels, False)
            got = Qt._hist_mse_clip(c, h, levels)
            e_ref, e_got = mse(v, ref, levels), mse(v, got, levels)
            assert e_got <= 1.01 * e_ref, (name, levels, e_got / e_ref)
            worst = max(worst, e_got / e_ref)
    print(f'worst MSE excess of the histogram clip: {worst - 1:.5f}')


@pytest.mark.parametrize('method', ['percentile', 'mse', 'max'])
@pytest.mark.parametrize('widths', ['all8', 'qmobilenet_default'])
def test_scales_from_stats_pack(sd, stats128, method, widths):
    from spef_amd import _lib as L
    bw = Qt.BitWidths() if widths == 'all8' else Qt.BitWidths.qmobilenet_default()
    counters = np.zeros((55, 8), np.uint64)
    hist = np.zeros((55, Qt.OBS_BINS), np.uint64)
    for tap, (_, _, (c, h)) in stats128.items():
        counters[tap], hist[tap] = c, h
    qp = Qt.scales_from_stats(counters, hist, bw, method=method)
    Qt.validate(qp)
    assert qp['bits'] == bw
    blob = pack_int8(sd, qp)
    lib = L.load()
    dt = C.c_int()
    buf = C.create_string_buffer(blob, len(blob))
    assert lib.spef_validate_blob(buf, len(blob), C.byref(dt), None, None, None) == 0, lib.spef_last_error()
    assert dt.value == 3
    if method == 'percentile' and widths == 'all8':
        # np.percentile interpolates between the ranks below and above p; the histogram takes the upper rank's bin edge
        ref = Qt.calibrate(sd, synth_frames(4, 128, 128, 900), bw=bw)
        for k in ('image', 'stem', 'final', 'last'):
            assert ref[k] <= qp[k] * (1 + 1e-6), k
    if method == 'max':
        for tap, (name, v, _) in stats128.items():
            if name == 'last':
                assert qp['last'] == float(v.max()) / Qt.uint_levels(bw.last_conv[1])


def test_scales_from_stats_edge_cases():
    counters = np.zeros(8, np.uint64)
    hist = np.zeros(Qt.OBS_BINS, np.uint64)
    assert Qt._hist_percentile(counters, hist, 99.0) == 0.0            # an empty tap
    assert Qt._hist_mse_clip(counters, hist, 255) == 1e-8
    c, h = Qt.observe_host(np.zeros(100, np.float32))                   # all zeros: the rank falls in the underflow
    assert Qt._hist_percentile(c, h, 99.999) == 0.0
    c, h = Qt.observe_host(np.array([0.0] * 10 + [300.0] * 90, np.float32))   # the rank falls in the overflow
    assert Qt._hist_percentile(c, h, 99.0) == 300.0
    c, h = Qt.observe_host(np.array([1.0] * 99 + [np.nan], np.float32))       # non-finite values hold no rank
    assert Qt._hist_percentile(c, h, 100.0) == 1.0


def test_calibrate_on_taps_keeps_its_values(sd):
    """``calibrate`` is written on top of ``taps``; these are the values it returned before."""
    fr = synth_frames(2, 64, 64, 900)
    pins = {
        'percentile': (0.007194688939672756, 0.023318028448142156, 0.01865321563393457, 0.035992908257197476,
                       0.014649084455565833, 0.013712645656108734, 0.02009105226396576, 0.01045566052044469,
                       0.006499805436938417),
        'mse': (0.007194688939672756, 0.022923557468489106, 0.018687824174469594, 0.03367115178446132,
                0.014510212449466483, 0.0137267645667581, 0.02009838209377499, 0.01035305021316048,
                0.006436854138093837),
    }
    for method, want in pins.items():
        qp = Qt.calibrate(sd, fr, method=method)
        Qt.validate(qp)
        got = (qp['image'], qp['stem'], qp['blocks'][0]['dw'], qp['blocks'][2]['quant'], qp['blocks'][2]['expand'],
               qp['blocks'][9]['dw'], qp['blocks'][16]['quant'], qp['final'], qp['last'])
        assert got == want, method
        assert qp['blocks'][0]['quant'] is None and qp['blocks'][0]['expand'] is None
