"""The head-fit twin (spef_amd/solver/head_fit.py) against the reference's loss, torch's autograd and torch's optimizers
(tests/golden/head_fit.npz, float64 against float64), its encoders against the reference's (encode.npz, decode_pos.npz),
``blob.replace_head``, and the argument checks of the new entry points that need no device."""
import ctypes as C

import numpy as np
import pytest

from oracle import decode_ref as D
from spef_amd import _lib as L
from spef_amd import blob
from spef_amd.solver import head_fit as HF

N_ORI = 37
# tests/golden/make_headfit_golden.py CASES / SGD / ADAM
CASES = {'cc_b1': ('classification', False, 1.0), 'cc_b05': ('classification', False, 0.5),
         'cr_b1': ('regression', False, 1.0), 'cr_norm_b05': ('regression', True, 0.5)}
OPTS = {'sgd': dict(lr=0.05, momentum=0.9, weight_decay=1e-4), 'adam': dict(lr=0.01, weight_decay=1e-4)}
RTOL = 1e-12


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.max(np.abs(a - b))
    scale = np.max(np.abs(b))
    print(f'{what}: max |d| = {err:.3e} at scale {scale:.3e}')
    assert err <= RTOL * scale, what


@pytest.mark.parametrize('name', list(CASES))
def test_loss_and_gradients_match_autograd(golden, name):
    g = golden('head_fit.npz')
    pos_mode, norm, beta = CASES[name]
    X = g[f'{name}_X']
    W = np.concatenate([g[f'{name}_wo'], g[f'{name}_wp']])
    b = np.concatenate([g[f'{name}_bo'], g[f'{name}_bp']])
    z = HF.forward(X, W, b)
    (total, lo, lp), G = HF.loss_and_g(z[:, :N_ORI], g[f'{name}_to'], z[:, N_ORI:], g[f'{name}_tp'], beta, pos_mode, norm)
    assert abs(total - float(g[f'{name}_loss'])) <= RTOL * abs(float(g[f'{name}_loss']))
    assert abs(total - (beta * lo + lp)) <= 1e-15 * abs(total)
    dW, db = HF.gradients(G, X, X, N_ORI)
    _close(dW[:N_ORI], g[f'{name}_gwo'], 'dW ori')
    _close(dW[N_ORI:], g[f'{name}_gwp'], 'dW pos')
    _close(db[:N_ORI], g[f'{name}_gbo'], 'db ori')
    _close(db[N_ORI:], g[f'{name}_gbp'], 'db pos')


@pytest.mark.parametrize('opt', list(OPTS))
@pytest.mark.parametrize('name', list(CASES))
def test_optimizer_steps_match_torch(golden, name, opt):
    g = golden('head_fit.npz')
    pos_mode, norm, beta = CASES[name]
    o = dict(OPTS[opt])
    lr = o.pop('lr')
    n_pos = g[f'{name}_wp'].shape[0]
    tw = HF.HeadFitTwin(48, N_ORI, n_pos, optimizer=opt, pos_mode=pos_mode, beta=beta, norm_distance=norm, **o)
    tw.set_weights(np.concatenate([g[f'{name}_wo'], g[f'{name}_wp']]), np.concatenate([g[f'{name}_bo'], g[f'{name}_bp']]))
    for s in range(3):
        loss = tw.step(g[f'{name}_X'], g[f'{name}_to'], g[f'{name}_tp'], lr)
        ref = float(g[f'{name}_{opt}_loss'][s])
        assert abs(loss[0] - ref) <= RTOL * abs(ref), (s, loss[0], ref)
        _close(tw.W, g[f'{name}_{opt}_w'][s], f'W after step {s + 1}')
        _close(tw.b, g[f'{name}_{opt}_b'][s], f'b after step {s + 1}')


def test_float32_optimizer_is_one_rounding_per_operation():
    """The float32 twin is NumPy float32 arithmetic (what the device reproduces bit for bit from the same gradient): it
    stays within a few float32 ulps of the float64 twin over one step, and keeps float32 state."""
    rng = np.random.Generator(np.random.PCG64(7))
    w, g = rng.standard_normal(1000), rng.standard_normal(1000) * 0.1
    for step64, step32 in ((lambda a, c: HF.sgd_step(a, np.zeros_like(a), c, 0.05, 0.9, 1e-4)[0],) * 2,
                           (lambda a, c: HF.adam_step(a, np.zeros_like(a), np.zeros_like(a), c, 0.01, 1,
                                                      weight_decay=1e-4)[0],) * 2):
        a64 = step64(w, g)
        a32 = step32(w.astype(np.float32), g.astype(np.float32))
        assert a32.dtype == np.float32
        assert np.max(np.abs(a32 - a64)) <= 8 * np.finfo(np.float32).eps * np.max(np.abs(w))


def test_encode_matches_reference(golden):
    g = golden('encode.npz')
    h, red = D.orientation_histogram(12, False)
    enc = HF.encode_orientation(g['q'], h, HF.soft_variance(3, 12), red)
    np.testing.assert_allclose(enc, g['enc'], rtol=1e-6, atol=1e-9)
    gp = golden('decode_pos.npz')
    encp = HF.encode_position(gp['enc_t'], D.position_histogram(10), HF.soft_variance(100, 10))
    np.testing.assert_allclose(encp, gp['enc'], rtol=1e-6, atol=1e-9)


def test_encode_flags_bad_rows():
    h, red = D.orientation_histogram(12, False)
    q = np.array([[1.0, 0, 0, 0], [np.nan, 0, 0, 0], [0, 1.0, 0, 0]])
    enc = HF.encode_orientation(q, h, HF.soft_variance(3, 12), red)
    assert np.all(np.isnan(enc[1])) and np.all(np.isfinite(enc[[0, 2]]))
    assert np.all(enc[0][red] == 0) and abs(float(enc[0].astype(np.float64).sum()) - 1) < 1e-5


def test_dropout_hash_is_stated_and_fair():
    idx = np.arange(1 << 16, dtype=np.uint64)
    h = HF.dropout_hash(5, 3, idx)
    assert h.dtype == np.uint32 and len(np.unique(h)) == len(h)          # the finaliser is a bijection of the mixed word
    assert int(HF.dropout_hash(0, 0, 0)) == 0                             # fmix32(0) = 0: the one fixed point
    assert not np.array_equal(h, HF.dropout_hash(5, 4, idx)) and not np.array_equal(h, HF.dropout_hash(6, 3, idx))
    for p in (0.2, 0.5):
        keep = HF.dropout_keep(11, 2, 64, 128, p)
        n = keep.size
        assert abs(keep.mean() - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n)
        X = np.ones((64, 128), np.float32)
        Xd = HF.dropout_apply(X, keep, p)
        assert np.all(Xd[~keep] == 0) and np.all(Xd[keep] == np.float32(1.0 / (1.0 - p)))


# ------------------------------------------------------------------------------------------------------ replace_head
def _blob():
    from spef_amd.arch import mobilenet_v2
    from spef_amd.weights import synthetic_state_dict
    return blob.pack(synthetic_state_dict(mobilenet_v2('ursonet', 40, 8), seed=3), dtype='fp32')


def test_replace_head_round_trips_through_validation():
    b0 = _blob()
    rng = np.random.Generator(np.random.PCG64(9))
    wo, bo = rng.standard_normal((40, 1280)).astype(np.float32), rng.standard_normal(40).astype(np.float32)
    wp, bp = rng.standard_normal((8, 1280)).astype(np.float32), rng.standard_normal(8).astype(np.float32)
    b1 = blob.replace_head(b0, wo, bo, wp, bp)
    assert len(b1) == len(b0) and b1 != b0
    lib = L.load()
    dt, head, n0, n1 = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    buf = C.create_string_buffer(b1, len(b1))
    assert lib.spef_validate_blob(buf, len(b1), C.byref(dt), C.byref(head), C.byref(n0), C.byref(n1)) == L.OK
    assert (dt.value, head.value, n0.value, n1.value) == (4, 0, 40, 8)
    info = blob.describe(b1)
    fc = [o for o in info['ops'] if o[0] == blob.OP_FC][0]
    w = np.frombuffer(b1, np.float32, 48 * 1280, info['data_off'] + fc[8]).reshape(48, 1280)
    bias = np.frombuffer(b1, np.float32, 48, info['data_off'] + fc[9])
    assert np.array_equal(w[:40], wo) and np.array_equal(w[40:], wp)
    assert np.array_equal(bias[:40], bo) and np.array_equal(bias[40:], bp)
    # only the two FC tensors differ
    a0, a1 = np.frombuffer(b0, np.uint8), np.frombuffer(b1, np.uint8)
    diff = np.flatnonzero(a0 != a1)
    lo_w, lo_b = info['data_off'] + fc[8], info['data_off'] + fc[9]
    assert np.all(((diff >= lo_w) & (diff < lo_w + 48 * 1280 * 4)) | ((diff >= lo_b) & (diff < lo_b + 48 * 4)))
    # and putting the old head back restores the blob
    w0 = np.frombuffer(b0, np.float32, 48 * 1280, lo_w).reshape(48, 1280)
    bias0 = np.frombuffer(b0, np.float32, 48, lo_b)
    assert blob.replace_head(b1, w0[:40], bias0[:40], w0[40:], bias0[40:]) == b0


def test_replace_head_refuses_wrong_shapes():
    b0 = _blob()
    z = np.zeros
    with pytest.raises(ValueError):
        blob.replace_head(b0, z((41, 1280)), z(41), z((8, 1280)), z(8))
    with pytest.raises(ValueError):
        blob.replace_head(b0, z((40, 1280)), z(40), z((8, 1264)), z(8))


# ------------------------------------------------------------------------------------------------------ argument checks
def test_entry_points_refuse_null_handles():
    lib = L.load()
    prm = L.HeadFitParams(L.CLASSIFICATION, L.CLASSIFICATION, L.HEADFIT_SGD, 0, 8, 0, 1.0, 0.9, 0.9, 0.999, 1e-8, 0, 0)
    h = C.c_void_p()
    assert lib.spef_headfit_create(None, 16, 5, 8, C.byref(prm), C.byref(h)) == L.ERR_ARG
    assert lib.spef_headfit_step(None, None, None, None, 1, None, 1, None, None, None, None) == L.ERR_ARG
    assert lib.spef_headfit_set_weights(None, None, None, None) == L.ERR_ARG
    assert lib.spef_headfit_get_weights(None, None, None, None) == L.ERR_ARG
    assert lib.spef_headfit_get_state(None, None, None, None, None, None) == L.ERR_ARG
    assert lib.spef_headfit_get_g(None, 1, None, None) == L.ERR_ARG
    assert lib.spef_headfit_reset_state(None, None) == L.ERR_ARG
    assert lib.spef_headfit_load_model(None, None, None) == L.ERR_ARG
    assert lib.spef_headfit_commit(None, None, None) == L.ERR_ARG
    assert lib.spef_headfit_destroy(None) == L.OK
    assert lib.spef_features(None, None, 0, 1, 64, 64, None, None) == L.ERR_ARG
    ep = L.EncodeParams(1.0, 1.0)
    assert lib.spef_encode_targets(None, None, None, 1, C.byref(ep), None, None, None, None, None) == L.ERR_ARG
    assert b'null' in lib.spef_last_error()
