"""Record tests/golden/decode_cov.npz from the REFERENCE's orientation decode (build container only).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cov_golden.py <reference checkout>

``OrientationSoftClassification.decode`` (src/spe/classification_utils.py:113-147) returns ``(q_avg, h_inv)`` with
``h_inv = inv(a)``, a = sum_i p_i q_i q_i^T; ``SPEUtils.decode`` drops the second value (spe_utils.py:97). This script
imports the reference read-only (the stubs of make_golden.py for the packages absent here), runs that decode and keeps
the second value:
  rand_hinv     [16 x 4 x 4] float32  of the 16 ``rand_soft`` rows already in decode_ori.npz
  planted_soft  [3 x 4 x 1728] float32  ``SPEUtils.last_activ`` (the softmax) of the first 4 ``planted_logits`` rows of
                                        decode_ori.npz per temperature (T = 1, 0.5, 0.2). The PDFs themselves are stored:
                                        inverting a amplifies an ulp of a re-derived softmax by cond(a).
  planted_hinv  [3 x 4 x 4 x 4] float32  their h_inv (NaN where np.linalg.inv raised LinAlgError)
  planted_raised [3 x 4] bool
  temps         [3] float32
No reference source is copied.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def main(ref_root):
    from make_golden import _install_stubs
    _install_stubs()
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref_root)
    from src.spe.spe_utils import SPEUtils
    from src.data.datasets.speed import Camera
    su = SPEUtils(Camera(), 'classification', 12, 3, False, 'classification', 10, 100, None)
    g = np.load(os.path.join(HERE, 'decode_ori.npz'), allow_pickle=False)
    assert np.array_equal(su.orientation.histogram, g['hist'])
    rand_hinv = np.stack([su.orientation.decode(p)[1] for p in g['rand_soft']])
    temps, n = g['temps'], 4
    soft = np.empty((len(temps), n, 1728), np.float32)
    hinv = np.full((len(temps), n, 4, 4), np.nan, np.float32)
    raised = np.zeros((len(temps), n), bool)
    for ti in range(len(temps)):
        lg = g['planted_logits'][ti, :n]
        soft[ti] = su.last_activ({'ori_soft': lg.copy(), 'pos_soft': np.zeros((n, 1000), np.float32)})['ori_soft']
        for i in range(n):
            try:
                hinv[ti, i] = su.orientation.decode(soft[ti, i])[1]
            except np.linalg.LinAlgError:
                raised[ti, i] = True
    out = os.path.join(HERE, 'decode_cov.npz')
    np.savez_compressed(out, rand_hinv=rand_hinv, planted_soft=soft, planted_hinv=hinv, planted_raised=raised,
                        temps=temps)
    print(out, os.path.getsize(out), 'bytes;', 'raised:', int(raised.sum()), 'dtype', rand_hinv.dtype)


if __name__ == '__main__':
    main(sys.argv[1])
