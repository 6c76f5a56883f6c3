"""Record tests/golden/kalman_pos.npz from the REFERENCE's position Kalman filter (build container only).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_track_golden.py <reference checkout>

The reference's ``KalmanFilterPosSimple`` (src/temporal/kalman.py) is loaded from its file, read-only, and run with
dt = 1 as predict -> update per frame, initialised from the first measurement (whose output is the measurement):
  pos_in   [40 x 3] float64  a seeded noisy constant-velocity position track
  pos_out  [40 x 3] float64  the filter's position estimate after every frame
The pose tracker (spef_amd/spe/track.py) must reproduce pos_out when configured like it (q = p0 = 1, r = 100, no
gate, no covariance). No reference source is copied.
"""
import importlib.util
import os
import sys

import numpy as np


def main(ref_root):
    path = os.path.join(ref_root, 'src', 'temporal', 'kalman.py')
    spec = importlib.util.spec_from_file_location('reference_kalman', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(11)
    k = np.arange(40)[:, None]
    pos_in = np.array([0.2, -0.1, 9.0]) + k * np.array([0.004, -0.003, -0.03]) + rng.normal(0, [0.01, 0.01, 0.1], (40, 3))
    kf = mod.KalmanFilterPosSimple(1, pos_in[0])
    pos_out = np.empty_like(pos_in)
    pos_out[0] = pos_in[0]
    for i in range(1, 40):
        kf.predict()
        pos_out[i] = np.asarray(kf.update(np.matrix(pos_in[i]).T))[:3, 0]
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'kalman_pos.npz')
    np.savez(out, pos_in=pos_in, pos_out=pos_out)
    print(out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1])
