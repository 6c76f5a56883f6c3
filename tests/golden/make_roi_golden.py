"""Record tests/golden/roi.npz from the REFERENCE's KeyPoints.project and create_bbox_from_keypoints (build container
only).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_roi_golden.py <reference checkout>

The reference's ``KeyPoints`` (src/spe/keypoints_utils.py) is imported from the checkout, read-only, with an empty
in-memory stand-in for cv2 (absent here; neither function calls it), and run on the first 10 poses of its valid.json
with the SPEED camera (no distortion) and the next 10 with the SPEED+ camera (radial + tangential distortion); the
camera objects are spef_amd.spe.camera's, which carry the attributes the reference's Camera classes do (their dataset
modules import packages that are absent here):
  q [20 x 4], t [20 x 3] float32  the poses;  plus [20] bool  which camera
  px   [20 x 12 x 2] float64  project(q, t): pixels of the origin and the 11 model points
  bbox [20 x 4]      float64  create_bbox_from_keypoints(create_keypoints2d(q, t)): normalised (xmin, ymin, xmax, ymax)
  kp3d, K, K_plus, dist, nu, nv  the model points and the two cameras
The box rule's twin (spef_amd/spe/roi.py) must reproduce px and, before its margin, bbox. No reference source is copied.
"""
import json
import os
import sys
import types

import numpy as np


def main(ref_root):
    sys.dont_write_bytecode = True
    sys.modules.setdefault('cv2', types.ModuleType('cv2'))
    sys.path.insert(0, ref_root)
    from src.spe.keypoints_utils import KeyPoints

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))),
                                    'spacecraft-pose-estimation-framework_amd'))
    from spef_amd.spe.camera import SpeedCamera, SpeedPlusCamera   # the reference's Camera attributes (K, nu, nv, distCoeffs)

    cams = [SpeedCamera(), SpeedPlusCamera()]
    mat = os.path.join(ref_root, 'models', '3d_models', 'tangoPoints.mat')
    kps = [KeyPoints(c, mat) for c in cams]
    valid = json.load(open(os.path.join(ref_root, 'src', 'data', 'datasets', 'speed_split', 'valid.json')))[:20]
    q = np.array([v['q_vbs2tango'] for v in valid], np.float32)
    t = np.array([v['r_Vo2To_vbs_true'] for v in valid], np.float32)
    plus = np.arange(20) >= 10
    # the float32 poses are handed over as float64 (the same values): the reference's quat2dcm computes in the dtype of
    # its argument, and the ROI path's arithmetic is float64
    q64, t64 = q.astype(np.float64), t.astype(np.float64)
    px = np.stack([kps[int(plus[i])].project(q64[i], t64[i]).T for i in range(20)])
    bbox = np.stack([kps[int(plus[i])].create_bbox_from_keypoints(kps[int(plus[i])].create_keypoints2d(q64[i], t64[i]))
                     for i in range(20)])
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'roi.npz')
    np.savez(out, q=q, t=t, plus=plus, px=px.astype(np.float64), bbox=bbox.astype(np.float64), kp3d=kps[0].keypoints3d,
             K=np.asarray(cams[0].K, np.float64), K_plus=np.asarray(cams[1].K, np.float64),
             dist=np.asarray(cams[1].distCoeffs, np.float64), nu=cams[0].nu, nv=cams[0].nv)
    print(out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1])
