// fp64 helpers shared by the keypoint decode kernels: the batched EPnP (k_epnp.hip), the 3-point consensus
// (k_consensus.hip) and the pose refinement (k_refine.hip) behind it -- reciprocal / square root from the hardware estimates, cv::undistortPoints, dcm2quat.
#pragma once

#include <math.h>

#include "spef_common.hpp"
#include "spef_kernels.hpp"

namespace spef {

#define EPNP_MAXN 16

// Reciprocal and reciprocal square root: the hardware fp64 estimates (v_rcp_f64 / v_rsq_f64) refined by Newton steps
// instead of the IEEE-correct library sequences (scaling, fixup): within an ulp or two, on one lane's critical path.
__device__ __forceinline__ double rcp_nr(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(r, fma(-x, r, 1.0), r);
  return fma(r, fma(-x, r, 1.0), r);
}
__device__ __forceinline__ double rsq_nr(double x) {   // x > 0
  double r = __builtin_amdgcn_rsq(x);
  const double h = 0.5 * x;
  r = r * fma(-h * r, r, 1.5);
  return r * fma(-h * r, r, 1.5);
}
// Division and square root in the small serial solves (QR least squares, Gauss-Newton, Procrustes): the same
// hardware-estimate + Newton forms (a x (1/b) is within an ulp or two of a / b, against ~15 dependent instructions of
// the IEEE division sequence on one lane's critical path).
__device__ __forceinline__ double ddiv(double a, double b) { return a * rcp_nr(b); }
__device__ __forceinline__ double dsqrt(double x) { return x > 0.0 ? x * rsq_nr(x) : 0.0; }   // x >= 0
// cv::undistortPoints as solvePnP(SOLVEPNP_EPNP) applies it before EPnP (OpenCV 4.5.5 solvepnp.cpp;
// undistort.dispatch.cpp cvUndistortPointsInternal, default criteria COUNT = 5) followed by epnp::init_points'
// re-projection with K: x = (u - cx) * (1/fx); five fixed-point steps x <- (x0 - delta(x)) * icdist(x) (5-coefficient
// model: k1 k2 p1 p2 k3); the normalised point is stored as float32 (the reference's points are float32) and
// re-projected in double, us = x fu + uc. Without distortion only that float32 round trip remains (the reference
// always passes distCoeffs, zeros for SPEED: keypoints_utils.py:136-142).
__device__ __forceinline__ void undistort_point(const EpnpDist& d, double fu, double fv, double uc, double vc,
                                                float uf, float vf, double& u_out, double& v_out) {
  const double ifx = 1.0 / fu, ify = 1.0 / fv;
  const double x0 = ((double)uf - uc) * ifx, y0 = ((double)vf - vc) * ify;
  double x = x0, y = y0;
  if (d.on) {
    for (int it = 0; it < 5; ++it) {
      const double r2 = x * x + y * y;
      const double icdist = 1.0 / (1.0 + ((d.k3 * r2 + d.k2) * r2 + d.k1) * r2);
      if (icdist < 0) {
        x = x0;
        y = y0;
        break;
      }
      const double dx = 2 * d.p1 * x * y + d.p2 * (r2 + 2 * x * x);
      const double dy = d.p1 * (r2 + 2 * y * y) + 2 * d.p2 * x * y;
      x = (x0 - dx) * icdist;
      y = (y0 - dy) * icdist;
    }
  }
  u_out = (double)(float)x * fu + uc;
  v_out = (double)(float)y * fv + vc;
}

// dcm2quat (spe/utils.py:56-118, Spurrier): q = the quaternion (scalar first) of the rotation matrix R, before the
// division by its norm (which is 1 up to R's distance from a rotation).
__device__ __forceinline__ void dcm2quat(const double (&R)[3][3], double (&q)[4]) {
  const double m11 = R[0][0], m12 = R[0][1], m13 = R[0][2];
  const double m21 = R[1][0], m22 = R[1][1], m23 = R[1][2];
  const double m31 = R[2][0], m32 = R[2][1], m33 = R[2][2];
  const double tr = m11 + m22 + m33;
  double q0, q1, q2, q3;
  if (tr > fmax(m11, fmax(m22, m33))) {
    q0 = sqrt(1 + tr) / 2;
    q1 = (m32 - m23) / (4 * q0); q2 = (m13 - m31) / (4 * q0); q3 = (m21 - m12) / (4 * q0);
  } else if (m11 > fmax(tr, fmax(m22, m33))) {
    q1 = sqrt(m11 / 2 + (1 - tr) / 4);
    q0 = (m32 - m23) / (4 * q1); q2 = (m21 + m12) / (4 * q1); q3 = (m31 + m13) / (4 * q1);
  } else if (m22 > fmax(tr, fmax(m11, m33))) {
    q2 = sqrt(m22 / 2 + (1 - tr) / 4);
    q0 = (m13 - m31) / (4 * q2); q3 = (m32 + m23) / (4 * q2); q1 = (m12 + m21) / (4 * q2);
  } else {
    q3 = sqrt(m33 / 2 + (1 - tr) / 4);
    q0 = (m21 - m12) / (4 * q3); q1 = (m13 + m31) / (4 * q3); q2 = (m23 + m32) / (4 * q3);
  }
  q[0] = q0;
  q[1] = q1;
  q[2] = q2;
  q[3] = q3;
}

}  // namespace spef
