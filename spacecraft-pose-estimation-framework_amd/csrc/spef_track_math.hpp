// Quaternion helpers of the pose tracker and the pose smoother (k_track.hip, k_smooth.hip): the arithmetic of
// spef_amd/spe/track.py's qmul / qexp / _unit, in fp64, with the hardware-estimate + Newton reciprocal and square root
// of spef_pose_math.hpp.
#pragma once
#include <math.h>

#include "spef_common.hpp"
#include "spef_pose_math.hpp"

namespace spef {

enum : int { TS_INVALID = 1, TS_GATED = 2, TS_REINIT = 4, TS_NO_TRACK = 8 };

// Hamilton product, scalar first: R(a (x) b) = R(a) R(b)
__device__ __forceinline__ void track_qmul(const double (&a)[4], const double (&b)[4], double (&o)[4]) {
  o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}

// the quaternion of the rotation vector w (series below |w|^2 = 1e-16)
__device__ __forceinline__ void track_qexp(const double (&w)[3], double (&o)[4]) {
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double c = 1.0 - th2 / 8.0, s = 0.5 - th2 / 48.0;
  if (!(th2 < 1e-16)) {
    const double th = dsqrt(th2);
    double sh;
    sincos(0.5 * th, &sh, &c);
    s = sh * rcp_nr(th);
  }
  o[0] = c;
  o[1] = s * w[0];
  o[2] = s * w[1];
  o[3] = s * w[2];
}

__device__ __forceinline__ void track_unit(double (&q)[4]) {
  const double inv = rsq_nr(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] *= inv;
}

// o = exp(w) (x) q, normalised, in the hemisphere of ref
__device__ __forceinline__ void track_rotate(const double (&w)[3], const double (&q)[4], const double (&ref)[4],
                                             double (&o)[4]) {
  double e[4];
  track_qexp(w, e);
  track_qmul(e, q, o);
  track_unit(o);
  if (o[0] * ref[0] + o[1] * ref[1] + o[2] * ref[2] + o[3] * ref[3] < 0.0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = -o[k];
  }
}

__device__ __forceinline__ bool track_finite(double x) { return fabs(x) < INFINITY; }

// The rotation vector of the unit quaternion a (x) conj(b), |angle| <= pi: the Log of the tracker's innovation (the
// difference flipped to a scalar part >= 0; series below |v| = 1e-8).
__device__ __forceinline__ void track_qlog_diff(const double (&a)[4], const double (&b)[4], double (&o)[3]) {
  const double bc[4] = {b[0], -b[1], -b[2], -b[3]};
  double d[4];
  track_qmul(a, bc, d);
  if (d[0] < 0.0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = -d[k];
  }
  const double n2 = d[1] * d[1] + d[2] * d[2] + d[3] * d[3];
  const double n = dsqrt(n2);
  const double fl = n < 1e-8 ? 2.0 / d[0] * (1.0 - n2 / (3.0 * d[0] * d[0])) : 2.0 * atan2(n, d[0]) * rcp_nr(n);
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] = fl * d[1 + k];
}

}  // namespace spef
