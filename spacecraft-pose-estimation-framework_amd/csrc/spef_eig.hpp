// Top eigenvector of a symmetric 4 x 4 matrix in fp64: the Markley average of the orientation decode (k_head.hip) and of
// every cluster of the multi-hypothesis decode (k_modes.hip).
#pragma once

#include <math.h>

#include "spef_common.hpp"

namespace spef {

// Top eigenvector of the symmetric PSD 4x4 a (fp64, packed upper triangle t) by repeated squaring: each step
// M <- M^2 multiplies the eigenvalue ratios (l_i / l_1) by themselves, so after k steps M is l_1-dominated to
// (l_2 / l_1)^(2^k); M is rescaled by a power of two each step (exact, no division) and the loop stops when M is
// rank one to fp64 precision (tr(M^2) = tr(M)^2), at most 40 steps. The eigenvector is M's column of largest
// diagonal entry, polished by two power steps with a. Replaces np.linalg.eig (classification_utils.py:137-141):
// <= 8 squarings after the Gershgorin shift below (<= 11 without it on every golden/random/near-uniform case; equal to
// numpy's eigenvector in float32), a short dependent chain of independent FMAs where cyclic Jacobi spent ~20 us of
// fp64 divides and square roots on one lane.
__device__ inline void sym4_top_eigvec(const double t[10], double out[4]) {
  // packed upper triangle: 0:00 1:01 2:02 3:03 4:11 5:12 6:13 7:22 8:23 9:33
  double m[10];
  {
    // shift by (just under) the Gershgorin lower bound g <= l_4 of a: the eigenvectors stay, every shifted
    // eigenvalue stays >= 0 and the ratio (l_2 - g) / (l_1 - g) < l_2 / l_1 -- near-flat softmaxes (a ~ I/4, the
    // slow case) converge in ~7 squarings instead of ~10; peaked ones have g <= 0 and keep sigma = 0
    const double g0 = t[0] - (fabs(t[1]) + fabs(t[2]) + fabs(t[3]));
    const double g1 = t[4] - (fabs(t[1]) + fabs(t[5]) + fabs(t[6]));
    const double g2 = t[7] - (fabs(t[2]) + fabs(t[5]) + fabs(t[8]));
    const double g3 = t[9] - (fabs(t[3]) + fabs(t[6]) + fabs(t[8]));
    const double sg = fmax(0.0, fmin(fmin(g0, g1), fmin(g2, g3))) * (1.0 - 0x1p-10);
#pragma unroll
    for (int k = 0; k < 10; ++k) m[k] = t[k];
    m[0] -= sg; m[4] -= sg; m[7] -= sg; m[9] -= sg;
    int e;
    frexp((m[0] + m[4]) + (m[7] + m[9]), &e);
#pragma unroll
    for (int k = 0; k < 10; ++k) m[k] = ldexp(m[k], -e);
  }
  for (int it = 0; it < 40; ++it) {
    const double m00 = m[0], m01 = m[1], m02 = m[2], m03 = m[3], m11 = m[4], m12 = m[5], m13 = m[6], m22 = m[7],
                 m23 = m[8], m33 = m[9];
    const double trm = (m00 + m11) + (m22 + m33);
    double q[10];
    q[0] = m00 * m00 + m01 * m01 + m02 * m02 + m03 * m03;
    q[1] = m00 * m01 + m01 * m11 + m02 * m12 + m03 * m13;
    q[2] = m00 * m02 + m01 * m12 + m02 * m22 + m03 * m23;
    q[3] = m00 * m03 + m01 * m13 + m02 * m23 + m03 * m33;
    q[4] = m01 * m01 + m11 * m11 + m12 * m12 + m13 * m13;
    q[5] = m01 * m02 + m11 * m12 + m12 * m22 + m13 * m23;
    q[6] = m01 * m03 + m11 * m13 + m12 * m23 + m13 * m33;
    q[7] = m02 * m02 + m12 * m12 + m22 * m22 + m23 * m23;
    q[8] = m02 * m03 + m12 * m13 + m22 * m23 + m23 * m33;
    q[9] = m03 * m03 + m13 * m13 + m23 * m23 + m33 * m33;
    const double tr = (q[0] + q[4]) + (q[7] + q[9]);
    int e;
    frexp(tr, &e);
#pragma unroll
    for (int k = 0; k < 10; ++k) m[k] = ldexp(q[k], -e);
    if (tr >= (1.0 - 1e-15) * (trm * trm)) break;   // M was rank one: tr(M^2) = tr(M)^2
  }
  // column of the largest diagonal entry (static indices only: no scratch)
  double v[4] = {m[0], m[1], m[2], m[3]}, bd = m[0];
  if (m[4] > bd) { bd = m[4]; v[0] = m[1]; v[1] = m[4]; v[2] = m[5]; v[3] = m[6]; }
  if (m[7] > bd) { bd = m[7]; v[0] = m[2]; v[1] = m[5]; v[2] = m[7]; v[3] = m[8]; }
  if (m[9] > bd) { v[0] = m[3]; v[1] = m[6]; v[2] = m[8]; v[3] = m[9]; }
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const double w0 = t[0] * v[0] + t[1] * v[1] + t[2] * v[2] + t[3] * v[3];
    const double w1 = t[1] * v[0] + t[4] * v[1] + t[5] * v[2] + t[6] * v[3];
    const double w2 = t[2] * v[0] + t[5] * v[1] + t[7] * v[2] + t[8] * v[3];
    const double w3 = t[3] * v[0] + t[6] * v[1] + t[8] * v[2] + t[9] * v[3];
    const double n = 1.0 / sqrt((w0 * w0 + w1 * w1) + (w2 * w2 + w3 * w3));
    v[0] = w0 * n; v[1] = w1 * n; v[2] = w2 * n; v[3] = w3 * n;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) out[k] = v[k];
}

}  // namespace spef
