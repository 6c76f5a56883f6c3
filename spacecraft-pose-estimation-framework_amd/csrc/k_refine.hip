// Robust Levenberg-Marquardt pose refinement behind the batched EPnP (k_epnp.hip): minimises the reprojection error of
// the n <= 16 keypoints over the pose itself, with an optional Huber loss and per-point confidences, and returns the
// pose covariance of the same normal matrix. The algorithm and its constants are those of the NumPy twin
// (spef_amd/spe/refine.py: refine_pose_host); EPnP, OpenCV's and the reference's last step, has no such stage.
//
// One problem per wave, 16 lanes of it: lane i < n owns point i -- its 3-D point, undistorted pixel, confidence, and per
// evaluation its residual, IRLS weight and 2 x 6 Jacobian rows, all in registers. The 21 + 6 + 2 sums of an evaluation
// (upper triangle of J^T W J, J^T W r, cost, squared residuals) are reduced over the 16-lane DPP row in a fixed order
// (quad swaps, half-row mirror, row mirror: every lane ends with the same bits), so the 6 x 6 Cholesky solve, the
// exponential map and the accept / damping logic run uniformly on every lane: no LDS, no barrier. A problem is a
// serial chain of trials, so latency per problem is what matters, as in EPnP (a B = 64 batch is 64 concurrent waves).
#include <math.h>

#include "spef_common.hpp"
#include "spef_kernels.hpp"
#include "spef_pose_math.hpp"
#include "spef_reduce.hpp"

namespace spef {

#define REFINE_NSUM 29   // 0..20 upper triangle of A row by row, 21..26 g, 27 cost, 28 sum of squared residuals

__device__ __forceinline__ double row_sum16_d(double v) {   // sum over the 16-lane row, identical in every lane
  v = dpp_add_d<0xB1>(v);    // quad_perm [1,0,3,2]
  v = dpp_add_d<0x4E>(v);    // quad_perm [2,3,0,1]
  v = dpp_add_d<0x141>(v);   // row_half_mirror
  return dpp_add_d<0x140>(v);   // row_mirror
}

// Residuals, weights and the normal equations at (R, t); returns true when a point is not in front of the camera.
// Left perturbation R <- exp([w]x) R, t <- t + dt: d(Xc) = -[R X]x w + dt.
__device__ __forceinline__ bool refine_eval(const double (&R)[3][3], const double (&t)[3], bool pt,
                                            const double (&X)[3], double uo, double vo, double conf, double fu,
                                            double fv, double uc, double vc, double huber,
                                            double (&S)[REFINE_NSUM]) {
  double s[REFINE_NSUM];
#pragma unroll
  for (int k = 0; k < REFINE_NSUM; ++k) s[k] = 0.0;
  bool behind = false;
  if (pt) {
    const double px = R[0][0] * X[0] + R[0][1] * X[1] + R[0][2] * X[2];
    const double py = R[1][0] * X[0] + R[1][1] * X[1] + R[1][2] * X[2];
    const double pz = R[2][0] * X[0] + R[2][1] * X[1] + R[2][2] * X[2];
    const double z = pz + t[2];
    behind = !(z > 0.0);
    const double iz = rcp_nr(z);
    const double x = (px + t[0]) * iz, y = (py + t[1]) * iz;
    const double ru = fu * x + uc - uo, rv = fv * y + vc - vo;
    const double e2 = ru * ru + rv * rv;
    double w = conf, rho = conf * e2;
    if (huber > 0.0) {
      const double e = dsqrt(e2);
      if (e > huber) {
        w = conf * (huber * rcp_nr(e));
        rho = conf * (2.0 * huber * e - huber * huber);
      }
    }
    const double a = fu * iz, c = fv * iz;
    const double bx = a * x, by = c * y;
    const double Ju[6] = {-bx * py, a * pz + bx * px, -a * py, a, 0.0, -bx};
    const double Jv[6] = {-c * pz - by * py, by * px, c * px, 0.0, c, -by};
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) s[k++] = w * (Ju[i] * Ju[j] + Jv[i] * Jv[j]);
#pragma unroll
    for (int i = 0; i < 6; ++i) s[21 + i] = w * (Ju[i] * ru + Jv[i] * rv);
    s[27] = rho;
    s[28] = e2;
  }
#pragma unroll
  for (int k = 0; k < REFINE_NSUM; ++k) S[k] = row_sum16_d(s[k]);
  return __ballot(behind) != 0;
}

// Cholesky of A + lam diag(A) (A = the upper triangle in S): L lower, inv[j] = 1 / L[j][j]; false on a pivot that is
// not positive (or not finite).
__device__ __forceinline__ bool refine_chol(const double (&S)[REFINE_NSUM], double lam, double (&L)[6][6],
                                            double (&inv)[6]) {
  double M[6][6];
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) {
      M[j][i] = S[k++];
      if (i == j) M[i][i] += lam * M[i][i];
    }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = M[j][j];
#pragma unroll
    for (int q = 0; q < j; ++q) d -= L[j][q] * L[j][q];
    const bool good = d > 0.0 && d < INFINITY;
    ok = ok && good;
    d = good ? d : 1.0;
    inv[j] = rsq_nr(d);
    L[j][j] = d * inv[j];
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = M[i][j];
#pragma unroll
      for (int q = 0; q < j; ++q) v -= L[i][q] * L[j][q];
      L[i][j] = v * inv[j];
    }
  }
  return ok;
}

// x = (L L^T)^-1 b
__device__ __forceinline__ void refine_solve(const double (&L)[6][6], const double (&inv)[6], const double (&b)[6],
                                             double (&x)[6]) {
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double v = b[i];
#pragma unroll
    for (int q = 0; q < i; ++q) v -= L[i][q] * y[q];
    y[i] = v * inv[i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double v = y[i];
#pragma unroll
    for (int q = i + 1; q < 6; ++q) v -= L[q][i] * x[q];
    x[i] = v * inv[i];
  }
}

// R2 = exp([w]x) R: I + a [w]x + b [w]x^2 with a = sin(th) / th = 2 sin(th / 2) cos(th / 2) / th and b = (1 - cos(th))
// / th^2 = 2 sin^2(th / 2) / th^2 (no cancellation; one sincos of the half angle)
__device__ __forceinline__ void refine_rotate(const double (&w)[3], const double (&R)[3][3], double (&R2)[3][3]) {
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double a = 1.0, b = 0.5;
  if (!(th2 < 1e-300)) {
    const double th = dsqrt(th2);
    double sh, ch;
    sincos(0.5 * th, &sh, &ch);
    a = 2.0 * sh * ch * rcp_nr(th);
    b = 2.0 * sh * sh * rcp_nr(th2);
  }
  const double Kx[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
  double E[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double k2 = Kx[i][0] * Kx[0][j] + Kx[i][1] * Kx[1][j] + Kx[i][2] * Kx[2][j];
      E[i][j] = (i == j ? 1.0 : 0.0) + a * Kx[i][j] + b * k2;
    }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R2[i][j] = E[i][0] * R[0][j] + E[i][1] * R[1][j] + E[i][2] * R[2][j];
}

__global__ __launch_bounds__(64) void refine_kernel(const float* __restrict__ kp, const float* __restrict__ weights,
                                                    int B, int n, const float* __restrict__ kp3d, double fu, double fv,
                                                    double uc, double vc, float nu, float nv, EpnpDist dist,
                                                    int max_iters, float huber_px, float* __restrict__ quat,
                                                    float* __restrict__ pos, float* __restrict__ fit,
                                                    float* __restrict__ cov, int* __restrict__ iters,
                                                    int* __restrict__ status) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;   // uniform per wave
  const int nk = 2 * (n + 1);
  const bool pt = lane < n;
  const double huber = (double)huber_px;

  // ---- observations: what epnp_kernel solves on (float32 pixels, origin dropped, undistortPoints)
  double X[3] = {0, 0, 0}, uo = 0.0, vo = 0.0, conf = 0.0;
  if (pt) {
    const float x = kp[(size_t)b * nk + 2 * (lane + 1)], y = kp[(size_t)b * nk + 2 * (lane + 1) + 1];
    undistort_point(dist, fu, fv, uc, vc, x * nu, y * nv, uo, vo);
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = (double)kp3d[3 * lane + k];
    conf = weights ? (double)weights[(size_t)b * n + lane] : 1.0;
  }
  double q[4], t[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = (double)quat[4 * b + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = (double)pos[3 * b + k];
  const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const bool pose_ok = qn > 0.0 && qn < INFINITY && fabs(t[0]) < INFINITY && fabs(t[1]) < INFINITY && fabs(t[2]) < INFINITY;
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = q[k] / qn;
  double R[3][3] = {   // quat2dcm (spe/utils.py:10-53)
      {2 * q[0] * q[0] - 1 + 2 * q[1] * q[1], 2 * q[1] * q[2] - 2 * q[0] * q[3], 2 * q[1] * q[3] + 2 * q[0] * q[2]},
      {2 * q[1] * q[2] + 2 * q[0] * q[3], 2 * q[0] * q[0] - 1 + 2 * q[2] * q[2], 2 * q[2] * q[3] - 2 * q[0] * q[1]},
      {2 * q[1] * q[3] - 2 * q[0] * q[2], 2 * q[2] * q[3] + 2 * q[0] * q[1], 2 * q[0] * q[0] - 1 + 2 * q[3] * q[3]}};

  const bool lane_bad = pt && !(fabs(uo) < INFINITY && fabs(vo) < INFINITY && conf >= 0.0 && conf < INFINITY);
  const int m = __popcll(__ballot(pt && conf > 0.0));
  double S[REFINE_NSUM];
  const bool behind0 = refine_eval(R, t, pt, X, uo, vo, conf, fu, fv, uc, vc, huber, S);
  const bool refuse = (status[b] & 8) != 0 || __ballot(lane_bad) != 0 || !pose_ok || behind0 || m < 3 ||
                      !(fabs(S[27]) < INFINITY);
  if (refuse) {   // uniform: the pose stays as it came
    if (lane == 0) {
      status[b] |= 16;
      if (iters) iters[b] = 0;
    }
    if (fit && lane < 4) fit[4 * b + lane] = NAN;
    if (cov)
      for (int k = lane; k < 36; k += 16) cov[36 * (size_t)b + k] = NAN;
    return;
  }

  const double cost0 = S[27], ss0 = S[28];
  double lam = 1e-3;
  int it = 0;
  bool accepted = false, stopped = false;
  while (it < max_iters) {
    ++it;
    double L[6][6], inv[6], g[6], d[6];
    const bool ok = refine_chol(S, lam, L, inv);
    bool small = false, take = false;
    if (ok) {
#pragma unroll
      for (int k = 0; k < 6; ++k) g[k] = -S[21 + k];
      refine_solve(L, inv, g, d);
      bool fin = true;
#pragma unroll
      for (int k = 0; k < 6; ++k) fin = fin && fabs(d[k]) < INFINITY;
      if (fin) {
        const double w[3] = {d[0], d[1], d[2]};
        double R2[3][3], S2[REFINE_NSUM];
        refine_rotate(w, R, R2);
        const double t2[3] = {t[0] + d[3], t[1] + d[4], t[2] + d[5]};
        const bool behind = refine_eval(R2, t2, pt, X, uo, vo, conf, fu, fv, uc, vc, huber, S2);
        // |dw| < 1e-10 and |dt| < 1e-10 |t|, as squares
        small = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] < 1e-20 &&
                d[3] * d[3] + d[4] * d[4] + d[5] * d[5] < 1e-20 * (t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
        take = !behind && S2[27] < S[27];
        if (take) {
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            t[i] = t2[i];
#pragma unroll
            for (int j = 0; j < 3; ++j) R[i][j] = R2[i][j];
          }
#pragma unroll
          for (int k = 0; k < REFINE_NSUM; ++k) S[k] = S2[k];
          accepted = true;
        }
      }
    }
    lam = take ? fmax(lam / 10, 1e-9) : lam * 10;
    if (small || lam > 1e12) {
      stopped = true;
      break;
    }
  }

  // ---- covariance s^2 A^-1 at the final pose: A^-1 = L^-T L^-1
  if (cov) {
    double L[6][6], inv[6], Li[6][6];
    const bool ok = refine_chol(S, 0.0, L, inv);
#pragma unroll
    for (int c = 0; c < 6; ++c)        // column c of L^-1 (rows c..5)
#pragma unroll
      for (int i = c; i < 6; ++i) {
        double v = i == c ? 1.0 : 0.0;
#pragma unroll
        for (int k = c; k < i; ++k) v -= L[i][k] * Li[k][c];
        Li[i][c] = v * inv[i];
      }
    const int dof = 2 * m - 6 > 1 ? 2 * m - 6 : 1;
    const double s2 = S[27] / (double)dof;
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) {
          double v = 0.0;
#pragma unroll
          for (int k = j; k < 6; ++k) v += Li[k][i] * Li[k][j];
          const float c = ok ? (float)(s2 * v) : NAN;
          cov[36 * (size_t)b + 6 * i + j] = c;
          cov[36 * (size_t)b + 6 * j + i] = c;
        }
    }
  }
  if (lane != 0) return;
  if (accepted) {
    double qo[4];
    dcm2quat(R, qo);
    const double no = sqrt(qo[0] * qo[0] + qo[1] * qo[1] + qo[2] * qo[2] + qo[3] * qo[3]);
    const double sg = qo[0] * q[0] + qo[1] * q[1] + qo[2] * q[2] + qo[3] * q[3] < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) quat[4 * b + k] = (float)(sg * (qo[k] / no));
#pragma unroll
    for (int k = 0; k < 3; ++k) pos[3 * b + k] = (float)t[k];
  }
  if (fit) {
    fit[4 * b + 0] = (float)sqrt(ss0 / (double)n);
    fit[4 * b + 1] = (float)sqrt(S[28] / (double)n);
    fit[4 * b + 2] = (float)cost0;
    fit[4 * b + 3] = (float)S[27];
  }
  if (iters) iters[b] = it;
  if (!stopped) status[b] |= 32;
}

hipError_t launch_refine(const float* kp, const float* weights, int B, int n, const float* kp3d, const double* K,
                         float nu, float nv, const EpnpDist& dist, int max_iters, float huber_px, float* quat,
                         float* pos, float* fit, float* cov, int* iters, int* status, hipStream_t s) {
  if (n < 4 || n > EPNP_MAXN) return hipErrorInvalidValue;
  refine_kernel<<<B, 16, 0, s>>>(kp, weights, B, n, kp3d, K[0], K[4], K[2], K[5], nu, nv, dist, max_iters, huber_px,
                                 quat, pos, fit, cov, iters, status);
  return hipGetLastError();
}

}  // namespace spef
