// Pose covariance of the soft-classification decode on gfx950 (spef_decode_cov; the NumPy twin and the specification
// is spef_amd/spe/decode_cov.py).
//
//   decode_cov_kernel  per row: the 6 x 6 measurement covariance the pose tracker takes (theta first, then t; theta a
//                      left perturbation in the camera frame, R = exp([theta]x) R^, the convention of k_track.hip and
//                      k_refine.hip) from the PDFs the decode averaged, about the pose it decoded them to:
//                        theta block = sum_i p_i theta_i theta_i^T / sum_i p_i + floor, theta_i = Log(q_i (x) conj(q^))
//                        t block     = sum_i p_i (g_i - t^)(g_i - t^)^T / sum_i p_i + floor   (the centred form)
//                      and, when asked for, inv(a) of the Markley matrix a = sum_i p_i q_i q_i^T: the second value of
//                      OrientationSoftClassification.decode (classification_utils.py:142), "the uncertainty in the maximum
//                      likelihood sense", which the decode kernels drop.
// One 256-thread workgroup per (row, head): blockIdx.y = 0 the orientation head (rows 0..2 of cov, ori_hinv and the
// status word), 1 the position head (rows 3..5). The bins are read in a strided loop (any table size), every
// accumulator is fp64 and the workgroup's partials are reduced in the fixed order of decode_ori_kernel -- LDS, then each
// 16-lane row sums one accumulator by DPP -- so a row's result does not depend on the batch it is in. The status word
// is written by the orientation workgroup alone (no atomics): it sums the position PDF's mass as well, in the order the
// position workgroup does, and so evaluates the same predicate for bit 4. One lane does the tail: the 4 x 4 Cholesky
// inverse, the floors, the float32 casts.
#include <math.h>

#include "spef_common.hpp"
#include "spef_kernels.hpp"
#include "spef_pose_math.hpp"
#include "spef_reduce.hpp"

namespace spef {

enum : int { CS_ORI = 1, CS_HINV = 2, CS_POS = 4 };

constexpr int COV_NACC = 18;   // orientation workgroup: 6 theta theta^T + 10 a + sum p + the position PDF's sum p
constexpr int COV_NPOS = 7;    // position workgroup: 6 (g - t^)(g - t^)^T + sum p

__device__ __forceinline__ bool cov_finite(double x) { return fabs(x) < INFINITY; }
__device__ __forceinline__ bool cov_mass_ok(double sp) { return sp > 0.0 && sp < INFINITY; }

// (the workgroup's fixed-order sum of the accumulators, cov_reduce: spef_reduce.hpp)

// inv(a) of the symmetric 4 x 4 a (packed upper triangle t: 0:00 1:01 2:02 3:03 4:11 5:12 6:13 7:22 8:23 9:33) through
// its Cholesky factor a = L L^T, inv = L^-T L^-1. -> false when a is not positive definite to fp64: a pivot that is not
// finite, or not above 2^-48 of its diagonal entry (the rounding of the sums that made it; 0 for an exact 0).
__device__ bool sym4_inverse(const double t[10], double inv[4][4]) {
  const double a[4][4] = {{t[0], t[1], t[2], t[3]}, {t[1], t[4], t[5], t[6]}, {t[2], t[5], t[7], t[8]},
                          {t[3], t[6], t[8], t[9]}};
  double L[4][4] = {}, id[4];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double d = a[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    const bool good = d > 0x1p-48 * a[j][j] && d < INFINITY;
    ok = ok && good;
    d = good ? d : 1.0;
    L[j][j] = sqrt(d);
    id[j] = 1.0 / L[j][j];
#pragma unroll
    for (int i = j + 1; i < 4; ++i) {
      double v = a[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
      L[i][j] = v * id[j];
    }
  }
  // M = L^-1 (lower), column by column
  double M[4][4] = {};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    M[c][c] = id[c];
#pragma unroll
    for (int i = c + 1; i < 4; ++i) {
      double v = 0.0;
#pragma unroll
      for (int k = c; k < i; ++k) v -= L[i][k] * M[k][c];
      M[i][c] = v * id[i];
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = i; j < 4; ++j) {
      double v = 0.0;
#pragma unroll
      for (int k = j; k < 4; ++k) v += M[k][i] * M[k][j];
      inv[i][j] = inv[j][i] = v;
    }
  return ok;
}

__global__ __launch_bounds__(256) void decode_cov_kernel(int ori_cls, int pos_cls, const float* __restrict__ ori_pdf,
                                                         int n_ori, const double* __restrict__ qb,
                                                         const float* __restrict__ pos_pdf, int n_pos,
                                                         const double* __restrict__ grid, const float* __restrict__ quat,
                                                         const float* __restrict__ pos, CovParams prm,
                                                         float* __restrict__ cov, float* __restrict__ hinv,
                                                         int* __restrict__ cov_status) {
  __shared__ double shd[COV_NACC][256];
  __shared__ double shp[COV_NACC];
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  float* out = cov + 36 * b;

  // the position PDF's partial sums of sum p (both workgroups: the same loop, the same reduction, the same value)
  double t[3] = {0.0, 0.0, 0.0};
  bool t_ok = true;
  double psp = 0.0;
  const float* pp = pos_cls ? pos_pdf + b * (size_t)n_pos : nullptr;
  if (pos_cls) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      t[k] = (double)pos[3 * b + k];
      t_ok = t_ok && cov_finite(t[k]);
    }
  }

  if (blockIdx.y == 1) {   // ------------------------------------------------------------------ position head
    float* o = out + 18;
    if (!pos_cls) {   // regression: no PDF, the caller's fixed variance
      if (tid < 18) o[tid] = (tid == 3 || tid == 10 || tid == 17) ? (float)prm.fixed_var[1] : 0.0f;
      return;
    }
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n_pos; i += 256) {
      const double p = (double)pp[i];
      const double ex = grid[3 * i] - t[0], ey = grid[3 * i + 1] - t[1], ez = grid[3 * i + 2] - t[2];
      psp += p;
      acc[0] += (ex * ex) * p; acc[1] += (ex * ey) * p; acc[2] += (ex * ez) * p;
      acc[3] += (ey * ey) * p; acc[4] += (ey * ez) * p; acc[5] += (ez * ez) * p;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) shd[k][tid] = acc[k];
    shd[6][tid] = psp;
    __syncthreads();
    cov_reduce(shd, shp, COV_NPOS);
    if (tid != 0) return;
    const double sp = shp[6];
    const bool ok = t_ok && cov_mass_ok(sp);
    const double r = 1.0 / sp, fl = prm.floor_var[1];
    const float xx = ok ? (float)(shp[0] * r + fl) : NAN, xy = ok ? (float)(shp[1] * r) : NAN;
    const float xz = ok ? (float)(shp[2] * r) : NAN, yy = ok ? (float)(shp[3] * r + fl) : NAN;
    const float yz = ok ? (float)(shp[4] * r) : NAN, zz = ok ? (float)(shp[5] * r + fl) : NAN;
    o[0] = 0.f; o[1] = 0.f; o[2] = 0.f; o[3] = xx; o[4] = xy; o[5] = xz;
    o[6] = 0.f; o[7] = 0.f; o[8] = 0.f; o[9] = xy; o[10] = yy; o[11] = yz;
    o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = xz; o[16] = yz; o[17] = zz;
    return;
  }

  // ---------------------------------------------------------------------------------------------- orientation head
  if (pos_cls)
    for (int i = tid; i < n_pos; i += 256) psp += (double)pp[i];
  double acc[17];
#pragma unroll
  for (int k = 0; k < 17; ++k) acc[k] = 0.0;
  bool q_ok = true;
  if (ori_cls) {
    double qh[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) qh[k] = (double)quat[4 * b + k];
    const double qn2 = (qh[0] * qh[0] + qh[1] * qh[1]) + (qh[2] * qh[2] + qh[3] * qh[3]);
    q_ok = qn2 > 0.0 && qn2 < INFINITY;   // a NaN or an infinity in q^ makes qn2 NaN or infinite
    const double qs = rsq_nr(q_ok ? qn2 : 1.0);
#pragma unroll
    for (int k = 0; k < 4; ++k) qh[k] *= qs;
    const float* x = ori_pdf + b * (size_t)n_ori;
    for (int i = tid; i < n_ori; i += 256) {
      const double p = (double)x[i];
      const double4 q = *reinterpret_cast<const double4*>(qb + 4 * (size_t)i);
      // d = q_i (x) conj(q^) on the hemisphere d0 >= 0; theta_i = Log(d) = f d_xyz (spe.track.qlog)
      double d0 = q.x * qh[0] + q.y * qh[1] + q.z * qh[2] + q.w * qh[3];
      double d1 = -q.x * qh[1] + q.y * qh[0] - q.z * qh[3] + q.w * qh[2];
      double d2 = -q.x * qh[2] + q.y * qh[3] + q.z * qh[0] - q.w * qh[1];
      double d3 = -q.x * qh[3] - q.y * qh[2] + q.z * qh[1] + q.w * qh[0];
      if (d0 < 0.0) { d0 = -d0; d1 = -d1; d2 = -d2; d3 = -d3; }
      const double n2 = d1 * d1 + d2 * d2 + d3 * d3;
      const double n = dsqrt(n2);
      const double f = n < 1e-8 ? 2.0 / d0 * (1.0 - n2 / (3.0 * d0 * d0)) : 2.0 * atan2(n, d0) * rcp_nr(n);
      const double w = (f * f) * p;
      acc[0] += (d1 * d1) * w; acc[1] += (d1 * d2) * w; acc[2] += (d1 * d3) * w;
      acc[3] += (d2 * d2) * w; acc[4] += (d2 * d3) * w; acc[5] += (d3 * d3) * w;
      acc[6] += (q.x * q.x) * p; acc[7] += (q.x * q.y) * p; acc[8] += (q.x * q.z) * p; acc[9] += (q.x * q.w) * p;
      acc[10] += (q.y * q.y) * p; acc[11] += (q.y * q.z) * p; acc[12] += (q.y * q.w) * p;
      acc[13] += (q.z * q.z) * p; acc[14] += (q.z * q.w) * p; acc[15] += (q.w * q.w) * p;
      acc[16] += p;
    }
  }
#pragma unroll
  for (int k = 0; k < 17; ++k) shd[k][tid] = acc[k];
  shd[17][tid] = psp;
  __syncthreads();
  cov_reduce(shd, shp, COV_NACC);
  if (tid != 0) return;
  int st = 0;
  if (pos_cls && !(t_ok && cov_mass_ok(shp[17]))) st |= CS_POS;
  if (!ori_cls) {   // regression: no PDF, the caller's fixed variance
    const float fv = (float)prm.fixed_var[0];
#pragma unroll
    for (int k = 0; k < 18; ++k) out[k] = (k == 0 || k == 7 || k == 14) ? fv : 0.0f;
    cov_status[b] = st;
    return;
  }
  const double sp = shp[16];
  const bool ok = q_ok && cov_mass_ok(sp);
  if (!ok) st |= CS_ORI;
  const double r = 1.0 / sp, fl = prm.floor_var[0];
  const float xx = ok ? (float)(shp[0] * r + fl) : NAN, xy = ok ? (float)(shp[1] * r) : NAN;
  const float xz = ok ? (float)(shp[2] * r) : NAN, yy = ok ? (float)(shp[3] * r + fl) : NAN;
  const float yz = ok ? (float)(shp[4] * r) : NAN, zz = ok ? (float)(shp[5] * r + fl) : NAN;
  out[0] = xx; out[1] = xy; out[2] = xz; out[3] = 0.f; out[4] = 0.f; out[5] = 0.f;
  out[6] = xy; out[7] = yy; out[8] = yz; out[9] = 0.f; out[10] = 0.f; out[11] = 0.f;
  out[12] = xz; out[13] = yz; out[14] = zz; out[15] = 0.f; out[16] = 0.f; out[17] = 0.f;
  double inv[4][4];
  const bool pd = sym4_inverse(&shp[6], inv);
  if (!pd) st |= CS_HINV;
  if (hinv) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) hinv[16 * b + 4 * i + j] = pd ? (float)inv[i][j] : NAN;
  }
  cov_status[b] = st;
}

hipError_t launch_decode_cov(int ori_cls, int pos_cls, const float* ori_pdf, int n_ori, const double* q_bins,
                             const float* pos_pdf, int n_pos, const double* grid, const float* quat, const float* pos,
                             int B, const CovParams& prm, float* cov, float* ori_hinv, int* cov_status, hipStream_t s) {
  if (B < 1) return hipErrorInvalidValue;
  decode_cov_kernel<<<dim3((unsigned)B, 2), 256, 0, s>>>(ori_cls, pos_cls, ori_pdf, n_ori, q_bins, pos_pdf, n_pos, grid,
                                                         quat, pos, prm, cov, ori_hinv, cov_status);
  return hipGetLastError();
}

}  // namespace spef
