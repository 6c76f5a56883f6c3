// Exhaustive 3-point consensus between the batched EPnP (k_epnp.hip) and the pose refinement (k_refine.hip): an inlier
// selection for keypoint heads that regress occluded or out-of-frame points without a confidence. A model has n <= 16
// points, so all C(n, 3) <= 560 minimal samples are solved (P3P: Grunert's quartic in the form of Haralick et al. 1994)
// and every hypothesis is scored on all candidate points with the truncated squared reprojection error -- no sampling,
// no seed, nothing that depends on the batch. The algorithm and its constants are those of the NumPy twin
// (spef_amd/spe/consensus.py: consensus_host), which is the specification.
//
// One workgroup per problem, one triple per thread: 192 threads take the 165 triples of the 11-point Tango model in
// one pass (256 threads stride over the 560 triples of a 16-point model in three). A hypothesis is a serial chain (quartic
// -> distances, polished by two Newton steps on the law of cosines -> pose -> n reprojections), so the latency of a problem is that chain once, not C(n, 3) / 64 times as with one wave
// per problem; a B = 64 batch is 192 waves on 256 CUs either way. The n observations, bearings, model points and
// confidences sit in LDS (written once by the first n threads; the scoring loop reads one address per step, a
// broadcast). The arg-min over (cost, triple, root) is a total order, reduced in a fixed pattern: the 16-lane rows by
// DPP, the 4 rows by readlane, the waves through LDS. The winner's thread publishes its pose through LDS and the first
// n threads classify the points. No atomics, no allocation, fp64 throughout.
#include <limits.h>
#include <math.h>

#include "spef_common.hpp"
#include "spef_kernels.hpp"
#include "spef_pose_math.hpp"
#include "spef_reduce.hpp"

namespace spef {

#define CONS_DEGENERATE 1e-6   // model triangle: |cross| <= CONS_DEGENERATE (longest edge)^2 is skipped
#define CONS_A4_MIN 1e-12      // quartic: |A4| <= CONS_A4_MIN max |A_k| is skipped
#define CONS_POLISH_STEPS 2    // Newton steps on the three distances after the quartic

template <int CTRL>
__device__ __forceinline__ double dpp_get_d(double v) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)u, CTRL, 0xf, 0xf, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)(u >> 32), CTRL, 0xf, 0xf, false);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
// (cost, key) <- the smaller of itself and (oc, ok): cost first, then key. Costs are never NaN (none = +inf, INT_MAX).
__device__ __forceinline__ void argmin_take(double& c, int& k, double oc, int ok) {
  const bool take = oc < c || (oc == c && ok < k);
  c = take ? oc : c;
  k = take ? ok : k;
}
template <int CTRL>
__device__ __forceinline__ void argmin_dpp(double& c, int& k, int& cnt) {
  const double oc = dpp_get_d<CTRL>(c);
  const int ok = __builtin_amdgcn_mov_dpp(k, CTRL, 0xf, 0xf, false);
  cnt += __builtin_amdgcn_mov_dpp(cnt, CTRL, 0xf, 0xf, false);
  argmin_take(c, k, oc, ok);
}
// the wave's arg-min and the sum of cnt, identical in every lane
__device__ __forceinline__ void argmin_wave(double& c, int& k, int& cnt) {
  argmin_dpp<0xB1>(c, k, cnt);    // quad_perm [1,0,3,2]
  argmin_dpp<0x4E>(c, k, cnt);    // quad_perm [2,3,0,1]
  argmin_dpp<0x141>(c, k, cnt);   // row_half_mirror
  argmin_dpp<0x140>(c, k, cnt);   // row_mirror
  double bc = readlane_d(c, 0);
  int bk = __builtin_amdgcn_readlane(k, 0), bn = __builtin_amdgcn_readlane(cnt, 0);
#pragma unroll
  for (int r = 16; r < 64; r += 16) {
    argmin_take(bc, bk, readlane_d(c, r), __builtin_amdgcn_readlane(k, r));
    bn += __builtin_amdgcn_readlane(cnt, r);
  }
  c = bc;
  k = bk;
  cnt = bn;
}

// One Newton step on a4 x^4 + ... + a0; not taken when the derivative is zero or the result is not finite.
__device__ __forceinline__ double newton4(double a4, double a3, double a2, double a1, double a0, double x) {
  const double f = (((a4 * x + a3) * x + a2) * x + a1) * x + a0;
  const double df = ((4.0 * a4 * x + 3.0 * a3) * x + 2.0 * a2) * x + a1;
  const double x2 = x - ddiv(f, df);
  return (df != 0.0 && fabs(x2) < INFINITY) ? x2 : x;
}
__device__ __forceinline__ double newton3(double c2, double c1, double c0, double x) {
  const double f = ((x + c2) * x + c1) * x + c0;
  const double df = (3.0 * x + 2.0 * c2) * x + c1;
  const double x2 = x - ddiv(f, df);
  return (df != 0.0 && fabs(x2) < INFINITY) ? x2 : x;
}

// Real roots of the quartic, ascending, +inf where there is none. Ferrari: depressed quartic y^4 + p y^2 + q y + r,
// the largest real root m of the resolvent cubic m^3 + p m^2 + (p^2 / 4 - r) m - q^2 / 8 (Cardano when it has one real
// root, the trigonometric form when it has three; two Newton steps), then y^2 -+ w y + (p / 2 + m +- q / (2 w)),
// w = sqrt(2 m); two Newton steps on the original quartic.
__device__ __forceinline__ void quartic_roots(double A4, double A3, double A2, double A1, double A0, double& r0,
                                              double& r1, double& r2, double& r3) {
  const double big = fmax(fmax(fabs(A3), fabs(A2)), fmax(fabs(A1), fabs(A0)));
  bool ok = fabs(A4) > CONS_A4_MIN * fmax(fabs(A4), big);
  const double i4 = rcp_nr(ok ? A4 : 1.0);
  const double b = A3 * i4, c = A2 * i4, d = A1 * i4, e = A0 * i4;
  const double b2 = b * b;
  const double p = c - 0.375 * b2;
  const double q = d - 0.5 * b * c + 0.125 * b2 * b;
  const double r = e - 0.25 * b * d + 0.0625 * b2 * c - (3.0 / 256.0) * b2 * b2;
  const double c2 = p, c1 = 0.25 * p * p - r, c0 = -0.125 * q * q;
  const double P = c1 - c2 * c2 * (1.0 / 3.0);
  const double Q = 2.0 * c2 * c2 * c2 * (1.0 / 27.0) - c2 * c1 * (1.0 / 3.0) + c0;
  const double D = 0.25 * Q * Q + P * P * P * (1.0 / 27.0);
  double t;
  if (D > 0.0) {
    double A = cbrt(0.5 * fabs(Q) + dsqrt(D));
    A = Q > 0.0 ? -A : A;
    t = A - ddiv(P, 3.0 * A);
  } else {
    const double k = dsqrt(fmax(-P * (1.0 / 3.0), 0.0));
    const double k3 = k * k * k;
    t = 0.0;
    if (k3 > 0.0) {
      const double cs = fmin(fmax(ddiv(-Q, 2.0 * k3), -1.0), 1.0);
      t = 2.0 * k * cos(acos(cs) * (1.0 / 3.0));
    }
  }
  double m = t - c2 * (1.0 / 3.0);
  m = newton3(c2, c1, c0, m);
  m = newton3(c2, c1, c0, m);
  ok = ok && m > 0.0 && m < INFINITY;
  const double w = dsqrt(ok ? 2.0 * m : 1.0);
  const double qw = ddiv(2.0 * q, w);
  const double base = -2.0 * p - 2.0 * m;
  const double d1 = base - qw, d2 = base + qw;
  const double s1 = dsqrt(fmax(d1, 0.0)), s2 = dsqrt(fmax(d2, 0.0));
  const double sh = 0.25 * b;
  const bool h1 = ok && d1 >= 0.0, h2 = ok && d2 >= 0.0;
  double y[4] = {0.5 * (w - s1) - sh, 0.5 * (w + s1) - sh, 0.5 * (-w - s2) - sh, 0.5 * (-w + s2) - sh};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool have = k < 2 ? h1 : h2;
    double x = have ? y[k] : 0.0;
    x = newton4(A4, A3, A2, A1, A0, x);
    x = newton4(A4, A3, A2, A1, A0, x);
    y[k] = (have && fabs(x) < INFINITY) ? x : INFINITY;
  }
  double a0 = fmin(y[0], y[1]), a1 = fmax(y[0], y[1]), a2 = fmin(y[2], y[3]), a3 = fmax(y[2], y[3]);   // sorting network
  r0 = fmin(a0, a2);
  const double m02 = fmax(a0, a2), m13 = fmin(a1, a3);
  r3 = fmax(a1, a3);
  r1 = fmin(m13, m02);
  r2 = fmax(m13, m02);
}

// One Newton step on the three law-of-cosines equations the distances solve (3 x 3, Cramer's rule; the Jacobian's
// diagonal is zero): u comes from v through a quotient that can be small, and two of these bring the camera triangle
// back to the model's to rounding. Not taken when the Jacobian is singular or the result is not finite.
__device__ __forceinline__ void polish_step(double& s1, double& s2, double& s3, double ca, double cb, double cg,
                                            double a2, double b2, double c2) {
  const double f1 = s2 * s2 + s3 * s3 - 2.0 * s2 * s3 * ca - a2;
  const double f2 = s1 * s1 + s3 * s3 - 2.0 * s1 * s3 * cb - b2;
  const double f3 = s1 * s1 + s2 * s2 - 2.0 * s1 * s2 * cg - c2;
  const double j12 = 2.0 * (s2 - s3 * ca), j13 = 2.0 * (s3 - s2 * ca);
  const double j21 = 2.0 * (s1 - s3 * cb), j23 = 2.0 * (s3 - s1 * cb);
  const double j31 = 2.0 * (s1 - s2 * cg), j32 = 2.0 * (s2 - s1 * cg);
  const double det = j12 * j23 * j31 + j13 * j21 * j32;
  const double idet = rcp_nr(det);
  const double d1 = (-f1 * j23 * j32 + j12 * j23 * f3 + j13 * f2 * j32) * idet;
  const double d2 = (j13 * j21 * f3 + f1 * j23 * j31 - j13 * f2 * j31) * idet;
  const double d3 = (j12 * f2 * j31 + f1 * j21 * j32 - j12 * j21 * f3) * idet;
  const bool good = det != 0.0 && fabs(d1) < INFINITY && fabs(d2) < INFINITY && fabs(d3) < INFINITY;
  s1 = good ? s1 - d1 : s1;
  s2 = good ? s2 - d2 : s2;
  s3 = good ? s3 - d3 : s3;
}

__global__ __launch_bounds__(256) void consensus_kernel(const float* __restrict__ kp, const float* __restrict__ weights,
                                                        int B, int n, const float* __restrict__ kp3d, double fu,
                                                        double fv, double uc, double vc, float nu, float nv,
                                                        EpnpDist dist, float inlier_px, int min_inliers,
                                                        float* __restrict__ quat, float* __restrict__ pos,
                                                        float* __restrict__ weights_out, int* __restrict__ info,
                                                        float* __restrict__ cost_out, double* __restrict__ pose64,
                                                        int* __restrict__ status) {
  __shared__ double sX[EPNP_MAXN][3], sF[EPNP_MAXN][3], sUV[EPNP_MAXN][2], sCost[4], sPose[12];
  __shared__ float sC[EPNP_MAXN];
  __shared__ int sKey[4], sCnt[4], sRow[2];
  const int b = blockIdx.x, tid = threadIdx.x, nthreads = blockDim.x;
  if (b >= B) return;   // uniform per workgroup
  const int nk = 2 * (n + 1);
  const bool pt = tid < n;   // n <= 16: all in wave 0
  const double tau2 = (double)inlier_px * (double)inlier_px;

  // ---- observations: what epnp_kernel and refine_kernel solve on; bearings f = (x, y, 1) / |.|
  float conf = 0.0f;
  if (tid < 64) {
    bool lane_bad = false;
    if (pt) {
      const float x = kp[(size_t)b * nk + 2 * (tid + 1)], y = kp[(size_t)b * nk + 2 * (tid + 1) + 1];
      double uo, vo;
      undistort_point(dist, fu, fv, uc, vc, x * nu, y * nv, uo, vo);
      conf = weights ? weights[(size_t)b * n + tid] : 1.0f;
      lane_bad = !(fabs(uo) < INFINITY && fabs(vo) < INFINITY && conf >= 0.0f && conf < INFINITY);
      const double bx = ddiv(uo - uc, fu), by = ddiv(vo - vc, fv);
      const double inv = rsq_nr(bx * bx + by * by + 1.0);
      sF[tid][0] = bx * inv;
      sF[tid][1] = by * inv;
      sF[tid][2] = inv;
      sUV[tid][0] = uo;
      sUV[tid][1] = vo;
      sC[tid] = conf;
#pragma unroll
      for (int k = 0; k < 3; ++k) sX[tid][k] = (double)kp3d[3 * tid + k];
    }
    const bool any_bad = __ballot(lane_bad) != 0;
    const int ncand = __popcll(__ballot(pt && conf > 0.0f));
    if (tid == 0) {
      sRow[0] = any_bad ? 1 : 0;
      sRow[1] = ncand;
    }
  }
  __syncthreads();
  if (sRow[0] != 0 || sRow[1] < 3) {   // uniform: no consensus, the pose stays as it came
    if (pt) weights_out[(size_t)b * n + tid] = conf;
    if (pose64 && tid < 12) pose64[12 * (size_t)b + tid] = NAN;
    if (tid == 0) {
      status[b] |= 64;
      if (cost_out) cost_out[b] = NAN;
      if (info) {
        info[4 * b + 0] = 0;
        info[4 * b + 1] = -1;
        info[4 * b + 2] = -1;
        info[4 * b + 3] = 0;
      }
    }
    return;
  }

  // ---- every triple: solve, form the poses, score them
  const int T = n * (n - 1) * (n - 2) / 6;
  double best = INFINITY, bR[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, bt[3] = {0, 0, 0};
  int bkey = INT_MAX, scored = 0;
  for (int tr = tid; tr < T; tr += nthreads) {
    int i = 0, rem = tr;   // the triple of rank tr in lexicographic order; every index stays below n
    while (i < n - 3) {
      const int m = n - 1 - i, cnt = m * (m - 1) / 2;
      if (rem < cnt) break;
      rem -= cnt;
      ++i;
    }
    int j = i + 1;
    while (j < n - 2) {
      const int cnt = n - 1 - j;
      if (rem < cnt) break;
      rem -= cnt;
      ++j;
    }
    const int k = min(j + 1 + rem, n - 1);
    if (!(sC[i] > 0.0f && sC[j] > 0.0f && sC[k] > 0.0f)) continue;

    double Xi[3], dj[3], dk[3], djk[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      Xi[a] = sX[i][a];
      dj[a] = sX[j][a] - Xi[a];
      dk[a] = sX[k][a] - Xi[a];
      djk[a] = sX[j][a] - sX[k][a];
    }
    const double a2 = djk[0] * djk[0] + djk[1] * djk[1] + djk[2] * djk[2];
    const double b2 = dk[0] * dk[0] + dk[1] * dk[1] + dk[2] * dk[2];
    const double c2 = dj[0] * dj[0] + dj[1] * dj[1] + dj[2] * dj[2];
    const double nm[3] = {dj[1] * dk[2] - dj[2] * dk[1], dj[2] * dk[0] - dj[0] * dk[2], dj[0] * dk[1] - dj[1] * dk[0]};
    const double nm2 = nm[0] * nm[0] + nm[1] * nm[1] + nm[2] * nm[2];
    const double lim = CONS_DEGENERATE * fmax(a2, fmax(b2, c2));
    if (!(nm2 > lim * lim)) continue;
    const double ic = rsq_nr(c2), inm = rsq_nr(nm2);
    const double m1[3] = {dj[0] * ic, dj[1] * ic, dj[2] * ic};
    const double m3[3] = {nm[0] * inm, nm[1] * inm, nm[2] * inm};
    const double m2[3] = {m3[1] * m1[2] - m3[2] * m1[1], m3[2] * m1[0] - m3[0] * m1[2], m3[0] * m1[1] - m3[1] * m1[0]};

    double fi[3], fj[3], fk[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      fi[a] = sF[i][a];
      fj[a] = sF[j][a];
      fk[a] = sF[k][a];
    }
    const double ca = fj[0] * fk[0] + fj[1] * fk[1] + fj[2] * fk[2];
    const double cb = fi[0] * fk[0] + fi[1] * fk[1] + fi[2] * fk[2];
    const double cg = fi[0] * fj[0] + fi[1] * fj[1] + fi[2] * fj[2];
    const double ib2 = rcp_nr(b2);
    const double qq = (a2 - c2) * ib2, pp = (a2 + c2) * ib2, ab = a2 * ib2, cbb = c2 * ib2;
    const double bmc = (b2 - c2) * ib2, bma = (b2 - a2) * ib2;
    const double ca2 = ca * ca, cg2 = cg * cg;
    const double A4 = (qq - 1.0) * (qq - 1.0) - 4.0 * cbb * ca2;
    const double A3 = 4.0 * (qq * (1.0 - qq) * cb - (1.0 - pp) * ca * cg + 2.0 * cbb * ca2 * cb);
    const double A2 = 2.0 * (qq * qq - 1.0 + 2.0 * qq * qq * cb * cb + 2.0 * bmc * ca2 - 4.0 * pp * ca * cb * cg +
                             2.0 * bma * cg2);
    const double A1 = 4.0 * (-qq * (1.0 + qq) * cb + 2.0 * ab * cg2 * cb - (1.0 - pp) * ca * cg);
    const double A0 = (1.0 + qq) * (1.0 + qq) - 4.0 * ab * cg2;
    double v0, v1, v2, v3;
    quartic_roots(A4, A3, A2, A1, A0, v0, v1, v2, v3);
    const double bl = dsqrt(b2);

#pragma unroll 1
    for (int root = 0; root < 4; ++root) {
      const double v = root == 0 ? v0 : root == 1 ? v1 : root == 2 ? v2 : v3;
      if (!(v > 0.0 && v < INFINITY)) continue;
      const double den = 2.0 * (cg - v * ca);
      const double u = ddiv((qq - 1.0) * v * v - 2.0 * qq * cb * v + 1.0 + qq, den);
      if (!(den != 0.0 && u > 0.0 && u < INFINITY)) continue;
      double s1 = bl * rsq_nr(1.0 + v * v - 2.0 * v * cb);
      double s2 = u * s1, s3 = v * s1;
#pragma unroll
      for (int it = 0; it < CONS_POLISH_STEPS; ++it) polish_step(s1, s2, s3, ca, cb, cg, a2, b2, c2);
      if (!(s1 > 0.0 && s2 > 0.0 && s3 > 0.0)) continue;
      double Yi[3], d1[3], d2[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        Yi[a] = s1 * fi[a];
        d1[a] = s2 * fj[a] - Yi[a];
        d2[a] = s3 * fk[a] - Yi[a];
      }
      const double nc[3] = {d1[1] * d2[2] - d1[2] * d2[1], d1[2] * d2[0] - d1[0] * d2[2], d1[0] * d2[1] - d1[1] * d2[0]};
      const double l1 = d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2];
      const double l3 = nc[0] * nc[0] + nc[1] * nc[1] + nc[2] * nc[2];
      if (!(l1 > 0.0 && l3 > 0.0 && l1 < INFINITY && l3 < INFINITY)) continue;
      const double i1 = rsq_nr(l1), i3 = rsq_nr(l3);
      const double e1[3] = {d1[0] * i1, d1[1] * i1, d1[2] * i1};
      const double e3[3] = {nc[0] * i3, nc[1] * i3, nc[2] * i3};
      const double e2[3] = {e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]};
      double R[3][3], t[3];
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[a][c] = e1[a] * m1[c] + e2[a] * m2[c] + e3[a] * m3[c];
#pragma unroll
      for (int a = 0; a < 3; ++a) t[a] = Yi[a] - (R[a][0] * Xi[0] + R[a][1] * Xi[1] + R[a][2] * Xi[2]);
      ++scored;
      double cost = 0.0;
      bool front = true;
      for (int p = 0; p < n; ++p) {
        const double X0 = sX[p][0], X1 = sX[p][1], X2 = sX[p][2];
        const double z = R[2][0] * X0 + R[2][1] * X1 + R[2][2] * X2 + t[2];
        front = front && z > 0.0;
        const double iz = rcp_nr(z);
        const double ru = fu * ((R[0][0] * X0 + R[0][1] * X1 + R[0][2] * X2 + t[0]) * iz) + uc - sUV[p][0];
        const double rv = fv * ((R[1][0] * X0 + R[1][1] * X1 + R[1][2] * X2 + t[1]) * iz) + vc - sUV[p][1];
        if (sC[p] > 0.0f) cost += fmin(ru * ru + rv * rv, tau2);
      }
      if (front && cost < best) {   // keys rise along a thread's own loop: strict < keeps the lowest on a tie
        best = cost;
        bkey = 4 * tr + root;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          bt[a] = t[a];
#pragma unroll
          for (int c = 0; c < 3; ++c) bR[a][c] = R[a][c];
        }
      }
    }
  }

  // ---- arg-min over the workgroup, in a fixed pattern
  double wc = best;
  int wk = bkey, wn = scored;
  argmin_wave(wc, wk, wn);
  const int nw = nthreads >> 6;
  if ((tid & 63) == 0) {
    sCost[tid >> 6] = wc;
    sKey[tid >> 6] = wk;
    sCnt[tid >> 6] = wn;
  }
  __syncthreads();
  double gc = sCost[0];
  int gk = sKey[0], gn = sCnt[0];
  for (int w = 1; w < nw; ++w) {
    argmin_take(gc, gk, sCost[w], sKey[w]);
    gn += sCnt[w];
  }
  const bool found = gk != INT_MAX;
  if (found && bkey == gk) {   // one thread: keys are unique
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      sPose[9 + a] = bt[a];
#pragma unroll
      for (int c = 0; c < 3; ++c) sPose[3 * a + c] = bR[a][c];
    }
  }
  __syncthreads();
  if (tid >= 64) return;

  // ---- inliers of the winner (the first n lanes of wave 0), accept, write
  bool inl = false;
  if (pt && found && conf > 0.0f) {
    const double X0 = sX[tid][0], X1 = sX[tid][1], X2 = sX[tid][2];
    const double z = sPose[6] * X0 + sPose[7] * X1 + sPose[8] * X2 + sPose[11];
    const double iz = rcp_nr(z);
    const double ru = fu * ((sPose[0] * X0 + sPose[1] * X1 + sPose[2] * X2 + sPose[9]) * iz) + uc - sUV[tid][0];
    const double rv = fv * ((sPose[3] * X0 + sPose[4] * X1 + sPose[5] * X2 + sPose[10]) * iz) + vc - sUV[tid][1];
    inl = ru * ru + rv * rv < tau2;
  }
  const int ninl = __popcll(__ballot(inl));
  const bool okay = found && ninl >= min_inliers;
  if (pt) weights_out[(size_t)b * n + tid] = okay ? (inl ? conf : 0.0f) : conf;
  if (pose64 && tid < 12) pose64[12 * (size_t)b + tid] = okay ? sPose[tid] : NAN;
  if (tid != 0) return;
  if (info) {
    info[4 * b + 0] = okay ? ninl : 0;
    info[4 * b + 1] = okay ? gk >> 2 : -1;
    info[4 * b + 2] = okay ? gk & 3 : -1;
    info[4 * b + 3] = gn;
  }
  if (cost_out) cost_out[b] = okay ? (float)gc : NAN;
  if (!okay) {
    status[b] |= 64;
    return;
  }
  double R[3][3], qo[4], qs[4];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) R[a][c] = sPose[3 * a + c];
  dcm2quat(R, qo);
  const double no = sqrt(qo[0] * qo[0] + qo[1] * qo[1] + qo[2] * qo[2] + qo[3] * qo[3]);
#pragma unroll
  for (int k = 0; k < 4; ++k) qs[k] = (double)quat[4 * b + k];
  const double ns = qs[0] * qs[0] + qs[1] * qs[1] + qs[2] * qs[2] + qs[3] * qs[3];
  const bool start_ok = ns > 0.0 && ns < INFINITY;   // finite and nonzero
  const double dot = qo[0] * qs[0] + qo[1] * qs[1] + qo[2] * qs[2] + qo[3] * qs[3];
  const double sg = (start_ok && dot < 0.0) ? -1.0 : 1.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) quat[4 * b + k] = (float)(sg * (qo[k] / no));
#pragma unroll
  for (int k = 0; k < 3; ++k) pos[3 * b + k] = (float)sPose[9 + k];
}

hipError_t launch_consensus(const float* kp, const float* weights, int B, int n, const float* kp3d, const double* K,
                            float nu, float nv, const EpnpDist& dist, float inlier_px, int min_inliers, float* quat,
                            float* pos, float* weights_out, int* info, float* cost, double* pose64, int* status,
                            hipStream_t s) {
  if (n < 4 || n > EPNP_MAXN) return hipErrorInvalidValue;
  const int T = n * (n - 1) * (n - 2) / 6;
  const int threads = T >= 256 ? 256 : (T + 63) / 64 * 64;   // one triple per thread up to 256; 4 .. 560 triples
  consensus_kernel<<<B, threads, 0, s>>>(kp, weights, B, n, kp3d, K[0], K[4], K[2], K[5], nu, nv, dist, inlier_px,
                                         min_inliers, quat, pos, weights_out, info, cost, pose64, status);
  return hipGetLastError();
}

}  // namespace spef
