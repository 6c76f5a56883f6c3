// Multi-hypothesis orientation decode on gfx950 (spef_decode_modes; the NumPy twin and the specification is
// spef_amd/spe/modes.py, which states every step).
//
//   decode_modes_kernel  per row: up to k_max orientations that the soft-classification PDF holds at once -- seeds by
//                        greedy suppression, `rounds` Lloyd rounds of (assign every bin to the mode of largest
//                        |q_i . m_k|, m_k <- the Markley average of its cluster), a prune by mass and separation, and a
//                        final assignment whose clusters give each mode its quaternion, its mass and its theta block
//                        (the one of k_cov.hip, restricted to the cluster's bins, about the mode).
// One 256-thread workgroup per row. The bins are read in strided loops (any table size); nothing is kept per bin: the
// alive test of the seeding is recomputed from the <= 4 seeds, the assignment from the <= 4 modes. Per pass a thread
// accumulates, in fp64, what every cluster needs (the packed 4 x 4 moment matrix and the mass; the mass alone for the
// prune; the 6 entries of the theta block) for up to 4 clusters in registers -- a bin adds its value to its own
// cluster and an exact 0.0 to the others, so no accumulator is indexed dynamically -- and the workgroup's partials are
// reduced cluster by cluster in the fixed order of cov_reduce (LDS, then DPP inside 16-lane rows): 11 x 256 doubles of
// LDS, 22 KB. Lanes 0..3 then take one cluster's top eigenvector each. The seeding's argmax is a fixed-order
// (value, index) reduction through LDS (the larger float32 value, then the lower index: associative, so the tree's
// shape does not matter). Lane 0 does the serial tails (prune, ordering, float32 casts). No atomics, no allocation; a
// row's result does not depend on the batch it is in.
#include <math.h>

#include "spef_common.hpp"
#include "spef_eig.hpp"
#include "spef_kernels.hpp"
#include "spef_pose_math.hpp"
#include "spef_reduce.hpp"

namespace spef {

constexpr int MD_MOM = 11;   // a cluster's 10 packed moments of sum p q q^T, then its mass

// |q . m| with every product and sum rounded on its own, left to right (no fused multiply-add): the value the twin's
// NumPy expression has, bit for bit. While the modes are still the seeds -- rows of the table, the same on both sides --
// the suppression and the assignment therefore decide as the twin does even on an exact tie, and the Euler-angle grid is
// symmetric enough to put a large share of a PDF's mass on bins that are exactly as close to one seed as to another.
__device__ __forceinline__ double modes_absdot(const double4& q, const double* m) {
#pragma clang fp contract(off)
  return fabs(((q.x * m[0] + q.y * m[1]) + q.z * m[2]) + q.w * m[3]);
}

struct ModesMoments {   // v = p (q q^T packed, 1)
  static constexpr int N = MD_MOM;
  __device__ __forceinline__ void operator()(const double4& q, double p, int, double (&v)[N]) const {
    v[0] = (q.x * q.x) * p; v[1] = (q.x * q.y) * p; v[2] = (q.x * q.z) * p; v[3] = (q.x * q.w) * p;
    v[4] = (q.y * q.y) * p; v[5] = (q.y * q.z) * p; v[6] = (q.y * q.w) * p;
    v[7] = (q.z * q.z) * p; v[8] = (q.z * q.w) * p; v[9] = (q.w * q.w) * p;
    v[10] = p;
  }
};

struct ModesMass {      // v = p
  static constexpr int N = 1;
  __device__ __forceinline__ void operator()(const double4&, double p, int, double (&v)[N]) const { v[0] = p; }
};

struct ModesTheta {     // v = p theta theta^T (upper triangle), theta = Log(q (x) conj(m_a)): the expressions of k_cov.hip
  static constexpr int N = 6;
  const double (*mn)[4];   // the modes, normalised (LDS)
  __device__ __forceinline__ void operator()(const double4& q, double p, int a, double (&v)[N]) const {
    const double* qh = mn[a];
    double d0 = q.x * qh[0] + q.y * qh[1] + q.z * qh[2] + q.w * qh[3];
    double d1 = -q.x * qh[1] + q.y * qh[0] - q.z * qh[3] + q.w * qh[2];
    double d2 = -q.x * qh[2] + q.y * qh[3] + q.z * qh[0] - q.w * qh[1];
    double d3 = -q.x * qh[3] - q.y * qh[2] + q.z * qh[1] + q.w * qh[0];
    if (d0 < 0.0) { d0 = -d0; d1 = -d1; d2 = -d2; d3 = -d3; }
    const double n2 = d1 * d1 + d2 * d2 + d3 * d3;
    const double n = dsqrt(n2);
    const double f = n < 1e-8 ? 2.0 / d0 * (1.0 - n2 / (3.0 * d0 * d0)) : 2.0 * atan2(n, d0) * rcp_nr(n);
    const double w = (f * f) * p;
    v[0] = (d1 * d1) * w; v[1] = (d1 * d2) * w; v[2] = (d1 * d3) * w;
    v[3] = (d2 * d2) * w; v[4] = (d2 * d3) * w; v[5] = (d3 * d3) * w;
  }
};

// One pass over the row's bins: bin i belongs to the mode of largest |q_i . m_k| among the K in sm (ties to the lowest
// k); out[F::N * k + j] = the sum over cluster k of f's value j. Ends on a barrier (K >= 1).
template <class F>
__device__ void modes_pass(const float* __restrict__ x, const double* __restrict__ qb, int n, int K,
                           const double (*sm)[4], double (*shd)[256], double* out, const F& f) {
  constexpr int N = F::N;
  const int tid = threadIdx.x;
  double acc[MODES_MAX][N];
#pragma unroll
  for (int k = 0; k < MODES_MAX; ++k)
#pragma unroll
    for (int j = 0; j < N; ++j) acc[k][j] = 0.0;
  for (int i = tid; i < n; i += 256) {
    const double p = (double)x[i];
    const double4 q = *reinterpret_cast<const double4*>(qb + 4 * (size_t)i);
    int a = 0;
    double best = modes_absdot(q, sm[0]);
#pragma unroll
    for (int k = 1; k < MODES_MAX; ++k) {
      if (k < K) {
        const double d = modes_absdot(q, sm[k]);
        if (d > best) {
          best = d;
          a = k;
        }
      }
    }
    double v[N];
    f(q, p, a, v);
#pragma unroll
    for (int k = 0; k < MODES_MAX; ++k)
#pragma unroll
      for (int j = 0; j < N; ++j) acc[k][j] += a == k ? v[j] : 0.0;
  }
#pragma unroll
  for (int k = 0; k < MODES_MAX; ++k) {
    if (k < K) {   // uniform
#pragma unroll
      for (int j = 0; j < N; ++j) shd[j][tid] = acc[k][j];
      __syncthreads();
      cov_reduce(shd, out + N * k, N);
    }
  }
}

// Lanes 0..K-1: the Markley average of cluster k from its reduced moments (a cluster without positive mass keeps its
// mode). Ends on a barrier.
__device__ __forceinline__ void modes_eig(int K, const double* mom, double (*sm)[4]) {
  const int tid = threadIdx.x;
  if (tid < K && mom[MD_MOM * tid + 10] > 0.0) {
    double q[4];
    sym4_top_eigvec(mom + MD_MOM * tid, q);
#pragma unroll
    for (int c = 0; c < 4; ++c) sm[tid][c] = q[c];
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void decode_modes_kernel(const float* __restrict__ pdf, int n,
                                                           const double* __restrict__ qb, ModesParams prm,
                                                           float* __restrict__ mode_quat, float* __restrict__ mode_mass,
                                                           float* __restrict__ mode_cov, int* __restrict__ n_modes,
                                                           int* __restrict__ modes_status) {
  __shared__ double shd[MD_MOM][256];
  __shared__ double shp[MODES_MAX * MD_MOM];
  __shared__ double sm[MODES_MAX][4], sfin[MODES_MAX][4], smn[MODES_MAX][4], smass[MODES_MAX], stot[1];
  __shared__ float sbv[256];
  __shared__ int sbi[256];
  __shared__ int sK, sseed[MODES_MAX];
  const int tid = threadIdx.x, kmax = prm.k_max;
  const size_t b = blockIdx.x;
  const float* x = pdf + b * (size_t)n;
  float* oq = mode_quat + b * (size_t)(4 * kmax);
  float* om = mode_mass + b * (size_t)kmax;
  float* oc = mode_cov + b * (size_t)(9 * kmax);

  // ---- 0. sum p: a NaN or an infinity anywhere in p makes it NaN or infinite
  {
    double sp = 0.0;
    for (int i = tid; i < n; i += 256) sp += (double)x[i];
    shd[0][tid] = sp;
    __syncthreads();
    cov_reduce(shd, stot, 1);
  }
  const double total = stot[0];
  if (!(total > 0.0 && total < INFINITY)) {   // uniform
    for (int e = tid; e < 14 * kmax; e += 256) {
      if (e < 4 * kmax) oq[e] = NAN;
      else if (e < 5 * kmax) om[e - 4 * kmax] = NAN;
      else oc[e - 5 * kmax] = NAN;
    }
    if (tid == 0) {
      n_modes[b] = 0;
      modes_status[b] = 1;
    }
    return;
  }

  // ---- 1. seeds: the alive bin of largest p > 0 (float32 compared exactly, ties to the lowest index)
  int K = 0;
  float p0 = 0.0f;
  for (int k = 0; k < kmax; ++k) {
    float bv = 0.0f;
    int bi = 0x7fffffff;
    for (int i = tid; i < n; i += 256) {   // ascending i and a strict >: the lowest index of equal values
      const float p = x[i];
      if (p > bv) {
        const double4 q = *reinterpret_cast<const double4*>(qb + 4 * (size_t)i);
        bool alive = true;   // a seed is never alive again, even where c rounds to 1 and its own |q . q| falls below it
        for (int s = 0; s < K; ++s) alive = alive && i != sseed[s] && modes_absdot(q, sm[s]) < prm.cos_half_sep;
        if (alive) {
          bv = p;
          bi = i;
        }
      }
    }
    sbv[tid] = bv;
    sbi[tid] = bi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) {
        const float ov = sbv[tid + s];
        const int oi = sbi[tid + s];
        if (ov > sbv[tid] || (ov == sbv[tid] && oi < sbi[tid])) {
          sbv[tid] = ov;
          sbi[tid] = oi;
        }
      }
      __syncthreads();
    }
    bv = sbv[0];
    bi = sbi[0];
    __syncthreads();   // every thread has read the winner before the next seed's candidates overwrite it
    if (!(bv > 0.0f)) break;
    if (k > 0 && (double)bv < prm.seed_rel * (double)p0) break;
    if (k == 0) p0 = bv;
    if (tid < 4) sm[k][tid] = qb[4 * (size_t)bi + tid];
    if (tid == 0) sseed[k] = bi;
    K = k + 1;
    __syncthreads();
  }
  // total > 0 and finite: some p > 0, so K >= 1

  // ---- 2. Lloyd rounds
  for (int r = 0; r < prm.rounds; ++r) {
    modes_pass(x, qb, n, K, sm, shd, shp, ModesMoments{});
    modes_eig(K, shp, sm);
  }

  // ---- 3. prune by descending mass (ties to the lowest k); the survivors move up in the order of their k
  modes_pass(x, qb, n, K, sm, shd, shp, ModesMass{});
  if (tid == 0) {
    unsigned used = 0, keep = 0;
    int first = 0;
    for (int r = 0; r < K; ++r) {
      int best = -1;
      for (int k = 0; k < K; ++k)
        if (!(used >> k & 1) && (best < 0 || shp[k] > shp[best])) best = k;
      used |= 1u << best;
      if (r == 0) first = best;
      const double mass = shp[best] / total;
      bool drop = mass < prm.min_mass || !(mass > 0.0);
      for (int j = 0; j < K; ++j)
        if (keep >> j & 1) {
          const double d = fabs(sm[best][0] * sm[j][0] + sm[best][1] * sm[j][1] + sm[best][2] * sm[j][2] +
                                sm[best][3] * sm[j][3]);
          drop = drop || d >= prm.cos_half_sep;
        }
      if (!drop) keep |= 1u << best;
    }
    if (!keep) keep = 1u << first;
    int w = 0;
    for (int k = 0; k < K; ++k)
      if (keep >> k & 1) {
        if (w != k)
          for (int c = 0; c < 4; ++c) sm[w][c] = sm[k][c];
        ++w;
      }
    sK = w;
  }
  __syncthreads();
  K = sK;

  // ---- 4. final clusters: mode, mass, theta block
  // the clusters stay those of sm; their Markley averages go to sfin, about which the theta blocks are taken
  modes_pass(x, qb, n, K, sm, shd, shp, ModesMoments{});
  if (tid < K) smass[tid] = shp[MD_MOM * tid + 10];
  if (tid < 4 * K) sfin[tid >> 2][tid & 3] = sm[tid >> 2][tid & 3];
  __syncthreads();
  modes_eig(K, shp, sfin);
  if (tid < K) {
    const double n2 = (sfin[tid][0] * sfin[tid][0] + sfin[tid][1] * sfin[tid][1]) +
                      (sfin[tid][2] * sfin[tid][2] + sfin[tid][3] * sfin[tid][3]);
    const double s = rsq_nr(n2);
#pragma unroll
    for (int c = 0; c < 4; ++c) smn[tid][c] = sfin[tid][c] * s;
  }
  __syncthreads();
  modes_pass(x, qb, n, K, sm, shd, shp, ModesTheta{smn});
  if (tid != 0) return;
  unsigned used = 0;
  for (int r = 0; r < kmax; ++r) {
    float* q = oq + 4 * r;
    float* c = oc + 9 * r;
    if (r >= K) {
      for (int e = 0; e < 4; ++e) q[e] = NAN;
      for (int e = 0; e < 9; ++e) c[e] = NAN;
      om[r] = NAN;
      continue;
    }
    int best = -1;   // descending mass, stable
    for (int k = 0; k < K; ++k)
      if (!(used >> k & 1) && (best < 0 || smass[k] > smass[best])) best = k;
    used |= 1u << best;
    double sgn = 1.0;
    for (int e = 3; e >= 0; --e)
      if (sfin[best][e] != 0.0) sgn = sfin[best][e] < 0.0 ? -1.0 : 1.0;   // the first non-zero component decides
    for (int e = 0; e < 4; ++e) q[e] = (float)(sgn * sfin[best][e]);
    om[r] = (float)(smass[best] / total);
    const bool ok = smass[best] > 0.0;
    const double inv = 1.0 / smass[best], fl = prm.floor_var;
    const double* t = shp + 6 * best;
    const float xx = ok ? (float)(t[0] * inv + fl) : NAN, xy = ok ? (float)(t[1] * inv) : NAN;
    const float xz = ok ? (float)(t[2] * inv) : NAN, yy = ok ? (float)(t[3] * inv + fl) : NAN;
    const float yz = ok ? (float)(t[4] * inv) : NAN, zz = ok ? (float)(t[5] * inv + fl) : NAN;
    c[0] = xx; c[1] = xy; c[2] = xz;
    c[3] = xy; c[4] = yy; c[5] = yz;
    c[6] = xz; c[7] = yz; c[8] = zz;
  }
  n_modes[b] = K;
  modes_status[b] = 0;
}

hipError_t launch_decode_modes(const float* ori_pdf, int n_ori, const double* q_bins, int B, const ModesParams& prm,
                               float* mode_quat, float* mode_mass, float* mode_cov, int* n_modes, int* modes_status,
                               hipStream_t s) {
  if (B < 1 || n_ori < 1 || prm.k_max < 1 || prm.k_max > MODES_MAX) return hipErrorInvalidValue;
  decode_modes_kernel<<<(unsigned)B, 256, 0, s>>>(ori_pdf, n_ori, q_bins, prm, mode_quat, mode_mass, mode_cov, n_modes,
                                                  modes_status);
  return hipGetLastError();
}

}  // namespace spef
