// Pose scoring on gfx950: SPEUtils.get_score (src/spe/spe_utils.py:103-159), the per-image error lists of
// evaluation() with their std and median absolute deviation (src/tools/evaluation.py:59-99) and the per-video min /
// max / median / mean / std of the temporal tool (temporal.py:27-48), on poses that never leave the device.
//
//   score_step_kernel      one thread per row (time-major: row t * S + s belongs to group s): the row's five values
//                          (pos_err, pos_norm, ori_rad, ori_deg, ori_stable) and flags go to log slot count[s] + t of
//                          (track, s) and, if asked, to the caller's [T * S][5]. The slot is a function of (s, t): no
//                          atomics. A slot at or past the capacity is not written.
//   score_advance_kernel   count[s] += T (clamped to the capacity, the excess counted as dropped): the step needs no
//                          host value and can be stream-captured.
//   score_finalize_kernel  one 256-thread workgroup per (group, track, quantity): the fp64 sums in the fixed order of
//                          spef_reduce.hpp, then a bitonic sort of a scratch copy of the quantity's good rows (the log
//                          itself is only read) for the exact median, median absolute deviation, min and max.
//   score_reset_kernel     clears the counts of one group or of all.
//
// Arithmetic (the host twin spef_amd/score.py states it in NumPy): elementwise float32 with every operation rounded
// on its own (no FMA contraction in this file; IEEE divide), every sum fp64 in a fixed order, acos / sqrt the fp64
// functions rounded to float32. A statistics sum runs over the log's slots, a flagged slot adding 0.0: thread i adds
// slots i, i + 256, ... in order, then block_sum256_d.
//
// The sort: the keys of the m slots (a flagged slot: +inf, so the n good ones come first) are padded with +inf to a
// power of two P. While P fits the LDS tile (SCORE_TILE rows, 32 KiB: five such workgroups fit a CU's 160 KiB, and
// the 1,800 frames of a SPEED validation run fit one tile) the workgroup sorts in LDS and the scratch in global memory
// is not touched. Above that the copy lives in global scratch: every tile is sorted in LDS first, and each later merge
// stage does its strides >= SCORE_TILE in global memory and the rest of the stage tile by tile in LDS, so a log of
// 2^20 rows takes 28 passes over global memory instead of 210.
#include <math.h>

#include "spef_common.hpp"
#include "spef_kernels.hpp"
#include "spef_reduce.hpp"

#pragma clang fp contract(off)

namespace spef {

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < INFINITY; }   // false for NaN

__global__ __launch_bounds__(256) void score_step_kernel(const ScoreLog lg, int track, const float* __restrict__ quat,
                                                         const float* __restrict__ pos, const int* __restrict__ status,
                                                         const float* __restrict__ quat_true,
                                                         const float* __restrict__ pos_true, int T, int S,
                                                         float* __restrict__ rows_out) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= (int64_t)T * S) return;
  const int s = (int)(r % S);
  const int64_t t = r / S;
  const float4 qp = reinterpret_cast<const float4*>(quat)[r];
  const float4 qt = reinterpret_cast<const float4*>(quat_true)[r];
  const float p0 = pos[r * 3], p1 = pos[r * 3 + 1], p2 = pos[r * 3 + 2];
  const float g0 = pos_true[r * 3], g1 = pos_true[r * 3 + 1], g2 = pos_true[r * 3 + 2];

  const float d0 = g0 - p0, d1 = g1 - p1, d2 = g2 - p2;
  const float e0 = d0 * d0, e1 = d1 * d1, e2 = d2 * d2;
  const float pos_err = (float)sqrt((double)(float)(((double)e0 + (double)e1) + (double)e2));
  const float h0 = g0 * g0, h1 = g1 * g1, h2 = g2 * g2;
  const float tnorm = (float)sqrt((double)(float)(((double)h0 + (double)h1) + (double)h2));
  const float pos_norm = pos_err / tnorm;
  const float m0 = qp.x * qt.x, m1 = qp.y * qt.y, m2 = qp.z * qt.z, m3 = qp.w * qt.w;
  const float dot = fabsf((float)((((double)m0 + (double)m1) + (double)m2) + (double)m3));
  const float ac = (float)acos((double)fminf(dot, 1.0f));
  const float ori_rad = 2.0f * ac;
  const float ori_deg = (ori_rad * 180.0f) / 3.14159274101257324f;   // float32(pi)
  // the stable angle in fp64: 2 atan2(|qp - s qt|, |qp + s qt|), s = sign(qp . qt)
  const double a0 = qp.x, a1 = qp.y, a2 = qp.z, a3 = qp.w, b0 = qt.x, b1 = qt.y, b2 = qt.z, b3 = qt.w;
  const double dd = ((a0 * b0 + a1 * b1) + a2 * b2) + a3 * b3;
  const double sg = dd < 0.0 ? -1.0 : 1.0;
  const double n0 = a0 - sg * b0, n1 = a1 - sg * b1, n2 = a2 - sg * b2, n3 = a3 - sg * b3;
  const double u0 = a0 + sg * b0, u1 = a1 + sg * b1, u2 = a2 + sg * b2, u3 = a3 + sg * b3;
  const double nm = sqrt(((n0 * n0 + n1 * n1) + n2 * n2) + n3 * n3);
  const double np = sqrt(((u0 * u0 + u1 * u1) + u2 * u2) + u3 * u3);
  const float ori_stable = (float)(2.0 * atan2(nm, np));

  int flags = 0;
  if (dot > 1.01f) flags |= 1;
  const bool fin = finite_f(qp.x) && finite_f(qp.y) && finite_f(qp.z) && finite_f(qp.w) && finite_f(qt.x) &&
                   finite_f(qt.y) && finite_f(qt.z) && finite_f(qt.w) && finite_f(p0) && finite_f(p1) &&
                   finite_f(p2) && finite_f(g0) && finite_f(g1) && finite_f(g2);
  if (!fin) flags |= 2;
  if (tnorm == 0.0f) flags |= 4;
  if (status && status[r] != 0) flags |= 8;
  float v[5] = {pos_err, pos_norm, ori_rad, ori_deg, ori_stable};
  if (flags) {
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = NAN;
  }
  if (rows_out) {
#pragma unroll
    for (int k = 0; k < 5; ++k) rows_out[r * 5 + k] = v[k];
  }
  const int64_t slot = (int64_t)lg.count[track * S + s] + t;
  if (slot < (int64_t)lg.capacity) {   // the index check comes before the store
    const size_t at = ((size_t)track * S + s) * lg.capacity + (size_t)slot;
#pragma unroll
    for (int k = 0; k < 5; ++k) lg.rows[at * 5 + k] = v[k];
    lg.flags[at] = flags;
  }
}

// count / dropped: [n_tracks][n_groups]
__global__ void score_advance_kernel(const ScoreLog lg, int track, int T, int S) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  const int64_t c = (int64_t)lg.count[track * S + s] + T;
  if (c > (int64_t)lg.capacity) {
    lg.dropped[track * S + s] += (long long)(c - lg.capacity);
    lg.count[track * S + s] = lg.capacity;
  } else {
    lg.count[track * S + s] = (int)c;
  }
}

__global__ void score_reset_kernel(const ScoreLog lg, int n_tracks, int group) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_tracks * lg.n_groups) return;
  if (group < 0 || idx % lg.n_groups == group) {
    lg.count[idx] = 0;
    lg.dropped[idx] = 0;
  }
}

// ------------------------------------------------------------------------------------------ statistics
// One compare-exchange step of the bitonic network on x[0, len): element i pairs with i ^ j; the direction is that
// of the element's place `base + i` in the whole array (base = 0 for the whole array, the tile's offset for a tile).
__device__ __forceinline__ void bitonic_step(float* x, unsigned len, unsigned base, unsigned k, unsigned j) {
  for (unsigned p = threadIdx.x; p < (len >> 1); p += 256) {
    const unsigned i = ((p & ~(j - 1)) << 1) | (p & (j - 1));   // the pair's lower index: bit j clear
    const unsigned l = i | j;
    const float a = x[i], b = x[l];
    const bool up = ((base + i) & k) == 0;
    if ((a > b) == up) {
      x[i] = b;
      x[l] = a;
    }
  }
  __syncthreads();
}

// Sort P (a power of two) keys ascending. P <= SCORE_TILE: the keys are in `tile` (LDS) and stay there. Otherwise
// they are in `g` (global scratch of this workgroup) and `tile` is the staging buffer.
__device__ void bitonic_sort(float* tile, float* g, unsigned P) {
  if (P <= SCORE_TILE) {
    for (unsigned k = 2; k <= P; k <<= 1)
      for (unsigned j = k >> 1; j > 0; j >>= 1) bitonic_step(tile, P, 0, k, j);
    return;
  }
  for (unsigned base = 0; base < P; base += SCORE_TILE) {   // every stage up to the tile size, tile by tile
    for (unsigned i = threadIdx.x; i < SCORE_TILE; i += 256) tile[i] = g[base + i];
    __syncthreads();
    for (unsigned k = 2; k <= SCORE_TILE; k <<= 1)
      for (unsigned j = k >> 1; j > 0; j >>= 1) bitonic_step(tile, SCORE_TILE, base, k, j);
    for (unsigned i = threadIdx.x; i < SCORE_TILE; i += 256) g[base + i] = tile[i];
    __syncthreads();
  }
  for (unsigned k = 2 * SCORE_TILE; k <= P; k <<= 1) {
    for (unsigned j = k >> 1; j >= SCORE_TILE; j >>= 1) bitonic_step(g, P, 0, k, j);
    for (unsigned base = 0; base < P; base += SCORE_TILE) {
      for (unsigned i = threadIdx.x; i < SCORE_TILE; i += 256) tile[i] = g[base + i];
      __syncthreads();
      for (unsigned j = SCORE_TILE >> 1; j > 0; j >>= 1) bitonic_step(tile, SCORE_TILE, base, k, j);
      for (unsigned i = threadIdx.x; i < SCORE_TILE; i += 256) g[base + i] = tile[i];
      __syncthreads();
    }
  }
}

// np.median of the n smallest of sorted keys: the middle one, or (a + b) * 0.5 in float32
__device__ __forceinline__ float median_sorted(const float* x, int n) {
  return (n & 1) ? x[n >> 1] : (x[(n >> 1) - 1] + x[n >> 1]) * 0.5f;
}

__device__ __forceinline__ double slot_sum(const ScoreLog& lg, size_t at0, int m, int col, double* sh) {
  double a = 0.0;
  for (int i = threadIdx.x; i < m; i += 256)
    a += lg.flags[at0 + i] ? 0.0 : (double)lg.rows[(at0 + i) * 5 + col];
  const double r = block_sum256_d(a, sh);
  __syncthreads();   // sh is free again
  return r;
}

// sum over the good slots of ((double)x - mean)^2
__device__ __forceinline__ double slot_dev2(const ScoreLog& lg, size_t at0, int m, int col, double mean, double* sh) {
  double a = 0.0;
  for (int i = threadIdx.x; i < m; i += 256) {
    const double d = (double)lg.rows[(at0 + i) * 5 + col] - mean;
    a += lg.flags[at0 + i] ? 0.0 : d * d;
  }
  const double r = block_sum256_d(a, sh);
  __syncthreads();
  return r;
}

// grid (n_groups, n_tracks, 2): z = 0 orientation (ori_deg; also the counts and the three scores), 1 position
// (pos_err). stats [n_groups][n_tracks][SCORE_FIELDS].
__global__ __launch_bounds__(256) void score_finalize_kernel(const ScoreLog lg, int n_tracks, float* scratch,
                                                             unsigned scratch_stride, double* stats) {
  __shared__ float tile[SCORE_TILE];
  __shared__ double shd[4];
  __shared__ int shi[4];
  const int g = blockIdx.x, track = blockIdx.y, q = blockIdx.z, tid = threadIdx.x;
  const int G = lg.n_groups;
  const int m = min(lg.count[track * G + g], lg.capacity);
  const size_t at0 = ((size_t)track * G + g) * lg.capacity;
  double* out = stats + ((size_t)g * n_tracks + track) * SCORE_FIELDS;
  const int col = q ? 0 : 3;   // pos_err / ori_deg

  // counts
  int good = 0, fl = 0;
  for (int i = tid; i < m; i += 256) {
    const int f = lg.flags[at0 + i];
    good += f == 0;
    fl |= f;
  }
  for (int o = 32; o > 0; o >>= 1) {
    good += __shfl_xor(good, o, 64);
    fl |= __shfl_xor(fl, o, 64);
  }
  if ((tid & 63) == 0) shi[tid >> 6] = good;
  __syncthreads();
  const int n = (shi[0] + shi[1]) + (shi[2] + shi[3]);
  __syncthreads();
  if ((tid & 63) == 0) shi[tid >> 6] = fl;
  __syncthreads();
  fl = (shi[0] | shi[1]) | (shi[2] | shi[3]);

  if (q == 0 && tid == 0) {
    out[SF_N] = (double)n;
    out[SF_N_BAD] = (double)(m - n);
    out[SF_N_DROPPED] = (double)lg.dropped[track * G + g];
    out[SF_FLAGS] = (double)fl;
  }
  const double nan = __builtin_nan("");
  if (n == 0) {   // uniform over the workgroup
    if (tid == 0) {
      if (q == 0) {
        out[SF_ORI_SCORE] = out[SF_POS_SCORE] = out[SF_ESA_SCORE] = out[SF_ORI_ERROR] = nan;
        out[SF_ORI_STD] = out[SF_ORI_MEDIAN] = out[SF_ORI_MAD] = out[SF_ORI_MIN] = out[SF_ORI_MAX] = nan;
      } else {
        out[SF_POS_ERROR] = out[SF_POS_STD] = out[SF_POS_MEDIAN] = out[SF_POS_MAD] = nan;
        out[SF_POS_MIN] = out[SF_POS_MAX] = nan;
      }
    }
    return;
  }
  const double dn = (double)n;
  const double mean = slot_sum(lg, at0, m, col, shd) / dn;
  const double sd = sqrt(slot_dev2(lg, at0, m, col, mean, shd) / dn);
  if (q == 0) {
    const double ori_score = slot_sum(lg, at0, m, 2, shd) / dn;
    const double pos_score = slot_sum(lg, at0, m, 1, shd) / dn;
    if (tid == 0) {
      out[SF_ORI_SCORE] = ori_score;
      out[SF_POS_SCORE] = pos_score;
      out[SF_ESA_SCORE] = ori_score + pos_score;
      out[SF_ORI_ERROR] = (ori_score * 180.0) / 3.14159265358979323846;
      out[SF_ORI_STD] = sd;
    }
  } else if (tid == 0) {
    out[SF_POS_ERROR] = mean;
    out[SF_POS_STD] = sd;
  }

  // order statistics on a scratch copy
  unsigned P = 1;
  while (P < (unsigned)m) P <<= 1;
  const bool in_lds = P <= SCORE_TILE;
  float* gs = scratch ? scratch + ((size_t)(g * n_tracks + track) * 2 + q) * scratch_stride : nullptr;
  float* x = in_lds ? tile : gs;   // P > SCORE_TILE only when capacity > SCORE_TILE: the launcher then gives scratch
  for (unsigned i = tid; i < P; i += 256)
    x[i] = (i < (unsigned)m && lg.flags[at0 + i] == 0) ? lg.rows[(at0 + i) * 5 + col] : INFINITY;
  __syncthreads();
  bitonic_sort(tile, gs, P);
  const float lo = x[0], hi = x[n - 1], med = median_sorted(x, n);
  __syncthreads();   // everyone has read the median
  for (unsigned i = tid; i < P; i += 256) x[i] = i < (unsigned)n ? fabsf(x[i] - med) : INFINITY;
  __syncthreads();
  bitonic_sort(tile, gs, P);
  if (tid == 0) {
    const float mad = median_sorted(x, n);
    out[q ? SF_POS_MEDIAN : SF_ORI_MEDIAN] = (double)med;
    out[q ? SF_POS_MAD : SF_ORI_MAD] = (double)mad;
    out[q ? SF_POS_MIN : SF_ORI_MIN] = (double)lo;
    out[q ? SF_POS_MAX : SF_ORI_MAX] = (double)hi;
  }
}

// Copy `n` log slots from `first` of (track, group) to the caller (the parity tests read the log through this).
__global__ void score_read_kernel(const ScoreLog lg, int track, int group, int first, int n, float* rows, int* flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t at = ((size_t)track * lg.n_groups + group) * lg.capacity + (size_t)first + i;
#pragma unroll
  for (int k = 0; k < 5; ++k) rows[(size_t)i * 5 + k] = lg.rows[at * 5 + k];
  flags[i] = lg.flags[at];
}

// ------------------------------------------------------------------------------------------ launchers
hipError_t launch_score_step(const ScoreLog& lg, int track, const float* quat, const float* pos, const int* status,
                             const float* quat_true, const float* pos_true, int T, int S, float* rows_out,
                             hipStream_t s) {
  const int64_t rows = (int64_t)T * S;
  if (T < 1 || S != lg.n_groups || rows > 0x7fffffff) return hipErrorInvalidValue;
  score_step_kernel<<<(unsigned)((rows + 255) / 256), 256, 0, s>>>(lg, track, quat, pos, status, quat_true, pos_true,
                                                                   T, S, rows_out);
  score_advance_kernel<<<(S + 255) / 256, 256, 0, s>>>(lg, track, T, S);
  return hipGetLastError();
}

hipError_t launch_score_reset(const ScoreLog& lg, int n_tracks, int group, hipStream_t s) {
  score_reset_kernel<<<(n_tracks * lg.n_groups + 255) / 256, 256, 0, s>>>(lg, n_tracks, group);
  return hipGetLastError();
}

hipError_t launch_score_finalize(const ScoreLog& lg, int n_tracks, float* scratch, unsigned scratch_stride,
                                 double* stats, hipStream_t s) {
  if (lg.capacity > SCORE_TILE && !scratch) return hipErrorInvalidValue;
  score_finalize_kernel<<<dim3(lg.n_groups, n_tracks, 2), 256, 0, s>>>(lg, n_tracks, scratch, scratch_stride, stats);
  return hipGetLastError();
}

hipError_t launch_score_read(const ScoreLog& lg, int track, int group, int first, int n, float* rows, int* flags,
                             hipStream_t s) {
  if (n < 1) return hipSuccess;
  score_read_kernel<<<(n + 255) / 256, 256, 0, s>>>(lg, track, group, first, n, rows, flags);
  return hipGetLastError();
}

}  // namespace spef
