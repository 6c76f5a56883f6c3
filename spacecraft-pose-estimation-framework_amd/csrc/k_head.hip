// Head and decode kernels on gfx950.
//
//   fc_kernel          URSONetHead Linear layers (src/modeling/head/ursonet.py:17-25), ori and pos weights
//                      concatenated into one fp32 GEMM on the exact f32-input MFMA (v_mfma_f32_16x16x4_f32)
//   decode_ori_kernel  SPEUtils.last_activ softmax (src/spe/spe_utils.py:75-76) fused with
//                      OrientationSoftClassification.decode (src/spe/classification_utils.py:113-146):
//                      a = sum_i p_i q_i q_i^T in fp64, top eigenvector by repeated squaring, normalised
//   decode_pos_kernel  softmax (spe_utils.py:78-79) + PositionSoftClassification.decode
//                      (classification_utils.py:242-267): 3-D soft-argmax over the bin grid
//   normalize_ori      orientation regression L2 normalisation (spe_utils.py:72)
// One 256-thread workgroup decodes one image (the reference loops over images in Python,
// classification_utils.py:163-164); the orientation decode supports up to 8192 bins.
#include <math.h>

#include "spef_common.hpp"
#include "spef_eig.hpp"
#include "spef_kernels.hpp"
#include "spef_reduce.hpp"

namespace spef {

// ------------------------------------------------------------------------------------------ fc
// out[b][i] = sum_k X[b][k] W[i][k] + bias[i]. One workgroup per 16x16 output tile; its 4 waves take
// interleaved quarters of K (split-K inside the workgroup, reduced through LDS in a fixed order, so the
// result is deterministic). Lane l loads float4 W[i0+(l&15)][t+4(l>>4)..] and X[j0+(l&15)][t+4(l>>4)..];
// MFMA step e takes element e from both, so A and B see the same k.
// 1-D grid, XCD-aware: the nJ image groups of one 16-row weight tile are consecutive logical ids, which
// xcd_remap places on one XCD, so the fp32 weight (8.85 MB for 1728 bins) is fetched from HBM once per batch
// and re-read from that XCD's L2 by the other image groups (round-robin placement fetched it once per group).
__global__ __launch_bounds__(256) void fc_kernel(const float* __restrict__ X, const float* __restrict__ W,
                                                 const float* __restrict__ bias, float* __restrict__ out0, int n0,
                                                 float* __restrict__ out1, int n1, int B, int K, int Np) {
  __shared__ f32x4 part[4][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t nJ = (uint32_t)(B + 15) / 16;
  const uint32_t L = xcd_remap(blockIdx.x, gridDim.x);
  const int i0 = (int)(L / nJ) * 16;
  const int j0 = (int)(L % nJ) * 16;
  const int r16 = lane & 15, kg = lane >> 4;
  const float* wp = W + (size_t)(i0 + r16) * K + 4 * kg;
  const int j = j0 + r16;
  const bool jv = j < B;
  const float* xp = X + (size_t)(jv ? j : 0) * K + 4 * kg;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int t = 16 * wave; t < K; t += 64) {
    const float4 a = *reinterpret_cast<const float4*>(wp + t);
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (jv) b = *reinterpret_cast<const float4*>(xp + t);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
  }
  part[wave][lane] = acc;
  __syncthreads();
  if (wave != 0 || !jv) return;
  const f32x4 s = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + 4 * kg + r;
    const float v = s[r] + bias[i];
    if (i < n0)
      out0[(size_t)j * n0 + i] = v;
    else if (i < n0 + n1)
      out1[(size_t)j * n1 + (i - n0)] = v;
  }
}

// Split-K form for very long K (KeypointRegressionHead: K = 1280*8*12 = 122880, keypoints.py:20): grid.z
// slices of K write fp32 partial tiles, fc_reduce_kernel sums them in slice order (deterministic).
__global__ __launch_bounds__(256) void fc_partial_kernel(const float* __restrict__ X, const float* __restrict__ W,
                                                         float* __restrict__ part, int B, int K, int Np, int kslice) {
  __shared__ f32x4 red[4][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t nJ = (uint32_t)(B + 15) / 16, nI = (uint32_t)Np / 16;
  uint32_t L = xcd_remap(blockIdx.x, gridDim.x);       // image groups of one (slice, row tile) on one XCD
  const int j0 = (int)(L % nJ) * 16;
  L /= nJ;
  const int i0 = (int)(L % nI) * 16, z = (int)(L / nI);
  const int r16 = lane & 15, kg = lane >> 4;
  const int j = j0 + r16;
  const bool jv = j < B;
  const float* wp = W + (size_t)(i0 + r16) * K + 4 * kg;
  const float* xp = X + (size_t)(jv ? j : 0) * K + 4 * kg;
  const int k0 = z * kslice, k1 = min(K, k0 + kslice);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int t = k0 + 16 * wave; t < k1; t += 64) {
    const float4 a = *reinterpret_cast<const float4*>(wp + t);
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (jv) b = *reinterpret_cast<const float4*>(xp + t);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
  }
  red[wave][lane] = acc;
  __syncthreads();
  if (wave != 0 || !jv) return;
  const f32x4 s = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
  float* o = part + ((size_t)z * B + j) * Np + i0 + 4 * kg;
  *reinterpret_cast<float4*>(o) = make_float4(s[0], s[1], s[2], s[3]);
}

__global__ void fc_reduce_kernel(const float* __restrict__ part, const float* __restrict__ bias,
                                 float* __restrict__ out, int n, int B, int Np, int splits) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * n) return;
  const int j = idx / n, i = idx - j * n;
  const float* p = part + (size_t)j * Np + i;
  const size_t zs = (size_t)B * Np;
  float v = bias[i];
  // 30 slices' loads in flight, then added in slice order (the sum order of one slice at a time: bit-identical);
  // one dependent load per slice made this 60-slice reduction latency-bound (15 us)
  constexpr int U = 30;
  int z = 0;
  for (; z + U <= splits; z += U) {
    float t[U];
#pragma unroll
    for (int u = 0; u < U; ++u) t[u] = p[(size_t)(z + u) * zs];
#pragma unroll
    for (int u = 0; u < U; ++u) v += t[u];
  }
  for (; z < splits; ++z) v += p[(size_t)z * zs];
  out[(size_t)j * n + i] = v;
}

// (workgroup reductions: spef_reduce.hpp)

// (the top eigenvector of the Markley matrix, sym4_top_eigvec: spef_eig.hpp)

// ------------------------------------------------------------------------------------------ decode ori
// One 256-thread workgroup per image; the image's logits stay in registers (PER per thread, n <= 256 PER) from one
// global read. Softmax in float32 as SPEUtils.last_activ; the ten fp64 moments of a = sum_i p_i q_i q_i^T are
// reduced through LDS (each of 160 threads sums 16 interleaved partials, each 16-lane row sums those by DPP: a fixed
// order).
// It also writes the image's whole status word (the decode's first kernel: no memset launch) and, in position
// regression mode, copies the 3 raw position outputs (no copy launch): pos_src == nullptr skips the copy.
// PDF = true (the video path, k_video.hip): `logits` already holds a PDF (the filtered one), so the softmax is
// skipped and p_i is the input itself; a row whose moments have no positive trace (all zero) is flagged like a NaN
// one (the reference's decode of the 0 / 0 row raises the same error). PDF = false is the still-frame decode.
template <int PER, bool PDF = false>
__global__ __launch_bounds__(256) void decode_ori_kernel(const float* __restrict__ logits, int n,
                                                         const double* __restrict__ qb, float* __restrict__ soft,
                                                         float* __restrict__ quat, int* __restrict__ status,
                                                         const float* __restrict__ pos_src, float* __restrict__ pos) {
  __shared__ float shf[2][4];
  __shared__ double shd[10][256];
  __shared__ double shp[10][16];
  const int tid = threadIdx.x, b = blockIdx.x;
  SPEF_TRACE(0);   // timeline probes (tools/kbench/head_bench.hip trace): nothing in the library build
  if (pos_src && tid < 3) pos[3 * b + tid] = pos_src[3 * b + tid];
  const float* x = logits + (size_t)b * n;
  float v[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + 256 * j;
    v[j] = i < n ? x[i] : (PDF ? 0.0f : -INFINITY);
  }
  // the bin quaternions are loaded with the logits (PER <= 8: 64 VGPRs), not after the softmax: in the network the
  // forward has evicted them, and that second dependent HBM round trip was 40 % of the kernel (head_bench trace)
  constexpr bool PF = PER <= 8;
  double4 qv[PF ? PER : 1];
  if constexpr (PF) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int i = tid + 256 * j;
      qv[j] = *reinterpret_cast<const double4*>(qb + 4 * (i < n ? i : 0));
    }
  }
  float s = 1.0f;
  if constexpr (!PDF) {
    float m = v[0];
#pragma unroll
    for (int j = 1; j < PER; ++j) m = fmaxf(m, v[j]);
    SPEF_TRACE(1);
    m = block_max256(m, shf[0]);
    SPEF_TRACE(2);
    s = 0.0f;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      v[j] = tid + 256 * j < n ? expf(v[j] - m) : 0.0f;
      s += v[j];
    }
    s = block_sum256(s, shf[1]);
    SPEF_TRACE(3);
  }
  double mom[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) mom[k] = 0.0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + 256 * j;
    if (i < n) {
      const float p = PDF ? v[j] : v[j] / s;
      if (!PDF && soft) soft[(size_t)b * n + i] = p;
      const double pd = (double)p;
      double4 q;
      if constexpr (PF) q = qv[j];
      else q = *reinterpret_cast<const double4*>(qb + 4 * i);
      mom[0] += (q.x * q.x) * pd; mom[1] += (q.x * q.y) * pd; mom[2] += (q.x * q.z) * pd; mom[3] += (q.x * q.w) * pd;
      mom[4] += (q.y * q.y) * pd; mom[5] += (q.y * q.z) * pd; mom[6] += (q.y * q.w) * pd;
      mom[7] += (q.z * q.z) * pd; mom[8] += (q.z * q.w) * pd; mom[9] += (q.w * q.w) * pd;
    }
  }
  SPEF_TRACE(4);
#pragma unroll
  for (int k = 0; k < 10; ++k) shd[k][tid] = mom[k];
  __syncthreads();
  SPEF_TRACE(5);
  if (tid < 160) {   // 16-lane row k sums moment k: 16 partials per lane, then the row by DPP
    const int k = tid >> 4, j = tid & 15;
    double a = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) a += shd[k][j + 16 * r];
    a = dpp_add_d<0xB1>(a);    // quad_perm [1,0,3,2]
    a = dpp_add_d<0x4E>(a);    // quad_perm [2,3,0,1]
    a = dpp_add_d<0x141>(a);   // row_half_mirror
    a = dpp_add_d<0x140>(a);   // row_mirror
    if (j == 0) shp[k][0] = a;
  }
  __syncthreads();
  SPEF_TRACE(6);
  if (tid != 0) return;
  double t[10];
  bool nan = false;
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    t[k] = shp[k][0];
    nan |= isnan(t[k]);
  }
  if constexpr (PDF) nan |= !((t[0] + t[4]) + (t[7] + t[9]) > 0.0);
  status[b] = nan ? 1 : 0;
  if (nan) {  // classification_utils.py:134-135
    for (int k = 0; k < 4; ++k) quat[4 * b + k] = NAN;
    return;
  }
  double q[4];
  SPEF_TRACE(7);
  sym4_top_eigvec(t, q);
  for (int k = 0; k < 4; ++k) quat[4 * b + k] = (float)q[k];
  SPEF_TRACE(8);
}

// ------------------------------------------------------------------------------------------ decode pos
// PDF = true (the video path): `logits` is the filtered PDF itself, no softmax.
template <bool PDF = false>
__global__ __launch_bounds__(256) void decode_pos_kernel(const float* __restrict__ logits, int n,
                                                         const double* __restrict__ grid, float* __restrict__ soft,
                                                         float* __restrict__ pos, int* __restrict__ status) {
  __shared__ float shf[2][4];
  __shared__ double shd[4][3];
  __shared__ float shp[4];
  const int b = blockIdx.x;
  const float* x = logits + (size_t)b * n;
  float m = 0.0f, s = 1.0f;
  if constexpr (!PDF) {
    m = -INFINITY;
    for (int i = threadIdx.x; i < n; i += 256) m = fmaxf(m, x[i]);
    m = block_max256(m, shf[0]);
    s = 0.0f;
    for (int i = threadIdx.x; i < n; i += 256) s += expf(x[i] - m);
    s = block_sum256(s, shf[1]);
  }
  double acc[3] = {0.0, 0.0, 0.0};
  float ps = 0.0f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float p = PDF ? x[i] : expf(x[i] - m) / s;
    if (!PDF && soft) soft[(size_t)b * n + i] = p;
    ps += p;
    const double pd = (double)p;
    acc[0] += grid[3 * i] * pd;
    acc[1] += grid[3 * i + 1] * pd;
    acc[2] += grid[3 * i + 2] * pd;
  }
  ps = warp_sum(ps);
  for (int k = 0; k < 3; ++k) acc[k] = warp_sum_d(acc[k]);
  if ((threadIdx.x & 63) == 0) {
    shp[threadIdx.x >> 6] = ps;
    for (int k = 0; k < 3; ++k) shd[threadIdx.x >> 6][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const float tot = (shp[0] + shp[1]) + (shp[2] + shp[3]);
  if (tot == 0.0f) status[b] |= 2;  // classification_utils.py:253-254
  for (int k = 0; k < 3; ++k) {
    const double v = ((shd[0][k] + shd[1][k]) + (shd[2][k] + shd[3][k])) / (double)tot;
    if (isnan(v)) status[b] |= 4;  // classification_utils.py:262-263
    pos[3 * b + k] = (float)v;
  }
}

__global__ void normalize_ori_kernel(const float* __restrict__ raw, int B, float* __restrict__ quat,
                                     int* __restrict__ status, const float* __restrict__ pos_src,
                                     float* __restrict__ pos) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  status[b] = 0;   // as decode_ori_kernel: the decode's first kernel owns the status word and the position copy
  if (pos_src)
    for (int k = 0; k < 3; ++k) pos[3 * b + k] = pos_src[3 * b + k];
  const float4 q = *reinterpret_cast<const float4*>(raw + 4 * b);
  const float n = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  *reinterpret_cast<float4*>(quat + 4 * b) = make_float4(q.x / n, q.y / n, q.z / n, q.w / n);
}

// ------------------------------------------------------------------------------------------ launchers
hipError_t launch_fc(const float* x, const float* w, const float* bias, float* out0, int n0, float* out1, int n1, int B,
                     int K, hipStream_t s) {
  if (K % 16) return hipErrorInvalidValue;
  const int Np = (n0 + n1 + 15) & ~15;
  const int64_t nwg = (int64_t)(Np / 16) * ((B + 15) / 16);
  if (nwg > 0x7fffffff) return hipErrorInvalidValue;
  fc_kernel<<<(uint32_t)nwg, 256, 0, s>>>(x, w, bias, out0, n0, out1, n1, B, K, Np);
  return hipGetLastError();
}

hipError_t launch_fc_splitk(const float* x, const float* w, const float* bias, float* out, int n, int B, int K,
                            int splits, float* part, hipStream_t s) {
  if (K % 16) return hipErrorInvalidValue;
  const int Np = (n + 15) & ~15;
  int kslice = (K + splits - 1) / splits;
  kslice = (kslice + 63) / 64 * 64;
  splits = (K + kslice - 1) / kslice;
  const int64_t nwg = (int64_t)(Np / 16) * ((B + 15) / 16) * splits;
  if (nwg > 0x7fffffff) return hipErrorInvalidValue;
  fc_partial_kernel<<<(uint32_t)nwg, 256, 0, s>>>(x, w, part, B, K, Np, kslice);
  fc_reduce_kernel<<<(B * n + 255) / 256, 256, 0, s>>>(part, bias, out, n, B, Np, splits);
  return hipGetLastError();
}

hipError_t launch_decode_ori(const float* logits, int B, int n_bins, const double* q_bins, float* soft, float* quat,
                             int* status, const float* pos_src, float* pos, hipStream_t s) {
  if (n_bins <= 256 * 8)
    decode_ori_kernel<8><<<B, 256, 0, s>>>(logits, n_bins, q_bins, soft, quat, status, pos_src, pos);
  else if (n_bins <= 256 * 32)
    decode_ori_kernel<32><<<B, 256, 0, s>>>(logits, n_bins, q_bins, soft, quat, status, pos_src, pos);
  else
    return hipErrorInvalidValue;   // more than 8192 orientation bins (20^3 = 8000 is the largest cubic grid)
  return hipGetLastError();
}

hipError_t launch_normalize_ori(const float* raw, int B, float* quat, int* status, const float* pos_src, float* pos,
                                hipStream_t s) {
  normalize_ori_kernel<<<(B + 255) / 256, 256, 0, s>>>(raw, B, quat, status, pos_src, pos);
  return hipGetLastError();
}

hipError_t launch_decode_pos(const float* logits, int B, int n_bins, const double* grid, float* soft, float* pos,
                             int* status, hipStream_t s) {
  decode_pos_kernel<false><<<B, 256, 0, s>>>(logits, n_bins, grid, soft, pos, status);
  return hipGetLastError();
}

hipError_t launch_decode_pdf(const float* ori_pdf, const float* pos_pdf, int B, int n_ori, const double* q_bins,
                             int n_pos, const double* grid, float* quat, float* pos, int* status, hipStream_t s) {
  if (n_ori <= 256 * 8)
    decode_ori_kernel<8, true><<<B, 256, 0, s>>>(ori_pdf, n_ori, q_bins, nullptr, quat, status, nullptr, nullptr);
  else if (n_ori <= 256 * 32)
    decode_ori_kernel<32, true><<<B, 256, 0, s>>>(ori_pdf, n_ori, q_bins, nullptr, quat, status, nullptr, nullptr);
  else
    return hipErrorInvalidValue;
  decode_pos_kernel<true><<<B, 256, 0, s>>>(pos_pdf, n_pos, grid, nullptr, pos, status);
  return hipGetLastError();
}

}  // namespace spef
