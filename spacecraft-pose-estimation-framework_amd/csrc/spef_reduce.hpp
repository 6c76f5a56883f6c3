// Workgroup reductions shared by the head / decode kernels (k_head.hip) and the video filter (k_video.hip).
#pragma once

#include "spef_common.hpp"

namespace spef {

// Workgroup (4 waves) max / sum of one float per thread: within a 16-lane row by DPP (quad swaps, half-row and row
// mirrors: every lane ends with its row's value, no LDS round trip), the 4 rows by readlane, the 4 waves through
// LDS with one barrier. sh[4] must not be reused by the caller. A fixed combination order: deterministic.
template <bool MAX>
__device__ __forceinline__ float dpp_op(float a, float b) { return MAX ? fmaxf(a, b) : a + b; }
template <bool MAX, int CTRL>
__device__ __forceinline__ float dpp_step(float v) {
  const float o = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
  return dpp_op<MAX>(v, o);
}
template <bool MAX>
__device__ __forceinline__ float block_reduce256(float v, float* sh) {
  v = dpp_step<MAX, 0xB1>(v);    // quad_perm [1,0,3,2]
  v = dpp_step<MAX, 0x4E>(v);    // quad_perm [2,3,0,1]
  v = dpp_step<MAX, 0x141>(v);   // row_half_mirror
  v = dpp_step<MAX, 0x140>(v);   // row_mirror
  const int u = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(u, 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(u, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(u, 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(u, 48));
  const float w = dpp_op<MAX>(dpp_op<MAX>(r0, r1), dpp_op<MAX>(r2, r3));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = w;
  __syncthreads();
  return dpp_op<MAX>(dpp_op<MAX>(sh[0], sh[1]), dpp_op<MAX>(sh[2], sh[3]));
}
template <int CTRL>
__device__ __forceinline__ double dpp_add_d(double v) {   // v + (v of the DPP source lane), fp64 as two dword moves
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)u, CTRL, 0xf, 0xf, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)(u >> 32), CTRL, 0xf, 0xf, false);
  return v + __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ float block_max256(float v, float* sh) { return block_reduce256<true>(v, sh); }
__device__ __forceinline__ float block_sum256(float v, float* sh) { return block_reduce256<false>(v, sh); }

// fp64 sums in the same fixed order: the 16-lane rows by DPP, the 4 rows by readlane (every lane of the wave ends
// with the wave's sum), the 4 waves through LDS with one barrier (sh[4] as above).
__device__ __forceinline__ double readlane_d(double v, int lane) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), lane);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double wave_sum64_d(double v) {
  v = dpp_add_d<0xB1>(v);
  v = dpp_add_d<0x4E>(v);
  v = dpp_add_d<0x141>(v);
  v = dpp_add_d<0x140>(v);
  return (readlane_d(v, 0) + readlane_d(v, 16)) + (readlane_d(v, 32) + readlane_d(v, 48));
}
__device__ __forceinline__ double block_sum256_d(double v, double* sh) {
  const double w = wave_sum64_d(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = w;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// Sum accumulator k of every thread of a 256-thread workgroup (sh[k][tid]) into out[k], k < nacc: 16-lane row r of the
// workgroup takes accumulators r, r + 16, ...; each lane adds 16 interleaved partials, the row adds its lanes by DPP.
// Ends on a barrier. (The decode covariance, k_cov.hip, and the multi-hypothesis decode, k_modes.hip.)
__device__ __forceinline__ void cov_reduce(const double (*sh)[256], double* out, int nacc) {
  const int tid = threadIdx.x, j = tid & 15;
  for (int k = tid >> 4; k < nacc; k += 16) {
    double a = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) a += sh[k][j + 16 * r];
    a = dpp_add_d<0xB1>(a);    // quad_perm [1,0,3,2]
    a = dpp_add_d<0x4E>(a);    // quad_perm [2,3,0,1]
    a = dpp_add_d<0x141>(a);   // row_half_mirror
    a = dpp_add_d<0x140>(a);   // row_mirror
    if (j == 0) out[k] = a;
  }
  __syncthreads();
}

}  // namespace spef
