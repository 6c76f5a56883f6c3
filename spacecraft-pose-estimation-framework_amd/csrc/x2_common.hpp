// fp32-accurate fused schedule on the fp16 matrix cores (blob dtype 5, "fp16x2"): the parity variant for heads
// whose output error the fp16 schedule cannot bound -- sharp URSONet heads (tools/sharp_head_budget.py: fp16 storage
// gives 1.6e-2 max |d logit| at head_std 0.3, hi + lo everything 1.8e-5) and the unpooled keypoint head
// (head/keypoints.py:20-27).
//
// Every value that feeds a matrix product is carried as an unevaluated pair of fp16 numbers, v = hi + lo with
// hi = fp16(v), lo = fp16(v - hi) (22 significant bits; |v - hi - lo| <= 2^-22 |v|, or 3e-8 absolute where lo is
// subnormal). A product a * b is the three MFMAs a_hi b_hi + a_lo b_hi + a_hi b_lo on the fp16 MFMA
// (v_mfma_f32_16x16x32_f16: fp32 accumulation, 16 cycles), which is 5.3x the rate of the exact fp32 MFMA
// (v_mfma_f32_16x16x4_f32, 8 instructions of 32 cycles for the same 16x16x32 tile; cdna_hip_programming.md section 3).
// The dropped a_lo b_lo term is below 2^-22 relative.
//
//   x2_irb_kernel  one InvertedResidual (pytorch_layers.py:65-98) per kernel (high-resolution blocks 1-7): each wave
//                  loads the fp32 input pixels of its expand tiles once and keeps them split (hi / lo B fragments) in
//                  registers; per 32-channel hidden chunk the expand (3 MFMAs per K step) writes ReLU(x We^T + be) as
//                  fp32 into an LDS slab; the depthwise 3x3 runs in fp32 (v_fma_f32 chains, kx-outer / ky-inner, weights
//                  staged in LDS once) on the slab, its ReLU'd output is split into hi / lo project B fragments in
//                  registers; the project accumulates over chunks in fp32 MFMA accumulators; + residual (fp32, read
//                  back from L2) -> fp32 block output. Block 1 (t = 1) stages its input straight into the slab.
//                  (k_x2_irb.hip)
//   x2_irw_kernel  the same block, role-split into expand and depthwise/project waves with LDS-staged weights (blocks
//                  8-17, k_x2_irw.hip; x2_irw_st_kernel there: the same with LDS-DMA staging kept in flight, the
//                  persistent-tile blocks 8-10 and 14); x2_irp_kernel, its three-stage form (k_x2_irp.hip).
//   x2_front_kernel  uint8 frames -> stem + block 1 (k_x2_front.hip).
//   x2_pw_kernel   1x1 conv on fp32 activations (the last ConvBnAct 320 -> 1280, mobilenet_v2.py:264): B fragments
//                  split on load, ReLU, fp32 output (the keypoint head's flatten input or the URSONet mean's)
//                  (k_x2_pw.hip).
// Which kernel a block runs on: x2_plan.hpp (the tile tables and the plan), launched by x2_dispatch.cpp.
//
// Block I/O is fp32 NHWC; weights come from the blob split by the packer (spef_amd/blob.py, dtype fp16x2).
//
// This header: the device helpers and the build switches that more than one of those files uses.
#pragma once
#include "spef_common.hpp"

namespace spef {

// hi / lo split of 8 fp32 values (the residual v - hi is exact in fp32; fmaf((float)h, -1, v) is one v_fma_mix)
__device__ __forceinline__ void split8(const float v[8], f16x8& hi, f16x8& lo) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const _Float16 h = (_Float16)v[e];
    hi[e] = h;
    lo[e] = (_Float16)fmaf((float)h, -1.0f, v[e]);
  }
}
__device__ __forceinline__ void split4(float4 v, uint2& hi, uint2& lo) {
  const float a[4] = {v.x, v.y, v.z, v.w};
  _Float16 h[4], l[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    h[e] = (_Float16)a[e];
    l[e] = (_Float16)fmaf((float)h[e], -1.0f, a[e]);
  }
  hi = make_uint2(pack_h2(h[0], h[1]), pack_h2(h[2], h[3]));
  lo = make_uint2(pack_h2(l[0], l[1]), pack_h2(l[2], l[3]));
}
// lo halves of a pair: fp16(a - hi.x), fp16(b - hi.y), each ONE v_fma_mix{lo,hi}_f16 (the difference is formed
// exactly and rounded once, the same value as split8's fp32 residual + convert, which takes 1.5 ops per value)
__device__ __forceinline__ uint32_t lo_pair(uint32_t hi2, float a, float b) {
  uint32_t r;
  asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixhi_f16 %0, %1, -1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
      : "=&v"(r) : "v"(hi2), "v"(a), "v"(b));
  return r;
}
// ReLU + hi / lo split of 8 fp32 values: 8 v_max + 4 v_cvt_pk + 8 v_fma_mix (bit-identical to max + split8)
__device__ __forceinline__ void relu_split8(const f32x2 v[4], f16x8& hi, f16x8& lo) {
  uint32_t h[4], l[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float a = fmaxf(v[i].x, 0.f), b = fmaxf(v[i].y, 0.f);
    h[i] = pack_h2((_Float16)a, (_Float16)b);
    l[i] = lo_pair(h[i], a, b);
  }
  hi = __builtin_bit_cast(f16x8, make_uint4(h[0], h[1], h[2], h[3]));
  lo = __builtin_bit_cast(f16x8, make_uint4(l[0], l[1], l[2], l[3]));
}
// acc += (a_hi + a_lo)(b_hi + b_lo) without the lo*lo term
__device__ __forceinline__ f32x4 mfma_x2(f16x8 ah, f16x8 al, f16x8 bh, f16x8 bl, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, acc, 0, 0, 0);
}
// acc += (a_hi + a_lo) b for an operand b that is exact in fp16 (fp16-stored activations: the fp16mx schedule)
__device__ __forceinline__ f32x4 mfma_x2w(f16x8 ah, f16x8 al, f16x8 b, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, b, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(al, b, acc, 0, 0, 0);
}
// depthwise tap on 8 channels as 4 v_pk_fma_f32 (each channel's fma in the same order as scalar fmaf chains)
__device__ __forceinline__ void dw_tap8(f32x2 a[4], float4 x0, float4 x1, const f32x2 w[4]) {
  a[0] = __builtin_elementwise_fma(f32x2{x0.x, x0.y}, w[0], a[0]);
  a[1] = __builtin_elementwise_fma(f32x2{x0.z, x0.w}, w[1], a[1]);
  a[2] = __builtin_elementwise_fma(f32x2{x1.x, x1.y}, w[2], a[2]);
  a[3] = __builtin_elementwise_fma(f32x2{x1.z, x1.w}, w[3], a[3]);
}
// block I/O element types (IO template bits): fp32, or fp16 where the fp16mx schedule stores a block output in fp16
constexpr int IO_IN16 = 1, IO_OUT16 = 2;
__device__ __forceinline__ float4 ld_act4(const void* p, size_t i, bool f16) {   // 4 channels at element i
  if (f16) {
    const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const _Float16*>(p) + i);
    return make_float4(h_lo(u.x), h_hi(u.x), h_lo(u.y), h_hi(u.y));
  }
  return *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p) + i);
}
__device__ __forceinline__ void st_act4(void* p, size_t i, f32x4 v, bool f16) {
  if (f16)
    *reinterpret_cast<uint2*>(reinterpret_cast<_Float16*>(p) + i) =
        make_uint2(pack_h2((_Float16)v[0], (_Float16)v[1]), pack_h2((_Float16)v[2], (_Float16)v[3]));
  else
    *reinterpret_cast<float4*>(reinterpret_cast<float*>(p) + i) = make_float4(v[0], v[1], v[2], v[3]);
}

// Hidden-chunk slab in LDS (fp32): two planes per 32-channel chunk, plane h holding channels 8k + 4h .. 8k + 4h + 3
// (k = 0..3) of every tile pixel as one 16-B granule each. A depthwise lane (pixel r16, channels 8kg .. 8kg + 7)
// reads granule kg of its pixel row in plane 0 and in plane 1; an expand lane writes the float4 of channels
// 16h + 4kg .. +3 (plane kg & 1, granule 2h + kg / 2). Row strides from the ds_read_b128 lane groups of
// MI355X_MICROARCH.md (LDS): 24 floats make the 16 consecutive rows of a 16-wide stride-1 pixel tile conflict-free
// (2-way on 8-wide tiles), 20 floats the stride-2 rows; the plane-1 base is offset to keep the expand's mixed-plane
// stores conflict-free.
template <int S, int PINP>
struct X2Slab {
  static constexpr int SSP = S == 2 ? 20 : 24;                   // floats per pixel row of a plane
  static constexpr int TGT = S == 2 ? 0 : 1;                     // plane-1 base, granules mod 16
  static constexpr int PLANE = PINP * SSP + ((TGT - PINP * SSP / 4) % 16 + 16) % 16 * 4;
  static constexpr int FLOATS = 2 * PLANE;
  static __device__ __forceinline__ int at(int p, int c4) {      // float offset of channels 4 c4 .. 4 c4 + 3 of pixel p
    return (c4 & 1) * PLANE + p * SSP + 4 * (c4 >> 1);
  }
};

#ifndef SPEF_X2_RES_AHEAD   // persistent tiles: chunks before a tile's end at which its residual is fetched (4: no gain)
#define SPEF_X2_RES_AHEAD 2
#endif
#ifndef SPEF_X2_STAMP   // timing builds only (outputs overwritten): s_memtime stamps per chunk of one workgroup
#define SPEF_X2_STAMP 0
#endif

// Workgroup barrier for LDS hand-offs only: this wave's LDS stores complete, then s_barrier -- without the vmcnt(0)
// that __syncthreads() gets when an LDS-DMA is in flight, so global loads and DMA pieces that are consumed later stay
// in flight across it (the callers wait with counted vmcnt for the pieces other waves read next).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

}  // namespace spef
