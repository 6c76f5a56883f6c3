// fp16x2 role-split kernels (plan kinds 1-3: the low-resolution blocks 8-17) and the hidden-split join; the arithmetic
// and the kernel overview are in x2_common.hpp. Two kernels share the roles, the pipeline and the arithmetic:
//   x2_irw_kernel     kinds 1 and 2 (the hidden-split rows, the PAIR form), and kind 3 under SPEF_OPT_X2_STAGE = 0
//   x2_irw_st_kernel  kind 3 (persistent tiles: blocks 8-10 and 14 at 512^2), the default: static staging, further down
#include "spef_kernels.hpp"
#include "x2_common.hpp"

namespace spef {

// ------------------------------------------------------------------------------------------ role-split form
// The low-resolution blocks (8-17: 32x32 and 16x16 maps at 512^2, 256-1024 tiles for 256 CUs, 12-30 hidden chunks)
// are bound by how fast a workgroup streams the chunk weights, not by arithmetic: every chunk needs its expand and
// project weights (hi + lo, 20 KB each for 160 -> 960 -> 160) from L2 at ~29 B/clk per CU, and a lone workgroup per
// CU exposes every round trip. Here 8 waves take fixed roles in a two-stage pipeline with ONE barrier per chunk:
//
//   expand waves [0, 4): expand chunk c+1 into slab (c+1) & 1; their input-tile B fragments (hi + lo) are loaded and
//                        split once and stay in registers for every chunk (no input tile in LDS)
//   depthwise waves [4, 8): depthwise of chunk c from slab c & 1 + project accumulation (weights from the LDS stage)
//
// Stage buffers (double-buffered, filled one iteration before use): expand weights + expand bias of chunk k in
// iteration k - 2, depthwise weights + bias and project weights of chunk k in iteration k - 1. Same arithmetic and
// rounding as x2_irb_kernel (bit-identical results). How a stage is filled is what the two kernels differ in:
//   x2_irw_kernel, register staging (GL off): the expand waves load every piece of all three stages one iteration
//     ahead and ds_write them at the start of the next -- 828 of the expand role's 2,720 cycles per chunk on blocks 8-10;
//   x2_irw_kernel, GL: LDS-DMA into the one dynamic smem[] array with __syncthreads() between chunks. The compiler
//     cannot tell the stage being filled from the stage being read, so both roles wait vmcnt(0) before their chunk's
//     first stage reads: each chunk's weights are fetched synchronously (block 14: 3,872 cycles per chunk);
//   x2_irw_st_kernel: LDS-DMA into separately named static buffers, kept in flight across the chunk barrier (block 14:
//     2,992 cycles per chunk; blocks 8-10: expand role 2,720 -> 1,850) -- see its comment.
#ifndef SPEF_X2_GLDS   // stage the role-split kernels' chunk weights by LDS-DMA (global_load_lds) instead of registers
#define SPEF_X2_GLDS 1
#endif
#ifndef SPEF_X2_GLDS_S2   // ... on block 14 (stride 2) too
#define SPEF_X2_GLDS_S2 1
#endif
#ifndef SPEF_X2_DPE_WIDE   // static staging, cout > 64 (block 14): depthwise / project pieces issued by the expand waves
#define SPEF_X2_DPE_WIDE 0
#endif
template <int CIN, int HID, int COUT, int S, int TH, int TW, int WCO, bool PST, int P = 1>
struct X2wGeom {
  static constexpr int NE = 4, ND = 4, NW = NE + ND;
  static constexpr int IH = (TH - 1) * S + 3, IW = (TW - 1) * S + 3;
  static constexpr int PIN = IH * IW, PIN16 = (PIN + 15) / 16, PINP = PIN16 * 16;
  static constexpr int CINP = (CIN + 31) / 32 * 32, KS = CINP / 32;
  static constexpr int WES = CINP + 16;                 // staged expand row (halves): 2 mod 4 granules
  static constexpr int WPS = 48;                        // staged project row (halves, 32 used)
  using SL = X2Slab<S, PINP>;
  static constexpr int NCH = (HID + 31) / 32, HIDP = NCH * 32;
  static constexpr int NCL = NCH / P;                   // chunks of this workgroup's hidden part
  static constexpr int NCT = (COUT + 15) / 16, NPC = NCT * 16;
  static constexpr int POUT16 = TH * TW / 16;
  static constexpr int WP = ND / WCO, QPW = POUT16 / WP, NCTW = NCT / WCO;
  static constexpr int EPT = (PIN16 + NE - 1) / NE;     // expand pixel tiles per expand wave
  // LDS: slabs | expand stage [2] | depthwise stage [2] | project stage [2]
  static constexpr int SLAB_B = SL::FLOATS * 4;
  static constexpr int SE_B = 2 * 32 * WES * 2 + 32 * 4;   // hi / lo weight planes + expand bias
  static constexpr int SD_B = (9 * 32 + 32) * 4;        // depthwise weights [9][32] + depthwise bias
  static constexpr int SP_B = PST ? 2 * NPC * WPS * 2 : 0;
  // LDS-DMA staging (GL): every stage region a whole number of 1-KiB wave-instruction pieces (a piece writes 64 x 16 B
  // lane-linearly); per buffer the depthwise and project stages are one contiguous region. Interleaved A/B at B = 64:
  // blocks 14 and 15-16 -2 / -5 us per step, block 17 +3, blocks 8-13 no gain (same box, interleaved), so the
  // cout = 160 blocks only. (That was this kernel's synchronous form, each chunk's pieces drained before its reads;
  // kept in flight -- x2_irw_st_kernel -- LDS-DMA takes 13 us per step off blocks 8-10 and 9 off block 14.)
  static constexpr bool GL = SPEF_X2_GLDS && COUT == 160 && (S == 1 || SPEF_X2_GLDS_S2);
  static constexpr int SE_BQ = (SE_B + 1023) / 1024 * 1024, SD_BQ = (SD_B + 1023) / 1024 * 1024;
  static constexpr int SP_BQ = (SP_B + 1023) / 1024 * 1024, DP_BQ = SD_BQ + SP_BQ;
  static constexpr int NIE = SE_BQ / 1024, NID = DP_BQ / 1024;                  // pieces per chunk stage
  static constexpr int IEW = (NIE + NE - 1) / NE, IDW = (NID + ND - 1) / ND;    // pieces per wave
  static constexpr int SE_STR = GL ? SE_BQ : SE_B, SD_STR = GL ? DP_BQ : SD_B, SP_STR = GL ? DP_BQ : SP_B;
  static constexpr int OFF_SE = 2 * SLAB_B;
  static constexpr int OFF_SD = GL ? OFF_SE + 2 * SE_BQ : OFF_SE + 2 * SE_B;
  static constexpr int OFF_SP = GL ? OFF_SD + SD_BQ : OFF_SD + 2 * SD_B;
  static constexpr int OFF_TR = GL ? OFF_SD + 2 * DP_BQ : OFF_SP + 2 * SP_B;   // dummy rows: invalid pixels' stores
  static constexpr int OFF_ST = OFF_TR + 16 * 24 * 4;     // SPEF_X2_STAMP: per-chunk clock stamps
  static constexpr int LDS_BYTES = OFF_ST + (SPEF_X2_STAMP ? 8 * 4 * 64 : 0);
  // 16-B stage pieces per chunk
  static constexpr int NPE = 2 * 32 * (CINP / 8) + 8, NPD = 9 * 8 + 8, NPP = PST ? 2 * NPC * 4 : 0;
  static constexpr int NPIECE = (NPE + NPD + NPP + NE * 64 - 1) / (NE * 64);
  static_assert(CIN % 8 == 0 && COUT % 4 == 0 && HID % 8 == 0, "channel counts");
  static_assert(TH * TW % 16 == 0 && POUT16 % WP == 0 && ND % WCO == 0 && NCT % WCO == 0, "tile split");
  static_assert(EPT <= 32 && NCH % P == 0 && NCL >= 2, "validity mask / hidden parts / pipeline depth");
  static_assert(SE_B % 16 == 0 && SD_B % 16 == 0 && SP_B % 16 == 0 && SLAB_B % 16 == 0, "16-B aligned stages");
  static_assert(LDS_BYTES <= 163840, "LDS budget");
  // Static staging (x2_irw_st_kernel, the persistent-tile rows): slab + dummy rows in floats, and how many of a chunk's
  // NID depthwise / project pieces the expand waves issue besides their own NIE (the rest: the depthwise waves).
  // Blocks 8-10 (cout 64): all 14. Their depthwise role is the longer one once the stage stores are gone (timing build,
  // cycles per chunk: expand 2,720 -> 1,850 with 7 pieces per wave costing 472 to issue, depthwise 2,494 -> 2,832) and runs
  // at the 256-register limit: with piece sources of its own it spilled. Block 14: none -- its depthwise role is the longer
  // one too (2,792 against 2,038), but with 16 / 32 of its 32 pieces on the expand waves it measured 53.3-53.5 -> 53.7-54.0 /
  // 55.1-55.5 us per step (tools/trim_ab.py, one process each).
  static constexpr int SLF = SL::FLOATS + 16 * 24;
  static constexpr int DPE = COUT == 64 ? NID : SPEF_X2_DPE_WIDE < NID ? SPEF_X2_DPE_WIDE : NID;
  static constexpr int ST_LDS = 2 * SLF * 4 + 2 * SE_BQ + 2 * DP_BQ + (SPEF_X2_STAMP ? 8 * 4 * 64 : 0);
};

// The helpers of x2_irw_st_kernel (below). x2w_expand and x2w_dwproj are x2_irw_kernel's expand and depthwise / project
// bodies for the rows with a project stage and persistent tiles, with the buffers as arguments; x2_irw_kernel keeps its
// own text so that SPEF_OPT_X2_STAGE = 0 runs the machine code it ran before.
// LDS-DMA source, at hidden chunk 0, of the 16-B slot at byte `off` of a chunk stage region (estage: weights hi / lo +
// bias of the expand; else depthwise weights + bias | project weights hi / lo), and the region's byte stride per chunk
// at `off`. Pad slots read a valid address of the same tensor.
template <class G>
__device__ __forceinline__ const char* x2w_stage_src(bool estage, int off, const _Float16* We, const float* be,
                                                     const float* Wd, const float* bd, const _Float16* Wp) {
  if (estage) {
    constexpr int EW_B = 2 * 32 * G::WES * 2, ROW_B = G::WES * 2;
    if (off < EW_B) {
      const int pl = off / (32 * ROW_B), rem = off - pl * (32 * ROW_B), rr = rem / ROW_B;
      const int col = (rem - rr * ROW_B) / 16;
      return reinterpret_cast<const char*>(We + (size_t)pl * G::HIDP * G::CINP + (size_t)rr * G::CINP +
                                           (col < G::CINP / 8 ? 8 * col : 0));
    }
    const int g = (off - EW_B) / 16;
    return reinterpret_cast<const char*>(be + (g < 8 ? 4 * g : 0));
  }
  if (off < 1152) return reinterpret_cast<const char*>(Wd + (size_t)(off / 128) * G::HIDP + 4 * ((off % 128) / 16));
  if (off < G::SD_BQ) {
    const int g = (off - 1152) / 16;
    return reinterpret_cast<const char*>(bd + (g < 8 ? 4 * g : 0));
  }
  const int o2 = off - G::SD_BQ;
  constexpr int ROW_B = G::WPS * 2;
  const int pl = o2 / (G::NPC * ROW_B), rem = o2 - pl * (G::NPC * ROW_B), rr = rem / ROW_B;
  const int q = (rem - rr * ROW_B) / 16;
  const bool ok = o2 < G::SP_B;
  return reinterpret_cast<const char*>(Wp + (ok ? (size_t)pl * G::NPC * G::HIDP + (size_t)rr * G::HIDP : 0) +
                                       (ok && q < 4 ? 8 * q : 0));
}
template <class G>
__device__ __forceinline__ int x2w_stage_stride(bool estage, int off) {
  return estage ? (off < 2 * 32 * G::WES * 2 ? 32 * G::CINP * 2 : 128) : off < G::SD_BQ ? 128 : 64;
}

// Expand of one hidden chunk by expand wave e: weights + bias from stage S0, ReLU'd fp32 results into slab Sl at soff
// (persistent tiles: zeros for the pixels outside the map; the dummy rows lie behind the slab).
template <class G>
__device__ __forceinline__ void x2w_expand(const char* S0, float* Sl, const f16x8 (&bxh)[G::EPT][G::KS],
                                           const f16x8 (&bxl)[G::EPT][G::KS], uint32_t pvmask,
                                           const int (&soff)[G::EPT], int r16, int kg) {
  const float* eb = reinterpret_cast<const float*>(S0 + 2 * 32 * G::WES * 2);
  f32x4 acc[G::EPT][2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float4 bb = *reinterpret_cast<const float4*>(eb + 16 * h + 4 * kg);
#pragma unroll
    for (int j = 0; j < G::EPT; ++j) acc[j][h] = f32x4{bb.x, bb.y, bb.z, bb.w};
  }
  const _Float16* Ws = reinterpret_cast<const _Float16*>(S0);
#pragma unroll
  for (int ks = 0; ks < G::KS; ++ks) {
    f16x8 ah[2], al[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      ah[h] = *reinterpret_cast<const f16x8*>(Ws + (16 * h + r16) * G::WES + 32 * ks + 8 * kg);
      al[h] = *reinterpret_cast<const f16x8*>(Ws + (32 + 16 * h + r16) * G::WES + 32 * ks + 8 * kg);
    }
#pragma unroll
    for (int j = 0; j < G::EPT; ++j) {
#pragma unroll
      for (int h = 0; h < 2; ++h) acc[j][h] = mfma_x2(ah[h], al[h], bxh[j][ks], bxl[j][ks], acc[j][h]);
    }
  }
#pragma unroll
  for (int j = 0; j < G::EPT; ++j) {
    const bool pv = (pvmask >> j) & 1u;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float4 v = make_float4(fmaxf(acc[j][h][0], 0.f), fmaxf(acc[j][h][1], 0.f), fmaxf(acc[j][h][2], 0.f),
                             fmaxf(acc[j][h][3], 0.f));
      if (!pv) v = make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(Sl + soff[j] + 8 * h) = v;
    }
  }
}

// P > 1 (hidden split): the P workgroups of a tile each run NCH / P consecutive hidden chunks and store their
// project partial sums (no bias, no residual) to Y + part * pstride; x2_split_reduce_kernel adds the P parts in order,
// the bias and the residual. Small maps get P times the workgroups while every workgroup streams only 1 / P of the
// block's weights.
// PT (persistent tiles): a workgroup runs tiles L, L + nwg, ... < ntile as ONE chunk stream (global chunk g = tile
// t * NCL + chunk c): the expand waves fetch the next tile's input two chunks ahead and expand its chunk 0 while the
// depthwise waves finish the current tile (residual fetched two chunks ahead, epilogue stores issued, accumulators
// reset), so a second tile per CU costs no prologue, epilogue or dispatch gap. Invalid input pixels are stored as
// zeros by every expand (a pixel valid in one tile may be padding in the next). NCL even: the stage / slab parity of
// global chunk g is that of its chunk c.
// Interleaved A/B at B = 64 (bit-identical): the occupancy target alone blocks 15-16 140 -> 139 us per step; with
// column batches one column ahead 140 -> 133, block 14 69 -> 66, blocks 8-13 unchanged (their expand role bounds the
// chunk period); 53.2k -> 53.5k img/s.
#ifndef SPEF_X2_DWB   // role-split depthwise: 0 = tap by tap, 1 = column batches, 2 = column batches one column ahead
#define SPEF_X2_DWB 2
#endif
#ifndef SPEF_X2_ROWS   // column batches share input rows between a wave's vertically adjacent pixel tiles
#define SPEF_X2_ROWS 1
#endif
// DWB 2 on two-pixel-tile waves up to this block input width. Without ROWS blocks 12-13 spilled at 96 and blocks 8-10
// measured 143.6 -> 145.4 us per step at 64; with ROWS (4 row reads per column instead of 6, interleaved A/B,
// bit-identical): blocks 12-13 161.6 -> 149.8, 8-10 141.7 -> 137.8, 11 53.0 -> 50.7 us per step.
#ifndef SPEF_X2_DWB2_CIN
#define SPEF_X2_DWB2_CIN 96
#endif
// Depthwise of one hidden chunk for this wave's QPW output pixel tiles (slab Sl, weights + bias D), ReLU, hi / lo split,
// then its project accumulation onto the wave's NCTW output-channel tiles, weights from the LDS stage Ps. mid(): called
// between the two (the timing builds' stamp).
template <class G, int CIN, int S, int TW, class Mid>
__device__ __forceinline__ void x2w_dwproj(const float* Sl, const float* D, const _Float16* Ps,
                                           const int (&pbase)[G::QPW], f32x4 (&acc)[G::QPW][G::NCTW], int wc, int r16,
                                           int kg, Mid mid) {
  using SL = typename G::SL;
  f32x2 a[G::QPW][4];
  {
    const float4 d0 = *reinterpret_cast<const float4*>(D + 288 + 8 * kg);
    const float4 d1 = *reinterpret_cast<const float4*>(D + 288 + 8 * kg + 4);
#pragma unroll
    for (int q = 0; q < G::QPW; ++q) {
      a[q][0] = f32x2{d0.x, d0.y}; a[q][1] = f32x2{d0.z, d0.w};
      a[q][2] = f32x2{d1.x, d1.y}; a[q][3] = f32x2{d1.z, d1.w};
    }
  }
  constexpr int DWB = (SPEF_X2_DWB == 2 && G::QPW > 1 && CIN > SPEF_X2_DWB2_CIN) ? 1 : SPEF_X2_DWB;
  if constexpr (DWB > 0) {
    // column batches: the 3 taps' weights and slab rows of column kx issued together (sched_barrier keeps them
    // ahead of the FMAs), DWB 2: column kx + 1's batch issued before column kx's FMAs. Same FMA order.
    // ROWS: a wave's pixel tiles are consecutive output rows (16-wide tiles, stride 1), so tap (ky, q) reads input
    // row q + ky of the column: QPW + 2 row reads per column instead of 3 QPW
    constexpr bool ROWS = SPEF_X2_ROWS && S == 1 && TW == 16 && G::QPW > 1;
    constexpr int NR = ROWS ? G::QPW + 2 : 3 * G::QPW;
    float4 wv[DWB][3][2], sr[DWB][NR][2];
    auto col = [&](int kx, int bf) {
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const float* wt = D + (ky * 3 + kx) * 32 + 8 * kg;
        wv[bf][ky][0] = *reinterpret_cast<const float4*>(wt);
        wv[bf][ky][1] = *reinterpret_cast<const float4*>(wt + 4);
      }
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int p = ROWS ? pbase[0] + r * G::IW + kx : pbase[r % G::QPW] + (r / G::QPW) * G::IW + kx;
        sr[bf][r][0] = *reinterpret_cast<const float4*>(Sl + SL::at(p, 2 * kg));
        sr[bf][r][1] = *reinterpret_cast<const float4*>(Sl + SL::at(p, 2 * kg + 1));
      }
    };
    col(0, 0);
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int bf = DWB == 2 ? (kx & 1) : 0;
      if (DWB == 2 && kx < 2) col(kx + 1, bf ^ 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const float4 w0 = wv[bf][ky][0], w1 = wv[bf][ky][1];
        const f32x2 w4[4] = {f32x2{w0.x, w0.y}, f32x2{w0.z, w0.w}, f32x2{w1.x, w1.y}, f32x2{w1.z, w1.w}};
#pragma unroll
        for (int q = 0; q < G::QPW; ++q) {
          const int r = ROWS ? q + ky : ky * G::QPW + q;
          dw_tap8(a[q], sr[bf][r][0], sr[bf][r][1], w4);
        }
      }
      if (DWB == 1 && kx < 2) {
        __builtin_amdgcn_sched_barrier(0);
        col(kx + 1, 0);
      }
    }
  } else {
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const float* wt = D + (ky * 3 + kx) * 32 + 8 * kg;
        const float4 w0 = *reinterpret_cast<const float4*>(wt), w1 = *reinterpret_cast<const float4*>(wt + 4);
        const f32x2 w4[4] = {f32x2{w0.x, w0.y}, f32x2{w0.z, w0.w}, f32x2{w1.x, w1.y}, f32x2{w1.z, w1.w}};
#pragma unroll
        for (int q = 0; q < G::QPW; ++q) {
          const int p = pbase[q] + ky * G::IW + kx;
          dw_tap8(a[q], *reinterpret_cast<const float4*>(Sl + SL::at(p, 2 * kg)),
                  *reinterpret_cast<const float4*>(Sl + SL::at(p, 2 * kg + 1)), w4);
        }
      }
  }
  f16x8 bh[G::QPW], bl[G::QPW];
#pragma unroll
  for (int q = 0; q < G::QPW; ++q) relu_split8(a[q], bh[q], bl[q]);
  mid();
#pragma unroll
  for (int t = 0; t < G::NCTW; ++t) {
    const int row = (wc * G::NCTW + t) * 16 + r16;
    const f16x8 ph = *reinterpret_cast<const f16x8*>(Ps + row * G::WPS + 8 * kg);
    const f16x8 pl = *reinterpret_cast<const f16x8*>(Ps + (G::NPC + row) * G::WPS + 8 * kg);
#pragma unroll
    for (int q = 0; q < G::QPW; ++q) acc[q][t] = mfma_x2(ph, pl, bh[q], bl[q], acc[q][t]);
  }
}

// occupancy target: one 8-wave workgroup per CU = 2 waves per SIMD (the VGPR budget is held to it)
// Roles by SIMD pair (PAIR, block 17: project fragments from L2, two cout groups): a workgroup's waves go to SIMDs in the
// cyclic order 0 -> 2 -> 1 -> 3 from a varying start (MI355X_MICROARCH.md, LDS), so waves {0, 1, 4, 5} (expand) share
// two SIMDs and {2, 3, 6, 7} (depthwise / project) the other two, and the two roles' MFMAs no longer share a SIMD's
// matrix pipe. Interleaved A/B at B = 64 (bit-identical): block 17 109.5 -> 102.6 us per step; blocks 8-16 slower
// (8-10 131.8 -> 146.5, 12-13 149.7 -> 168.2, 15-16 132.8 -> 136.0), so they keep waves 0-3 expand, 4-7 depthwise.
template <int CIN, int HID, int COUT, int S, int TH, int TW, bool RES, int WCO, bool PST, int P = 1, bool PT = false>
__global__ __launch_bounds__(8 * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void x2_irw_kernel(
    const float* __restrict__ X, const _Float16* __restrict__ We, const float* __restrict__ be,
    const float* __restrict__ Wd, const float* __restrict__ bd, const _Float16* __restrict__ Wp,
    const float* __restrict__ bp, float* __restrict__ Y, int H, int W, int OH, int OW, int tiles_x, int tiles_y,
    uint32_t nwg, size_t pstride, uint32_t ntile) {
  using G = X2wGeom<CIN, HID, COUT, S, TH, TW, WCO, PST, P>;
  using SL = typename G::SL;
  static_assert(!PT || (P == 1 && G::NCL % 2 == 0), "persistent tiles: one hidden part, even chunk count");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r16 = lane & 15, kg = lane >> 4;
  uint32_t L = xcd_remap(blockIdx.x, nwg);
  const bool stamp_wg = SPEF_X2_STAMP && L == 0;   // the workgroup of tile 0 (its output holds the stamps)
  auto stamp = [&](int c, int slot) {              // lane 0 of waves 0 / 4: shader clock into LDS slot (c, slot)
    if constexpr (SPEF_X2_STAMP) {
      if (stamp_wg && lane == 0 && c < 64)
        reinterpret_cast<uint32_t*>(smem + G::OFF_ST)[c * 8 + slot] = (uint32_t)__builtin_amdgcn_s_memtime();
    }
  };
  const uint32_t L0 = L;                           // first work item (PT: then L0 + nwg, ...)
  const int nt = PT ? (int)((ntile - L0 + nwg - 1) / nwg) : 1;   // tiles of this workgroup
  const int GT = nt * G::NCL;                      // chunks of this workgroup
  const int part = (int)(L % (uint32_t)P);        // hidden part (the parts of a tile share an XCD)
  L /= (uint32_t)P;
  const int cb = part * G::NCL;                    // first hidden chunk of this part
  auto tile_of = [&](uint32_t Lt, int& b_, int& oy0_, int& ox0_) {   // tile (without the part) -> image, origin
    const int tx_ = (int)(Lt % (uint32_t)tiles_x);
    Lt /= (uint32_t)tiles_x;
    b_ = (int)(Lt / (uint32_t)tiles_y);
    oy0_ = (int)(Lt % (uint32_t)tiles_y) * TH;
    ox0_ = tx_ * TW;
  };
  int b, oy0, ox0;
  tile_of(L, b, oy0, ox0);
  const int iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;
  // local chunk of global chunk g (G::NCL: none, past this workgroup's last tile)
  auto kmod = [&](int g) { return PT ? (g < GT ? g % G::NCL : G::NCL) : g; };
  auto slab = [&](int i) { return reinterpret_cast<float*>(smem + i * G::SLAB_B); };
  if (wave == 0) stamp(0, 3);                      // kernel entry (expand wave 0)
  auto se = [&](int i) { return smem + G::OFF_SE + i * G::SE_STR; };
  auto sd = [&](int i) { return reinterpret_cast<float*>(smem + G::OFF_SD + i * G::SD_STR); };
  auto sp = [&](int i) { return reinterpret_cast<_Float16*>(smem + G::OFF_SP + i * G::SP_STR); };

  // 16-B stage piece u of chunk k: kind 0 = expand (weights + bias, chunk ke), 1 = depthwise (chunk kd),
  // 2 = project (chunk kd). Source / destination pointers; null source = nothing to stage (chunk out of range).
  auto piece = [&](int u, int ke, int kd, const void*& src, void*& dst) {
    src = nullptr;
    dst = nullptr;
    if (u < G::NPE) {
      if (ke >= G::NCL) return;
      if (u < G::NPE - 8) {
        constexpr int PPR = G::CINP / 8;
        const int pl = u / (32 * PPR), rr = (u / PPR) % 32, g = u % PPR;
        src = We + (size_t)pl * G::HIDP * G::CINP + (size_t)(32 * (cb + ke) + rr) * G::CINP + 8 * g;
        dst = se(ke & 1) + ((pl * 32 + rr) * G::WES + 8 * g) * 2;
      } else {
        const int g = u - (G::NPE - 8);
        src = be + 32 * (cb + ke) + 4 * g;
        dst = se(ke & 1) + 2 * 32 * G::WES * 2 + 16 * g;
      }
      return;
    }
    u -= G::NPE;
    if (u < G::NPD) {
      if (kd >= G::NCL) return;
      if (u < 72) {
        const int tap = u >> 3, g = u & 7;
        src = Wd + (size_t)tap * G::HIDP + 32 * (cb + kd) + 4 * g;
        dst = sd(kd & 1) + tap * 32 + 4 * g;
      } else {
        src = bd + 32 * (cb + kd) + 4 * (u - 72);
        dst = sd(kd & 1) + 288 + 4 * (u - 72);
      }
      return;
    }
    u -= G::NPD;
    if (PST && u < G::NPP) {
      if (kd >= G::NCL) return;
      const int pl = u / (G::NPC * 4), rr = (u >> 2) % G::NPC, q = u & 3;
      src = Wp + (size_t)pl * G::NPC * G::HIDP + (size_t)rr * G::HIDP + 32 * (cb + kd) + 8 * q;
      dst = sp(kd & 1) + (pl * G::NPC + rr) * G::WPS + 8 * q;
    }
  };

  // ---- LDS-DMA stage pieces (G::GL). Expand waves: pieces e + NE j of the expand stage (weights hi / lo + bias); depthwise
  // waves: pieces d + ND j of the depthwise + project stage. Lane l of piece i fills LDS slot 64 i + l of the region
  // from a source whose address at chunk k is src0 + k * kstr (pad slots read a valid address of the same tensor).
  constexpr bool PAIR = !PST;
  const bool ewave = PAIR ? ((wave >> 1) & 1) == 0 : wave < G::NE;
  const int wr = PAIR ? (wave & 1) | ((wave >> 2) << 1) : ewave ? wave : wave - G::NE;   // index within the role
  if (!ewave && wr == 0) stamp(1, 7);              // kernel entry (depthwise wave 0)
  constexpr int NJ = G::GL ? (G::IEW > G::IDW ? G::IEW : G::IDW) : 1;
  const char* gsrc[NJ];
  int kstr[NJ];
#pragma unroll
  for (int j = 0; j < (G::GL ? NJ : 0); ++j) {
    const int off = ((ewave ? wr + G::NE * j : wr + G::ND * j) * 64 + lane) * 16;   // byte offset in the region
    const char* src;
    int ks;
    if (ewave) {
      constexpr int EW_B = 2 * 32 * G::WES * 2, ROW_B = G::WES * 2;
      if (off < EW_B) {
        const int pl = off / (32 * ROW_B), rem = off - pl * (32 * ROW_B), rr = rem / ROW_B;
        const int col = (rem - rr * ROW_B) / 16;
        src = reinterpret_cast<const char*>(We + (size_t)pl * G::HIDP * G::CINP + (size_t)(32 * cb + rr) * G::CINP +
                                            (col < G::CINP / 8 ? 8 * col : 0));
        ks = 32 * G::CINP * 2;
      } else {
        const int g = (off - EW_B) / 16;
        src = reinterpret_cast<const char*>(be + 32 * cb + (g < 8 ? 4 * g : 0));
        ks = 128;
      }
    } else {
      if (off < G::SD_BQ) {
        if (off < 1152) {
          src = reinterpret_cast<const char*>(Wd + (size_t)(off / 128) * G::HIDP + 32 * cb + 4 * ((off % 128) / 16));
        } else {
          const int g = (off - 1152) / 16;
          src = reinterpret_cast<const char*>(bd + 32 * cb + (g < 8 ? 4 * g : 0));
        }
        ks = 128;
      } else {
        const int o2 = off - G::SD_BQ;
        constexpr int ROW_B = G::WPS * 2;
        const int pl = o2 / (G::NPC * ROW_B), rem = o2 - pl * (G::NPC * ROW_B), rr = rem / ROW_B;
        const int q = (rem - rr * ROW_B) / 16;
        const bool ok = PST && o2 < G::SP_B;
        src = reinterpret_cast<const char*>(Wp + (ok ? (size_t)pl * G::NPC * G::HIDP + (size_t)rr * G::HIDP : 0) + 32 * cb +
                                            (ok && q < 4 ? 8 * q : 0));
        ks = 64;
      }
    }
    gsrc[j] = src;
    kstr[j] = ks;
  }
  // issue this wave's pieces of chunk k's stage (expand waves: the expand stage; depthwise waves: depthwise + project)
  auto dma = [&](int k) {
    if constexpr (!G::GL) return;
    char* base = ewave ? smem + G::OFF_SE + (k & 1) * G::SE_STR : smem + G::OFF_SD + (k & 1) * G::SD_STR;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int i = ewave ? wr + G::NE * j : wr + G::ND * j;
      if ((ewave && j < G::IEW && i < G::NIE) || (!ewave && j < G::IDW && i < G::NID))
        __builtin_amdgcn_global_load_lds((const void*)(gsrc[j] + (size_t)k * kstr[j]),
                                         (__attribute__((address_space(3))) void*)(base + i * 1024), 16, 0, 0);
    }
  };
  if constexpr (G::GL) {
    if (ewave) {
      dma(0);
      dma(1);
    } else {
      dma(0);
    }
  } else {
  // ---- prologue (all waves): expand stages of chunks 0 and 1, depthwise / project stage of chunk 0
    constexpr int NP0 = 2 * G::NPE + G::NPD + G::NPP;
    constexpr int NIT = (NP0 + G::NW * 64 - 1) / (G::NW * 64);
    uint4 v[NIT];
    void* dst[NIT];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      int u = tid + G::NW * 64 * i;
      const void* src = nullptr;
      dst[i] = nullptr;
      if (u < G::NPE) piece(u, 1, G::NCL, src, dst[i]);                     // expand chunk 1
      else if (u < NP0) piece(u - G::NPE, 0, 0, src, dst[i]);               // expand / dw / project chunk 0
      v[i] = src ? *reinterpret_cast<const uint4*>(src) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < NIT; ++i)
      if (dst[i]) *reinterpret_cast<uint4*>(dst[i]) = v[i];
  }

  if (ewave) {
    // ================= expand waves
    const int e = wr;
    // this wave's input-tile pixel tiles pt = e + NE j: B fragments (hi / lo) for every K step, loaded and split once
    // per tile. The fp32 rows are loaded into the fragments' own registers (8 floats of (j, ks) in the bits of
    // bxh[j][ks] | bxl[j][ks]) and split in place: no second register set
    f16x8 bxh[G::EPT][G::KS], bxl[G::EPT][G::KS];
    uint32_t pvmask = 0;   // bit j: pixel tile j's pixel of this lane is inside the map
    int soff[G::EPT];      // slab store offset (floats) of this lane's pixel, or the dummy rows
    auto pix = [&](int j, int iy0_, int ix0_, int& iy, int& ix) {   // input pixel of pixel tile j: inside the map?
      const int p = (e + G::NE * j) * 16 + r16;
      if (p >= G::PIN) return false;
      const int py = p / G::IW, px = p - py * G::IW;
      iy = iy0_ + py;
      ix = ix0_ + px;
      return iy >= 0 && iy < H && ix >= 0 && ix < W;
    };
    auto load_raw = [&](int b_, int iy0_, int ix0_) {   // fp32 input rows of the tile (zero outside the map)
      const float* Xb = X + (size_t)b_ * H * W * CIN;
#pragma unroll
      for (int j = 0; j < G::EPT; ++j) {
        int iy = 0, ix = 0;
        const bool ok = pix(j, iy0_, ix0_, iy, ix);
#pragma unroll
        for (int ks = 0; ks < G::KS; ++ks) {
          const int ch = 32 * ks + 8 * kg;
          float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0;
          if (ok && ch < CIN) {
            const float* src = Xb + ((size_t)iy * W + ix) * CIN + ch;
            r0 = *reinterpret_cast<const float4*>(src);
            r1 = *reinterpret_cast<const float4*>(src + 4);
          }
          bxh[j][ks] = __builtin_bit_cast(f16x8, r0);
          bxl[j][ks] = __builtin_bit_cast(f16x8, r1);
        }
      }
    };
    auto split_raw = [&]() {
#pragma unroll
      for (int j = 0; j < G::EPT; ++j)
#pragma unroll
        for (int ks = 0; ks < G::KS; ++ks) {
          const float4 a = __builtin_bit_cast(float4, bxh[j][ks]), c = __builtin_bit_cast(float4, bxl[j][ks]);
          const float v8[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
          split8(v8, bxh[j][ks], bxl[j][ks]);
        }
    };
    auto set_mask = [&](int iy0_, int ix0_) {   // PT: slab slots for every pixel of the tile (invalid ones get zeros)
      pvmask = 0;
#pragma unroll
      for (int j = 0; j < G::EPT; ++j) {
        const int p = (e + G::NE * j) * 16 + r16;
        int iy, ix;
        const bool ok = pix(j, iy0_, ix0_, iy, ix);
        if (ok) pvmask |= 1u << j;
        soff[j] = (PT ? p < G::PINP : ok) ? SL::at(p, kg) : G::OFF_TR / 4 + r16 * 24 + 4 * kg;
        if (!PT && !ok && p < G::PINP) {   // zero padding of the depthwise: both slabs, once
#pragma unroll
          for (int sb = 0; sb < 2; ++sb)
#pragma unroll
            for (int h = 0; h < 2; ++h)
              *reinterpret_cast<float4*>(slab(sb) + SL::at(p, kg) + 8 * h) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
    };
    load_raw(b, iy0, ix0);
    set_mask(iy0, ix0);
    split_raw();
    if (wave == 0) stamp(1, 3);   // input fragments loaded and split
    // expand of chunk k into slab k & 1 (stage k & 1)
    auto expand = [&](int k) {
      const char* S0 = se(k & 1);
      const float* eb = reinterpret_cast<const float*>(S0 + 2 * 32 * G::WES * 2);
      f32x4 acc[G::EPT][2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float4 bb = *reinterpret_cast<const float4*>(eb + 16 * h + 4 * kg);
#pragma unroll
        for (int j = 0; j < G::EPT; ++j) acc[j][h] = f32x4{bb.x, bb.y, bb.z, bb.w};
      }
      const _Float16* Ws = reinterpret_cast<const _Float16*>(S0);
#pragma unroll
      for (int ks = 0; ks < G::KS; ++ks) {
        f16x8 ah[2], al[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          ah[h] = *reinterpret_cast<const f16x8*>(Ws + (16 * h + r16) * G::WES + 32 * ks + 8 * kg);
          al[h] = *reinterpret_cast<const f16x8*>(Ws + (32 + 16 * h + r16) * G::WES + 32 * ks + 8 * kg);
        }
#pragma unroll
        for (int j = 0; j < G::EPT; ++j) {
#pragma unroll
          for (int h = 0; h < 2; ++h) acc[j][h] = mfma_x2(ah[h], al[h], bxh[j][ks], bxl[j][ks], acc[j][h]);
        }
      }
      // valid pixels -> slab k & 1; invalid ones -> the dummy rows (PT: zeros into their slab slots; slab offsets
      // are relative to slab 0, the dummy rows' to the LDS base, which is slab 0)
      float* Sl = reinterpret_cast<float*>(smem) + ((k & 1) ? G::SLAB_B / 4 : 0);
#pragma unroll
      for (int j = 0; j < G::EPT; ++j) {
        const bool pv = (pvmask >> j) & 1u;
        const int p = (e + G::NE * j) * 16 + r16;
        float* dst = (PT ? p < G::PINP : pv) ? Sl + soff[j] : reinterpret_cast<float*>(smem) + soff[j];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          float4 v = make_float4(fmaxf(acc[j][h][0], 0.f), fmaxf(acc[j][h][1], 0.f), fmaxf(acc[j][h][2], 0.f),
                                 fmaxf(acc[j][h][3], 0.f));
          if (PT && !pv) v = make_float4(0.f, 0.f, 0.f, 0.f);
          *reinterpret_cast<float4*>(dst + 8 * h) = v;
        }
      }
    };
    // PT, around the expand of global chunk gn: after a tile's last expand its successor's rows are loaded into the
    // (now dead) fragment registers, after that iteration's stage loads so the stage stores' vmcnt waits do not cover
    // them; chunk 0 of the next tile splits them. (An L2 prefetch chunks earlier by LDS-DMA into the dummy rows made
    // the compiler wait vmcnt(0) at every barrier, which serialises the register-staged weight loads.)
    auto next_tile = [&](int gn) {   // before expand(gn)
      if constexpr (PT) {
        if (gn % G::NCL == 0) {
          int b_, oy_, ox_;
          tile_of(L0 + (uint32_t)(gn / G::NCL) * nwg, b_, oy_, ox_);
          set_mask(oy_ * S - 1, ox_ * S - 1);
          split_raw();
        }
      }
    };
    auto fetch_tile = [&](int gn) {   // after expand(gn)
      if constexpr (PT) {
        const int cn = gn % G::NCL, tn = gn / G::NCL + 1;
        if (tn < nt && cn == G::NCL - 1) {
          int b_, oy_, ox_;
          tile_of(L0 + (uint32_t)tn * nwg, b_, oy_, ox_);
          load_raw(b_, oy_ * S - 1, ox_ * S - 1);
        }
      }
    };
    // Stage data is loaded one iteration before it is stored: the pieces of expand chunk c + 2 and depthwise /
    // project chunk c + 1 are fetched in iteration c - 1 (a whole chunk period of L2 latency hidden) and written to
    // LDS at the start of iteration c (the same buffers and barriers as a load-and-store in iteration c).
    if constexpr (G::GL) {
    __syncthreads();                 // prologue stages landed (vmcnt(0) + barrier)
    expand(0);
    __syncthreads();                 // slab 0 visible
#pragma unroll 1
    for (int c = 0; c < GT; ++c) {
      if (wave == 0) stamp(c, 0);
      if (c + 2 < GT) dma(kmod(c + 2));   // expand stage of chunk c + 2 into the buffer chunk c's expand released
      if (c + 1 < GT) {
        next_tile(c + 1);
        expand(kmod(c + 1));
        fetch_tile(c + 1);
      }
      if (wave == 0) stamp(c, 1);
      __syncthreads();                  // (waits for this wave's pieces: visible to every wave after the barrier)
    }
    } else {
    uint4 v[G::NPIECE];
    auto load_stage = [&](int c) {
#pragma unroll
      for (int i = 0; i < G::NPIECE; ++i) {
        const void* src;
        void* dst;
        piece(e * 64 + lane + G::NE * 64 * i, kmod(c + 2), kmod(c + 1), src, dst);
        v[i] = src ? *reinterpret_cast<const uint4*>(src) : make_uint4(0, 0, 0, 0);
      }
    };
    auto store_stage = [&](int c) {
#pragma unroll
      for (int i = 0; i < G::NPIECE; ++i) {
        const void* src;
        void* dst;
        piece(e * 64 + lane + G::NE * 64 * i, kmod(c + 2), kmod(c + 1), src, dst);
        if (src) *reinterpret_cast<uint4*>(dst) = v[i];
      }
    };
    load_stage(0);
    __syncthreads();                 // prologue stages visible
    expand(0);
    __syncthreads();                 // slab 0 visible
#pragma unroll 1
    for (int c = 0; c < GT; ++c) {
      if (wave == 0) stamp(c, 0);
      store_stage(c);                // expand chunk c + 2, depthwise / project chunk c + 1
      if (wave == 0) stamp(c, 2);
      if (c + 1 < GT) {
        load_stage(c + 1);
        next_tile(c + 1);
        expand(kmod(c + 1));
        fetch_tile(c + 1);
      }
      if (wave == 0) stamp(c, 1);
      __syncthreads();
    }
    }
  } else {
    // ================= depthwise / project waves
    const int d = wr;
    const int wp = d % G::WP, wc = d / G::WP;
    f32x4 acc[G::QPW][G::NCTW];
    auto init_acc = [&]() {
#pragma unroll
      for (int t = 0; t < G::NCTW; ++t) {   // (P > 1: the bias is added once, by the reduce)
        const float4 bb = P == 1 ? *reinterpret_cast<const float4*>(bp + (wc * G::NCTW + t) * 16 + 4 * kg)
                                 : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int q = 0; q < G::QPW; ++q) acc[q][t] = f32x4{bb.x, bb.y, bb.z, bb.w};
      }
    };
    init_acc();
    int pbase[G::QPW];
#pragma unroll
    for (int q = 0; q < G::QPW; ++q) {
      const int o = (wp * G::QPW + q) * 16 + r16;
      const int oy = o / TW, ox = o - (o / TW) * TW;
      pbase[q] = oy * S * G::IW + ox * S;
    }
    const _Float16* WpLo = Wp + (size_t)G::NPC * G::HIDP;
    f16x8 pgh[PST ? 1 : G::NCTW], pgl[PST ? 1 : G::NCTW];   // !PST: this chunk's project fragments from L2
    auto load_pg = [&](int k) {
      if constexpr (!PST) {
#pragma unroll
        for (int t = 0; t < G::NCTW; ++t) {
          const size_t off = (size_t)((wc * G::NCTW + t) * 16 + r16) * G::HIDP + 32 * (cb + k) + 8 * kg;
          pgh[t] = *reinterpret_cast<const f16x8*>(Wp + off);
          pgl[t] = *reinterpret_cast<const f16x8*>(WpLo + off);
        }
      }
    };
    // epilogue of the tile at (b_, oy0_, ox0_): + residual (the block input, pytorch_layers.py:93-96, added after the
    // BN bias; PT: fetched two chunks earlier into rres) -> fp32 NHWC
    constexpr int NRES = (PT && RES) ? G::QPW * G::NCTW : 1;
    float4 rres[NRES];
    auto out_pix = [&](int q, int b_, int oy0_, int ox0_, size_t& pix_) {
      const int o = (wp * G::QPW + q) * 16 + r16;
      const int oy = o / TW, ox = o - (o / TW) * TW;
      const int gy = oy0_ + oy, gx = ox0_ + ox;
      pix_ = ((size_t)b_ * OH + gy) * OW + gx;
      return gy < OH && gx < OW;
    };
    auto fetch_res = [&](int b_, int oy0_, int ox0_) {
      if constexpr (PT && RES) {
#pragma unroll
        for (int q = 0; q < G::QPW; ++q) {
          size_t pix_;
          const bool in = out_pix(q, b_, oy0_, ox0_, pix_);
#pragma unroll
          for (int t = 0; t < G::NCTW; ++t) {
            const int co = (wc * G::NCTW + t) * 16 + 4 * kg;
            rres[q * G::NCTW + t] = in && co < COUT ? *reinterpret_cast<const float4*>(X + pix_ * CIN + co)
                                                    : make_float4(0.f, 0.f, 0.f, 0.f);
          }
        }
      }
    };
    auto epilogue = [&](int b_, int oy0_, int ox0_) {
#pragma unroll
      for (int q = 0; q < G::QPW; ++q) {
        size_t pix;
        if (!out_pix(q, b_, oy0_, ox0_, pix)) continue;
#pragma unroll
        for (int t = 0; t < G::NCTW; ++t) {
          const int co = (wc * G::NCTW + t) * 16 + 4 * kg;
          if (co >= COUT) continue;
          f32x4 v = acc[q][t];
          if constexpr (P > 1) {   // partial sum of this hidden part
            *reinterpret_cast<float4*>(Y + part * pstride + pix * COUT + co) = make_float4(v[0], v[1], v[2], v[3]);
            continue;
          }
          if constexpr (RES) {
            const float4 r = PT ? rres[q * G::NCTW + t] : *reinterpret_cast<const float4*>(X + pix * CIN + co);
            v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
          }
          *reinterpret_cast<float4*>(Y + pix * COUT + co) = make_float4(v[0], v[1], v[2], v[3]);
        }
      }
    };
    load_pg(0);
    __syncthreads();
    __syncthreads();
#pragma unroll 1
    for (int g = 0; g < GT; ++g) {
      const int c = kmod(g);
      if (wr == 0) stamp(g, 4);
      if constexpr (G::GL)
        if (g + 1 < GT) dma(kmod(g + 1));   // depthwise + project stage of chunk g + 1 (buffer released by g - 1)
      const float* Sl = slab(c & 1);
      const float* D = sd(c & 1);
      f32x2 a[G::QPW][4];
      {
        const float4 d0 = *reinterpret_cast<const float4*>(D + 288 + 8 * kg);
        const float4 d1 = *reinterpret_cast<const float4*>(D + 288 + 8 * kg + 4);
#pragma unroll
        for (int q = 0; q < G::QPW; ++q) {
          a[q][0] = f32x2{d0.x, d0.y}; a[q][1] = f32x2{d0.z, d0.w};
          a[q][2] = f32x2{d1.x, d1.y}; a[q][3] = f32x2{d1.z, d1.w};
        }
      }
      // (block 17, !PST: no registers to spare for the batches; DWB 2 only where a wave owns one pixel tile)
      constexpr int DWB = !PST ? 0 : (SPEF_X2_DWB == 2 && G::QPW > 1 && CIN > SPEF_X2_DWB2_CIN) ? 1 : SPEF_X2_DWB;
      if constexpr (DWB > 0) {
      // column batches: the 3 taps' weights and slab rows of column kx issued together (sched_barrier keeps them
      // ahead of the FMAs), DWB 2: column kx + 1's batch issued before column kx's FMAs. Same FMA order.
      // ROWS: a wave's pixel tiles are consecutive output rows (16-wide tiles, stride 1), so tap (ky, q) reads input
      // row q + ky of the column: QPW + 2 row reads per column instead of 3 QPW
      constexpr bool ROWS = SPEF_X2_ROWS && S == 1 && TW == 16 && G::QPW > 1;
      constexpr int NR = ROWS ? G::QPW + 2 : 3 * G::QPW;
      float4 wv[DWB][3][2], sr[DWB][NR][2];
      auto col = [&](int kx, int bf) {
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          const float* wt = D + (ky * 3 + kx) * 32 + 8 * kg;
          wv[bf][ky][0] = *reinterpret_cast<const float4*>(wt);
          wv[bf][ky][1] = *reinterpret_cast<const float4*>(wt + 4);
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int p = ROWS ? pbase[0] + r * G::IW + kx : pbase[r % G::QPW] + (r / G::QPW) * G::IW + kx;
          sr[bf][r][0] = *reinterpret_cast<const float4*>(Sl + SL::at(p, 2 * kg));
          sr[bf][r][1] = *reinterpret_cast<const float4*>(Sl + SL::at(p, 2 * kg + 1));
        }
      };
      col(0, 0);
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int bf = DWB == 2 ? (kx & 1) : 0;
        if (DWB == 2 && kx < 2) col(kx + 1, bf ^ 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          const float4 w0 = wv[bf][ky][0], w1 = wv[bf][ky][1];
          const f32x2 w4[4] = {f32x2{w0.x, w0.y}, f32x2{w0.z, w0.w}, f32x2{w1.x, w1.y}, f32x2{w1.z, w1.w}};
#pragma unroll
          for (int q = 0; q < G::QPW; ++q) {
            const int r = ROWS ? q + ky : ky * G::QPW + q;
            dw_tap8(a[q], sr[bf][r][0], sr[bf][r][1], w4);
          }
        }
        if (DWB == 1 && kx < 2) {
          __builtin_amdgcn_sched_barrier(0);
          col(kx + 1, 0);
        }
      }
      } else {
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          const float* wt = D + (ky * 3 + kx) * 32 + 8 * kg;
          const float4 w0 = *reinterpret_cast<const float4*>(wt), w1 = *reinterpret_cast<const float4*>(wt + 4);
          const f32x2 w4[4] = {f32x2{w0.x, w0.y}, f32x2{w0.z, w0.w}, f32x2{w1.x, w1.y}, f32x2{w1.z, w1.w}};
#pragma unroll
          for (int q = 0; q < G::QPW; ++q) {
            const int p = pbase[q] + ky * G::IW + kx;
            dw_tap8(a[q], *reinterpret_cast<const float4*>(Sl + SL::at(p, 2 * kg)),
                    *reinterpret_cast<const float4*>(Sl + SL::at(p, 2 * kg + 1)), w4);
          }
        }
      }
      f16x8 bh[G::QPW], bl[G::QPW];
#pragma unroll
      for (int q = 0; q < G::QPW; ++q) relu_split8(a[q], bh[q], bl[q]);
      if (wr == 0) stamp(g, 5);
      if constexpr (PST) {
        const _Float16* Ps = sp(c & 1);
#pragma unroll
        for (int t = 0; t < G::NCTW; ++t) {
          const int row = (wc * G::NCTW + t) * 16 + r16;
          const f16x8 ph = *reinterpret_cast<const f16x8*>(Ps + row * G::WPS + 8 * kg);
          const f16x8 pl = *reinterpret_cast<const f16x8*>(Ps + (G::NPC + row) * G::WPS + 8 * kg);
#pragma unroll
          for (int q = 0; q < G::QPW; ++q) acc[q][t] = mfma_x2(ph, pl, bh[q], bl[q], acc[q][t]);
        }
      } else {
#pragma unroll
        for (int t = 0; t < G::NCTW; ++t)
#pragma unroll
          for (int q = 0; q < G::QPW; ++q) acc[q][t] = mfma_x2(pgh[t], pgl[t], bh[q], bl[q], acc[q][t]);
        if (g + 1 < GT) load_pg(kmod(g + 1));   // next chunk's fragments: in flight across the barrier and its depthwise
      }
      if constexpr (PT) {
        if (c == G::NCL - SPEF_X2_RES_AHEAD || c == G::NCL - 1) {
          int b_, oy_, ox_;
          tile_of(L0 + (uint32_t)(g / G::NCL) * nwg, b_, oy_, ox_);
          if (c == G::NCL - SPEF_X2_RES_AHEAD) {
            fetch_res(b_, oy_, ox_);
          } else {
            // the next tile's bias loads go out before the epilogue's stores: vmcnt counts both in order, so a
            // wait for loads issued after the stores would wait for the stores too
            float4 bn[G::NCTW];
#pragma unroll
            for (int t = 0; t < G::NCTW; ++t)
              bn[t] = *reinterpret_cast<const float4*>(bp + (wc * G::NCTW + t) * 16 + 4 * kg);
            epilogue(b_, oy_, ox_);
#pragma unroll
            for (int t = 0; t < G::NCTW; ++t)
#pragma unroll
              for (int q = 0; q < G::QPW; ++q) acc[q][t] = f32x4{bn[t].x, bn[t].y, bn[t].z, bn[t].w};
          }
        }
      }
      if (wr == 0) stamp(g, 6);
      __syncthreads();
    }
    if constexpr (!PT) epilogue(b, oy0, ox0);
    if (wr == 0) stamp(0, 7);   // epilogue stores issued
  }
  if constexpr (SPEF_X2_STAMP) {   // every wave: the last barrier, then the stamps over the start of tile 0's output
    __syncthreads();
    if (stamp_wg && tid < 8 * 64) {
      const int n = 8 * (GT < 64 ? GT : 64);
      if (tid < n) reinterpret_cast<uint32_t*>(Y)[tid] = reinterpret_cast<const uint32_t*>(smem + G::OFF_ST)[tid];
    }
  }
}

// The stage pieces a wave of one role issues per chunk (x2_irw_st_kernel): role piece i = wr + 4 j. Expand waves (EW):
// i < NIE is the expand stage's piece i, then the last G::DPE pieces of the depthwise | project region; depthwise waves:
// that region's pieces [0, NID - DPE). Per piece: this lane's source at chunk 0 (the only per-lane state) and, wave-uniform
// (scalar wave index; every sub-region is a whole number of pieces), the stride per chunk and the offset in its region.
template <class G, bool EW>
struct X2wPieces {
  static constexpr int N = EW ? G::NIE + G::DPE : G::NID - G::DPE, NJ = (N + 3) / 4;
  static_assert(G::DPE >= 0 && G::DPE <= G::NID, "pieces moved to the expand waves");
  static_assert(2 * 32 * G::WES * 2 % 1024 == 0 && G::SD_BQ % 1024 == 0, "a piece has one chunk stride");
  const char* src[NJ ? NJ : 1];
  int kstr[NJ ? NJ : 1], poff[NJ ? NJ : 1], wr;
  __device__ __forceinline__ X2wPieces(int wr_, int lane, const _Float16* We, const float* be, const float* Wd,
                                       const float* bd, const _Float16* Wp)
      : wr(wr_) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int i = wr + 4 * j;
      const bool es = EW && i < G::NIE;
      poff[j] = (es ? i : EW ? G::NID - G::DPE + (i - G::NIE) : i) * 1024;
      src[j] = x2w_stage_src<G>(es, poff[j] + lane * 16, We, be, Wd, bd, Wp);
      kstr[j] = x2w_stage_stride<G>(es, poff[j]);
    }
  }
  // expand chunk ke's pieces into stage ebuf (E) and depthwise / project chunk kd's into stage dbuf (D)
  template <bool E, bool D>
  __device__ __forceinline__ void issue(int ke, char* ebuf, int kd, char* dbuf) const {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int i = wr + 4 * j;
      const bool es = EW && i < G::NIE;
      if (i < N && (es ? E : D))
        __builtin_amdgcn_global_load_lds((const void*)(src[j] + (size_t)(es ? ke : kd) * kstr[j]),
                                         (__attribute__((address_space(3))) void*)((es ? ebuf : dbuf) + poff[j]), 16, 0,
                                         0);
    }
  }
};

// ------------------------------------------------------------------------------------------ static staging
// The persistent-tile rows (kind 3: blocks 8-10 and 14) with the staging discipline of x2_irp_kernel
// (SPEF_OPT_X2_STAGE = 1, the default; 0 runs x2_irw_kernel above). Same roles, same pipeline, same arithmetic in the
// same order (x2w_expand / x2w_dwproj are that kernel's bodies): bit-identical outputs. What differs is how a chunk's weights reach
// LDS and what the waves wait for:
//   * Each of slab, expand stage and depthwise + project stage is two separate static __shared__ arrays and the chunk
//     loop is unrolled by two, so every LDS access names its buffer at compile time and the compiler sees that a stage
//     read does not alias the stage an LDS-DMA of the same wave is filling (with one dynamic array it put vmcnt(0)
//     before the reads: every chunk waited out the round trip of the pieces it had just issued).
//   * Every stage piece moves by LDS-DMA (1-KiB lane-linear pieces), issued at the start of iteration g into the buffer
//     iteration g - 1 released: the expand stage of chunk g + 2 into Se[g & 1], the depthwise + project stage of chunk
//     g + 1 into Sd[(g + 1) & 1]. No stage goes through registers, so the expand role carries no ds_write of weights.
//     Expand waves issue the expand pieces and G::DPE of the depthwise / project pieces, depthwise waves the rest.
//   * The chunk barrier is lds_barrier(): it does not drain VMEM. A ds_read is not ordered behind another wave's pending
//     LDS-DMA, so each wave waits vmcnt(0) for its own pieces after its chunk's compute -- a chunk period after their
//     issue -- and before that barrier. vmcnt also counts the tile-transition traffic (the next tile's input rows, the
//     residual fetch, the epilogue stores): all of it is issued AFTER that wait, so the wait covers only the DMA pieces
//     (and, on the depthwise waves, stores a chunk old) and the transition traffic stays in flight across the barrier
//     as before. The next tile's bias comes from a copy in LDS (Sb), not from memory behind those stores.
template <int CIN, int HID, int COUT, int S, int TH, int TW, bool RES, int WCO>
__global__ __launch_bounds__(8 * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void x2_irw_st_kernel(
    const float* __restrict__ X, const _Float16* __restrict__ We, const float* __restrict__ be,
    const float* __restrict__ Wd, const float* __restrict__ bd, const _Float16* __restrict__ Wp,
    const float* __restrict__ bp, float* __restrict__ Y, int H, int W, int OH, int OW, int tiles_x, int tiles_y,
    uint32_t nwg, uint32_t ntile) {
  using G = X2wGeom<CIN, HID, COUT, S, TH, TW, WCO, true, 1>;
  using SL = typename G::SL;
  static_assert(G::NCL % 2 == 0 && G::ST_LDS <= 163840, "even chunk count (parity of a global chunk) / LDS budget");
  __shared__ __attribute__((aligned(16))) float Sl0[G::SLF], Sl1[G::SLF];                   // hidden chunk slabs + dummy rows
  __shared__ __attribute__((aligned(1024))) char Se0[G::SE_BQ], Se1[G::SE_BQ];     // expand stages
  __shared__ __attribute__((aligned(1024))) char Sd0[G::DP_BQ], Sd1[G::DP_BQ];     // depthwise | project stages
  __shared__ __attribute__((aligned(16))) float Sb[G::NPC];                        // project bias (accumulator resets)
  __shared__ uint32_t Stamps[SPEF_X2_STAMP ? 8 * 64 : 1];
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  auto slab = [&](auto p) -> float* { if constexpr (decltype(p)::value) return Sl1; else return Sl0; };
  auto se = [&](auto p) -> char* { if constexpr (decltype(p)::value) return Se1; else return Se0; };
  auto sd = [&](auto p) -> char* { if constexpr (decltype(p)::value) return Sd1; else return Sd0; };

  // (scalar wave index: the roles' branches, piece indices and strides stay off the vector registers)
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r16 = lane & 15, kg = lane >> 4;
  const uint32_t L0 = xcd_remap(blockIdx.x, nwg);   // first tile, then L0 + nwg, ...
  const int nt = (int)((ntile - L0 + nwg - 1) / nwg);
  const int GT = nt * G::NCL;                        // global chunks of this workgroup (even)
  auto tile_of = [&](int t, int& b_, int& oy0_, int& ox0_) {
    uint32_t Lt = L0 + (uint32_t)t * nwg;
    const int tx_ = (int)(Lt % (uint32_t)tiles_x);
    Lt /= (uint32_t)tiles_x;
    b_ = (int)(Lt / (uint32_t)tiles_y);
    oy0_ = (int)(Lt % (uint32_t)tiles_y) * TH;
    ox0_ = tx_ * TW;
  };
  const bool stamp_wg = SPEF_X2_STAMP && L0 == 0;   // the workgroup of tile 0 (its output holds the stamps)
  auto stamp = [&](int c, int slot) {               // tools/kstamp.py: slot 2 = after the DMA issue
    if constexpr (SPEF_X2_STAMP) {
      if (stamp_wg && lane == 0 && c < 64) Stamps[c * 8 + slot] = (uint32_t)__builtin_amdgcn_s_memtime();
    }
  };
  const bool ewave = wave < G::NE;
  static_assert(G::NE == 4 && G::ND == 4, "4 + 4 waves");
  const int wr = wave & 3;                          // index within the role
  if (wave == 0) stamp(0, 3);
  if (wave == G::NE) stamp(1, 7);

  if (ewave) {
    // ================= expand waves (x2_irw_kernel's, persistent tiles)
    const int e = wr;
    const X2wPieces<G, true> pieces(wr, lane, We, be, Wd, bd, Wp);
    pieces.template issue<true, true>(0, Se0, 0, Sd0);   // prologue: expand stages of chunks 0 and 1, depthwise /
    pieces.template issue<true, false>(1, Se1, 0, Sd1);  // project stage of chunk 0
    f16x8 bxh[G::EPT][G::KS], bxl[G::EPT][G::KS];
    uint32_t pvmask = 0;
    int soff[G::EPT];
    auto pix = [&](int j, int iy0_, int ix0_, int& iy, int& ix) {
      const int p = (e + G::NE * j) * 16 + r16;
      if (p >= G::PIN) return false;
      const int py = p / G::IW, px = p - py * G::IW;
      iy = iy0_ + py;
      ix = ix0_ + px;
      return iy >= 0 && iy < H && ix >= 0 && ix < W;
    };
    auto load_raw = [&](int t) {   // fp32 input rows of tile t into the fragment registers (zero outside the map)
      int b_, oy_, ox_;
      tile_of(t, b_, oy_, ox_);
      const float* Xb = X + (size_t)b_ * H * W * CIN;
#pragma unroll
      for (int j = 0; j < G::EPT; ++j) {
        int iy = 0, ix = 0;
        const bool ok = pix(j, oy_ * S - 1, ox_ * S - 1, iy, ix);
#pragma unroll
        for (int ks = 0; ks < G::KS; ++ks) {
          const int ch = 32 * ks + 8 * kg;
          float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0;
          if (ok && ch < CIN) {
            const float* src = Xb + ((size_t)iy * W + ix) * CIN + ch;
            r0 = *reinterpret_cast<const float4*>(src);
            r1 = *reinterpret_cast<const float4*>(src + 4);
          }
          bxh[j][ks] = __builtin_bit_cast(f16x8, r0);
          bxl[j][ks] = __builtin_bit_cast(f16x8, r1);
        }
      }
    };
    auto split_mask = [&](int t) {   // split tile t's loaded rows in place; slab slots / validity of its pixels
      int b_, oy_, ox_;
      tile_of(t, b_, oy_, ox_);
      pvmask = 0;
#pragma unroll
      for (int j = 0; j < G::EPT; ++j) {
        const int p = (e + G::NE * j) * 16 + r16;
        int iy, ix;
        if (pix(j, oy_ * S - 1, ox_ * S - 1, iy, ix)) pvmask |= 1u << j;
        // every slot of the tile is stored by every expand (zeros where invalid: a pixel valid in one tile may be
        // padding in the next); pixel tiles past the slab go to the dummy rows behind it
        soff[j] = p < G::PINP ? SL::at(p, kg) : SL::FLOATS + r16 * 24 + 4 * kg;
#pragma unroll
        for (int ks = 0; ks < G::KS; ++ks) {
          const float4 a = __builtin_bit_cast(float4, bxh[j][ks]), c = __builtin_bit_cast(float4, bxl[j][ks]);
          const float v8[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
          split8(v8, bxh[j][ks], bxl[j][ks]);
        }
      }
    };
    load_raw(0);
    split_mask(0);
    if (wave == 0) stamp(1, 3);
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): this wave's prologue pieces landed
    __syncthreads();
    x2w_expand<G>(Se0, Sl0, bxh, bxl, pvmask, soff, r16, kg);
    __syncthreads();                      // slab 0 visible
    // iteration g (parity p): this wave's pieces; E(g + 1) from stage p ^ 1 into slab p ^ 1 (the next tile's rows split
    // before its first chunk, loaded after the previous tile's last and after the wait for the pieces)
    auto iter = [&](auto par, int g) {
      using Q = std::integral_constant<int, decltype(par)::value ^ 1>;
      if (wave == 0) stamp(g, 0);
      const bool more = g + 1 < GT;
      const int cn = (g + 1) % G::NCL, tn = (g + 1) / G::NCL;   // chunk g + 1: local chunk, tile
      // vmcnt(0): only a next tile's rows can be in flight here, and its split below needs them. Said outright, so that
      // the compiler does not drain vmcnt -- with the pieces about to be issued -- at the first MFMA that reads bxh / bxl
      __builtin_amdgcn_s_waitcnt(0x0F70);
      if (more && cn == 0) split_mask(tn);
      pieces.template issue<true, true>((g + 2) % G::NCL, se(par), cn, sd(Q{}));
      if (wave == 0) stamp(g, 2);
      if (more) x2w_expand<G>(se(Q{}), slab(Q{}), bxh, bxl, pvmask, soff, r16, kg);
      __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): the pieces issued above (read by every wave after the barrier)
      if (more && cn == G::NCL - 1 && tn + 1 < nt) load_raw(tn + 1);
      if (wave == 0) stamp(g, 1);
      lds_barrier();
    };
#pragma unroll 1
    for (int g = 0; g < GT; g += 2) {
      iter(I0{}, g);
      iter(I1{}, g + 1);
    }
  } else {
    // ================= depthwise / project waves (x2_irw_kernel's, persistent tiles)
    const int d = wr;
    const X2wPieces<G, false> pieces(wr, lane, We, be, Wd, bd, Wp);
    pieces.template issue<false, true>(0, Se0, 0, Sd0);   // prologue: this role's part of chunk 0's depthwise / project stage
    const int wp = d % G::WP, wc = d / G::WP;
    const int co0 = wc * G::NCTW * 16 + 4 * kg;   // this lane's first output channel
    // ... as the tile transitions see it: opaque, so that X + co0 and Y + co0 are formed there, not kept in four
    // registers across the chunk loop (the depthwise role runs at the 256-register limit)
    auto co_here = [&] {
      int c_ = co0;
      asm volatile("" : "+v"(c_));
      return c_;
    };
    f32x4 acc[G::QPW][G::NCTW];
#pragma unroll
    for (int t = 0; t < G::NCTW; ++t) {
      const float4 bb = *reinterpret_cast<const float4*>(bp + co0 + 16 * t);
      *reinterpret_cast<float4*>(Sb + co0 + 16 * t) = bb;   // (this lane reads back what it wrote)
#pragma unroll
      for (int q = 0; q < G::QPW; ++q) acc[q][t] = f32x4{bb.x, bb.y, bb.z, bb.w};
    }
    int pbase[G::QPW];
#pragma unroll
    for (int q = 0; q < G::QPW; ++q) {
      const int o = (wp * G::QPW + q) * 16 + r16;
      const int oy = o / TW, ox = o - (o / TW) * TW;
      pbase[q] = oy * S * G::IW + ox * S;
    }
    // a tile's residual (the block input, pytorch_layers.py:93-96, added after the BN bias) is fetched
    // SPEF_X2_RES_AHEAD chunks before its end into rres. Output-channel tile t of this wave is channels
    // 16 (wc NCTW + t) + 4 kg .. + 3: one address per pixel tile, the tiles 64 B apart (instruction offsets).
    static_assert(COUT % 16 == 0 && (!RES || CIN == COUT), "whole output-channel tiles; a residual block keeps its width");
    constexpr int NRES = RES ? G::QPW * G::NCTW : 1;
    float4 rres[NRES];
    auto out_pix = [&](int q, int b_, int oy0_, int ox0_, size_t& pix_) {
      const int o = (wp * G::QPW + q) * 16 + r16;
      const int oy = o / TW, ox = o - (o / TW) * TW;
      const int gy = oy0_ + oy, gx = ox0_ + ox;
      pix_ = ((size_t)b_ * OH + gy) * OW + gx;
      return gy < OH && gx < OW;
    };
    auto fetch_res = [&](int b_, int oy0_, int ox0_) {
      if constexpr (RES) {
#pragma unroll
        for (int q = 0; q < G::QPW; ++q) {
          size_t pix_;
          const bool in = out_pix(q, b_, oy0_, ox0_, pix_);
          const float* xp = X + pix_ * CIN + co_here();
#pragma unroll
          for (int t = 0; t < G::NCTW; ++t)
            rres[q * G::NCTW + t] = in && (wc * G::NCTW + t) * 16 < COUT ? *reinterpret_cast<const float4*>(xp + 16 * t)
                                                                       : make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
    };
    auto epilogue = [&](int b_, int oy0_, int ox0_) {
#pragma unroll
      for (int q = 0; q < G::QPW; ++q) {
        size_t pix;
        if (!out_pix(q, b_, oy0_, ox0_, pix)) continue;
        float* yp = Y + pix * COUT + co_here();
#pragma unroll
        for (int t = 0; t < G::NCTW; ++t) {
          if ((wc * G::NCTW + t) * 16 >= COUT) continue;
          f32x4 v = acc[q][t];
          if constexpr (RES) {
            const float4 r = rres[q * G::NCTW + t];
            v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
          }
          *reinterpret_cast<float4*>(yp + 16 * t) = make_float4(v[0], v[1], v[2], v[3]);
        }
      }
    };
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): this wave's prologue pieces landed
    __syncthreads();
    __syncthreads();                      // slab 0 visible
    // iteration g (parity p): this wave's pieces of chunk g + 1's depthwise | project stage into stage p ^ 1 (released by
    // iteration g - 1); depthwise + project of chunk g from slab p and stage p
    auto iter = [&](auto par, int g) {
      using Q = std::integral_constant<int, decltype(par)::value ^ 1>;
      const int c = g % G::NCL;
      if (wr == 0) stamp(g, 4);
      pieces.template issue<false, true>(0, se(par), (g + 1) % G::NCL, sd(Q{}));
      x2w_dwproj<G, CIN, S, TW>(slab(par), reinterpret_cast<const float*>(sd(par)),
                                reinterpret_cast<const _Float16*>(sd(par) + G::SD_BQ), pbase, acc, wc, r16, kg,
                                [&] { if (wr == 0) stamp(g, 5); });
      __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): the pieces issued above (read by every wave after the barrier)
      if (c == G::NCL - SPEF_X2_RES_AHEAD || c == G::NCL - 1) {
        int b_, oy_, ox_;
        tile_of(g / G::NCL, b_, oy_, ox_);
        if (c == G::NCL - SPEF_X2_RES_AHEAD) {
          fetch_res(b_, oy_, ox_);
        } else {
          // the next tile's accumulators start from the bias kept in LDS: a global load here would sit in vmcnt behind
          // the epilogue's stores, and the compiler would drain it -- and the pieces just issued -- at the next MFMA
          epilogue(b_, oy_, ox_);
#pragma unroll
          for (int t = 0; t < G::NCTW; ++t) {
            const float4 bn = *reinterpret_cast<const float4*>(Sb + co0 + 16 * t);
#pragma unroll
            for (int q = 0; q < G::QPW; ++q) acc[q][t] = f32x4{bn.x, bn.y, bn.z, bn.w};
          }
        }
      }
      if (wr == 0) stamp(g, 6);
      lds_barrier();
    };
#pragma unroll 1
    for (int g = 0; g < GT; g += 2) {
      iter(I0{}, g);
      iter(I1{}, g + 1);
    }
    if (wr == 0) stamp(0, 7);   // epilogue stores issued
  }
  if constexpr (SPEF_X2_STAMP) {   // every wave: the last barrier, then the stamps over the start of tile 0's output
    __syncthreads();
    if (stamp_wg) {
      const int n = 8 * (GT < 64 ? GT : 64);
      if (tid < n) reinterpret_cast<uint32_t*>(Y)[tid] = Stamps[tid];
    }
  }
}

// Hidden-split join: y = ((part 0 + part 1) + ...) + bias (+ residual), in that order, 4 channels per thread.
template <int P, bool RES>
__global__ __launch_bounds__(256) void x2_split_reduce_kernel(const float* __restrict__ parts, size_t pstride,
                                                              const float* __restrict__ bias,
                                                              const float* __restrict__ X, float* __restrict__ Y,
                                                              size_t n4, int cout4) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  float4 v = reinterpret_cast<const float4*>(parts)[i];
#pragma unroll
  for (int p = 1; p < P; ++p) {
    const float4 u = reinterpret_cast<const float4*>(parts + p * pstride)[i];
    v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
  }
  const float4 bb = reinterpret_cast<const float4*>(bias)[i % (size_t)cout4];
  v.x += bb.x; v.y += bb.y; v.z += bb.z; v.w += bb.w;
  if constexpr (RES) {
    const float4 r = reinterpret_cast<const float4*>(X)[i];
    v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
  }
  reinterpret_cast<float4*>(Y)[i] = v;
}
// kind 1: project weights staged in LDS; kind 2: from L2; kind 3: kind 1 with persistent tiles (one part only)
template <int CIN, int HID, int COUT, int S, bool EXPAND, bool RES, int TH, int TW, int NW, int WCO, int KIND, int P>
static hipError_t x2_split_go(X2Row<CIN, HID, COUT, S, EXPAND, RES, TH, TW, NW, WCO, KIND, P>, const X2Args& a,
                              hipStream_t s) {
  static_assert(EXPAND && NW == 8, "role-split blocks expand, 4 + 4 waves");
  constexpr bool PT = KIND == 3 && P == 1;
  using G = X2wGeom<CIN, HID, COUT, S, TH, TW, WCO, KIND != 2, P>;
  TileGrid g;
  hipError_t e = tile_grid(g, a.OH, a.OW, TH, TW, a.B, P);
  if (e != hipSuccess) return e;
  if constexpr (PT) {   // static staging (static LDS: no attribute to raise, no dynamic size)
    if (a.stage) {
      const uint32_t grid = x2_persistent_grid(g.nwg, a.num_cu);
      x2_irw_st_kernel<CIN, HID, COUT, S, TH, TW, RES, WCO><<<grid, G::NW * 64, 0, s>>>(
          (const float*)a.x, (const _Float16*)a.we, a.be, a.wd, a.bd, (const _Float16*)a.wp, a.bp, (float*)a.y, a.H,
          a.W, a.OH, a.OW, g.tiles_x, g.tiles_y, grid, g.nwg);
      return hipGetLastError();
    }
  }
  auto k = x2_irw_kernel<CIN, HID, COUT, S, TH, TW, RES, WCO, KIND != 2, P, PT>;
  static DevOnce attr_set;
  if ((e = lds_attr_once(attr_set, k, G::LDS_BYTES)) != hipSuccess) return e;
  const size_t pstride = (size_t)a.B * a.OH * a.OW * COUT;   // floats per hidden part (16-B multiple: COUT % 4 == 0)
  if (P > 1 && !a.scratch) return hipErrorInvalidValue;
  const uint32_t grid = PT ? x2_persistent_grid(g.nwg, a.num_cu) : g.nwg;
  k<<<grid, G::NW * 64, G::LDS_BYTES, s>>>((const float*)a.x, (const _Float16*)a.we, a.be, a.wd, a.bd,
                                           (const _Float16*)a.wp, a.bp, P > 1 ? a.scratch : (float*)a.y, a.H, a.W,
                                           a.OH, a.OW, g.tiles_x, g.tiles_y, grid, pstride, g.nwg);
  if constexpr (P > 1) {
    const size_t n4 = pstride / 4;
    x2_split_reduce_kernel<P, RES><<<(unsigned)((n4 + 255) / 256), 256, 0, s>>>(a.scratch, pstride, a.bp,
                                                                                 (const float*)a.x, (float*)a.y, n4,
                                                                                 COUT / 4);
  }
  return hipGetLastError();
}

hipError_t launch_x2_split(const X2Block& b, const X2Plan& p, const X2Args& a, hipStream_t s) {
  return x2_visit_row<1, 3>(b, p, hipErrorNotSupported, [&](auto row) { return x2_split_go(row, a, s); });
}

}  // namespace spef
