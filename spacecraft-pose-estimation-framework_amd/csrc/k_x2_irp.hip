// fp16x2 three-stage kernel (x2_irp_kernel, plan kinds 5-6: blocks 11-13 and 15-17 at 512^2); the arithmetic and the
// kernel overview are in x2_common.hpp.
#include "spef_kernels.hpp"
#include "x2_common.hpp"

namespace spef {

// ------------------------------------------------------------------------------------------ three-stage form
// Blocks 15-16 (16x16 maps at 512^2: one 8x8 tile per CU, 30 hidden chunks), a three-stage pipeline with one barrier
// per chunk (the fp16 schedule's k_irp.hip structure with fp16x2 arithmetic):
//
//   MFMA waves [0, 4):  P(c-1)  project of chunk c - 1: B fragments (hi / lo depthwise outputs) from Ds[(c-1) & 1],
//                               A fragments from L2 (each wave its own output-channel tiles, one chunk ahead)
//                       E(c+1)  expand of chunk c + 1 into slab (c+1) & 1 (input fragments in registers, weights
//                               from the LDS stage that the same waves fill by LDS-DMA two chunks ahead)
//   VALU waves [4, 8):  V(c)    depthwise of chunk c from slab c & 1 (its weights by LDS-DMA one chunk ahead),
//                               ReLU, hi / lo split -> Ds[c & 1]
//
// Every double buffer is a separate static __shared__ array and the chunk loop is unrolled by two, so each LDS access
// names its buffer at compile time: the compiler's wait tracking (SIInsertWaitcnts, the LDS-DMA stores' alias scopes)
// then sees that a stage read does not alias the stage the same wave's LDS-DMA is filling, and does not drain vmcnt --
// i.e. the DMA just issued and the next project fragments -- before it (with one dynamic LDS array it waited there, and
// each chunk's 43 KB of weights were fetched synchronously: tools/kstamp_irp.py). The VALU waves hold no accumulators.
// Same operations per output, in the same order (fp32 depthwise kx outer / ky inner, relu_split8, three MFMAs per
// product accumulated over the chunks in order): bit-identical to the slab and role-split kernels. Ds: per buffer a hi
// and a lo plane of 64-B pixel rows (32 fp16 channels); granule kg of pixel p at position kg ^ (3 ((p >> 3) & 1)),
// conflict-free for the project's ds_read_b128 lane groups.
template <int CIN, int HID, int COUT, int S, int TH, int TW>
struct X2pGeom {
  static constexpr int NE = 4, ND = 4, NW = NE + ND;
  static constexpr int IH = (TH - 1) * S + 3, IW = (TW - 1) * S + 3;
  static constexpr int PIN = IH * IW, PIN16 = (PIN + 15) / 16, PINP = PIN16 * 16;
  static constexpr int CINP = (CIN + 31) / 32 * 32, KS = CINP / 32;
  static constexpr int WES = CINP + 16;                 // staged expand row (halves)
  using SL = X2Slab<S, PINP>;
  static constexpr int NCH = (HID + 31) / 32, HIDP = NCH * 32;
  static constexpr int NCT = (COUT + 15) / 16, NPC = NCT * 16;
  static constexpr int POUT16 = TH * TW / 16, QPV = POUT16 / ND;
  // the VALU waves' depthwise pixel tiles are consecutive output rows (16-wide tiles, stride 1): a column's input rows
  // are read once for both (4 row reads per column instead of 6)
  static constexpr bool ROWS = S == 1 && TW == 16 && QPV == 2;
  static constexpr int NCTW = (NCT + NE - 1) / NE;      // project output-channel tiles per MFMA wave
  static constexpr int EPT = (PIN16 + NE - 1) / NE;     // expand pixel tiles per MFMA wave
  static constexpr int SE_B = 2 * 32 * WES * 2 + 32 * 4, SE_BQ = (SE_B + 1023) / 1024 * 1024;
  static constexpr int SD_B = (9 * 32 + 32) * 4, SD_BQ = (SD_B + 1023) / 1024 * 1024;
  static constexpr int DS_PL = POUT16 * 16 * 64;        // one Ds plane (bytes)
  static constexpr int NIE = SE_BQ / 1024, NID = SD_BQ / 1024;
  static constexpr int SLF = SL::FLOATS + 16 * 24;    // a slab + its dummy rows (invalid pixels' expand stores)
  // PAL: the project A fragments staged in LDS, each MFMA wave's own tiles (by its own LDS-DMA, one chunk ahead),
  // instead of registers held across the expand -- where those registers (8 per output-channel tile) would spill:
  // block 17 (5 tiles per wave) 244 VGPRs, no spill, 101.5 -> 67.3 us per step at B = 64 on this kernel (from the
  // role-split kernel; tools/ktime.sh, bit-identical); blocks 15-16 (3 tiles) 102 -> 105 us with it, so they keep
  // the registers. Block 14 (EPT 5: 120 registers of input fragments) spills either way and has no LDS left for it.
  static constexpr int LDS_BASE = 2 * SLF * 4 + 2 * SE_BQ + 2 * SD_BQ + 4 * DS_PL;
  static constexpr bool PAL = NCTW >= 4 && POUT16 <= 4 && LDS_BASE + NE * NCTW * 2048 <= 163840;
  static constexpr int SP_B = PAL ? NE * NCTW * 2048 : 0;
  static constexpr int LDS_BYTES = LDS_BASE + SP_B;
  static_assert(CIN % 8 == 0 && COUT % 16 == 0 && HID % 32 == 0, "channel counts");
  static_assert(TH * TW % 16 == 0 && POUT16 % ND == 0 && NCH >= 4 && NCH % 2 == 0, "tile split / pipeline depth");
  static_assert(EPT <= 32 && LDS_BYTES <= 163840, "validity mask / LDS budget");
};

// PT (persistent tiles, the maps with more tiles than CUs): a workgroup runs tiles L, L + nwg, ... < ntile as ONE
// stream of global chunks g = t NCH + c (NCH even, so the parity of g is that of c): the MFMA waves load the next tile's
// input rows into their fragment registers after its predecessor's last expand and split them before its first, and
// store a tile's outputs right after its last project; invalid input pixels are stored as zeros by every expand (a
// pixel valid in one tile may be padding in the next).
template <int CIN, int HID, int COUT, int S, int TH, int TW, bool RES, bool PT>
__global__ __launch_bounds__(8 * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void x2_irp_kernel(
    const float* __restrict__ X, const _Float16* __restrict__ We, const float* __restrict__ be,
    const float* __restrict__ Wd, const float* __restrict__ bd, const _Float16* __restrict__ Wp,
    const float* __restrict__ bp, float* __restrict__ Y, int H, int W, int OH, int OW, int tiles_x, int tiles_y,
    uint32_t nwg, uint32_t ntile) {
  using G = X2pGeom<CIN, HID, COUT, S, TH, TW>;
  using SL = typename G::SL;
  __shared__ __attribute__((aligned(16))) float Sl0[G::SLF], Sl1[G::SLF];   // hidden chunk slabs (fp32) + dummy rows
  __shared__ __attribute__((aligned(1024))) char Se0[G::SE_BQ], Se1[G::SE_BQ];       // expand stages
  __shared__ __attribute__((aligned(1024))) char Sd0[G::SD_BQ], Sd1[G::SD_BQ];       // depthwise stages
  __shared__ __attribute__((aligned(16))) char Ds0[2 * G::DS_PL], Ds1[2 * G::DS_PL]; // depthwise outputs hi | lo
  __shared__ __attribute__((aligned(1024))) char Sp[G::PAL ? G::SP_B : 16];          // project A stage (PAL)
  __shared__ uint32_t Stamps[SPEF_X2_STAMP ? 8 * 64 : 1];
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  auto slab = [&](auto p) -> float* { if constexpr (decltype(p)::value) return Sl1; else return Sl0; };
  auto se = [&](auto p) -> char* { if constexpr (decltype(p)::value) return Se1; else return Se0; };
  auto sd = [&](auto p) -> char* { if constexpr (decltype(p)::value) return Sd1; else return Sd0; };
  auto dsb = [&](auto p) -> char* { if constexpr (decltype(p)::value) return Ds1; else return Ds0; };

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r16 = lane & 15, kg = lane >> 4;
  const uint32_t L0 = xcd_remap(blockIdx.x, nwg);   // first tile (PT: then L0 + nwg, ...)
  const int nt = PT ? (int)((ntile - L0 + nwg - 1) / nwg) : 1;
  const int GT = nt * G::NCH;                        // global chunks of this workgroup
  auto kmod = [&](int g) { return PT ? g % G::NCH : g; };
  auto tile_of = [&](int t, int& b_, int& oy0_, int& ox0_) {
    uint32_t Lt = L0 + (uint32_t)t * nwg;
    const int tx_ = (int)(Lt % (uint32_t)tiles_x);
    Lt /= (uint32_t)tiles_x;
    b_ = (int)(Lt / (uint32_t)tiles_y);
    oy0_ = (int)(Lt % (uint32_t)tiles_y) * TH;
    ox0_ = tx_ * TW;
  };
  const int dsx = 16 * (kg ^ (3 * ((r16 >> 3) & 1)));                         // this lane's Ds granule (bytes)
  const bool stamp_wg = SPEF_X2_STAMP && blockIdx.x == 0;
  auto stamp = [&](int c, int slot) {   // timing builds (tools/kstamp_irp.py): lane 0's shader clock into slot (c, slot)
    if constexpr (SPEF_X2_STAMP) {
      if (stamp_wg && lane == 0 && c < 64) Stamps[c * 8 + slot] = (uint32_t)__builtin_amdgcn_s_memtime();
    }
  };
  if (wave == 0) stamp(0, 3);
  if (wave == G::NE) stamp(1, 7);

  // Stage pieces, all moved by LDS-DMA from the VALU waves (the MFMA waves' critical path then carries none of it): the
  // expand stage (weights hi / lo + bias, 1-KiB pieces d + ND j) and the depthwise stage (weights + bias); lane l of
  // piece i fills slot 64 i + l of the region from src0 + k * kstr at chunk k (pad slots read a valid address of the
  // same tensor). Measured per step at B = 64 (tools/ktime.sh): blocks 15-16 with the expand stage issued by the MFMA
  // waves 102.9 -> 116.6 us, register staging (global loads an iteration ahead + ds_write) instead of LDS-DMA 181 us.
  const bool ewave = wave < G::NE;
  const int wr = ewave ? wave : wave - G::NE;
  constexpr int NJE = (G::NIE + G::ND - 1) / G::ND, NJD = (G::NID + G::ND - 1) / G::ND;
  const char* esrc[NJE];
  const char* dsrc[NJD];
  int ekstr[NJE];
#pragma unroll
  for (int j = 0; j < NJE; ++j) {
    const int off = ((wr + G::ND * j) * 64 + lane) * 16;
    constexpr int EW_B = 2 * 32 * G::WES * 2, ROW_B = G::WES * 2;
    if (off < EW_B) {
      const int pl = off / (32 * ROW_B), rem = off - pl * (32 * ROW_B), rr = rem / ROW_B;
      const int col = (rem - rr * ROW_B) / 16;
      esrc[j] = reinterpret_cast<const char*>(We + (size_t)pl * G::HIDP * G::CINP + (size_t)rr * G::CINP +
                                              (col < G::CINP / 8 ? 8 * col : 0));
      ekstr[j] = 32 * G::CINP * 2;
    } else {
      const int g = (off - EW_B) / 16;
      esrc[j] = reinterpret_cast<const char*>(be + (g < 8 ? 4 * g : 0));
      ekstr[j] = 128;
    }
  }
#pragma unroll
  for (int j = 0; j < NJD; ++j) {
    const int off = ((wr + G::ND * j) * 64 + lane) * 16;
    dsrc[j] = off < 1152 ? reinterpret_cast<const char*>(Wd + (size_t)(off / 128) * G::HIDP + 4 * ((off % 128) / 16))
                         : reinterpret_cast<const char*>(bd + (off - 1152 < 128 ? 4 * ((off - 1152) / 16) : 0));
  }
  auto dma_e = [&](int k, char* base) {
#pragma unroll
    for (int j = 0; j < NJE; ++j)
      if (wr + G::ND * j < G::NIE)
        __builtin_amdgcn_global_load_lds((const void*)(esrc[j] + (size_t)k * ekstr[j]),
                                         (__attribute__((address_space(3))) void*)(base + (wr + G::ND * j) * 1024), 16,
                                         0, 0);
  };
  auto dma_d = [&](int k, char* base) {
#pragma unroll
    for (int j = 0; j < NJD; ++j)
      if (wr + G::ND * j < G::NID)
        __builtin_amdgcn_global_load_lds((const void*)(dsrc[j] + (size_t)k * 128),
                                         (__attribute__((address_space(3))) void*)(base + (wr + G::ND * j) * 1024), 16,
                                         0, 0);
  };
  if (!ewave) {
    dma_e(0, Se0);
    dma_e(1, Se1);
    dma_d(0, Sd0);
  }

  if (ewave) {
    // ================= MFMA waves: expand (pixel tiles e + NE j, both hidden halves) and project (output-channel tiles
    // e + NE t, every output pixel tile)
    const int e = wr;
    // input-tile B fragments (hi / lo) for every K step; the fp32 rows are loaded into the fragments' own registers (8
    // floats of (j, ks) in the bits of bxh[j][ks] | bxl[j][ks]) and split in place
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
    auto load_raw = [&](int t) {   // fp32 input rows of tile t (zero outside the map)
      int b_, oy_, ox_;
      tile_of(t, b_, oy_, ox_);
      const float* Xb = X + (size_t)b_ * H * W * CIN;
#pragma unroll
      for (int j = 0; j < G::EPT; ++j) {
        int iy = 0, ix = 0;
        const bool ok = e + G::NE * j < G::PIN16 && pix(j, oy_ * S - 1, ox_ * S - 1, iy, ix);
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
        const bool ok = pix(j, oy_ * S - 1, ox_ * S - 1, iy, ix);
        if (ok) pvmask |= 1u << j;
        // PT: every slot of the tile is stored by every expand (zeros where invalid); else invalid pixels hold the
        // zeros stored once below and their expand stores go to the dummy rows
        soff[j] = (PT ? p < G::PINP : ok) ? SL::at(p, kg) : SL::FLOATS + r16 * 24 + 4 * kg;
#pragma unroll
        for (int ks = 0; ks < G::KS; ++ks) {
          const float4 a = __builtin_bit_cast(float4, bxh[j][ks]), c = __builtin_bit_cast(float4, bxl[j][ks]);
          const float v8[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
          split8(v8, bxh[j][ks], bxl[j][ks]);
        }
        if (!PT && !ok && p < G::PINP) {   // the depthwise's zero padding: both slabs, once
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            *reinterpret_cast<float4*>(Sl0 + SL::at(p, kg) + 8 * h) = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(Sl1 + SL::at(p, kg) + 8 * h) = make_float4(0.f, 0.f, 0.f, 0.f);
          }
        }
      }
    };
    load_raw(0);
    split_mask(0);
    // expand of a chunk: weights from stage `sp`, ReLU'd fp32 results into slab `sl`
    auto expand = [&](const char* sp, float* sl) {
      const float* eb = reinterpret_cast<const float*>(sp + 2 * 32 * G::WES * 2);
      f32x4 acc[G::EPT][2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float4 bb = *reinterpret_cast<const float4*>(eb + 16 * h + 4 * kg);
#pragma unroll
        for (int j = 0; j < G::EPT; ++j) acc[j][h] = f32x4{bb.x, bb.y, bb.z, bb.w};
      }
      const _Float16* Ws = reinterpret_cast<const _Float16*>(sp);
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
          if (e + G::NE * j >= G::PIN16) continue;   // (wave-uniform)
#pragma unroll
          for (int h = 0; h < 2; ++h) acc[j][h] = mfma_x2(ah[h], al[h], bxh[j][ks], bxl[j][ks], acc[j][h]);
        }
      }
#pragma unroll
      for (int j = 0; j < G::EPT; ++j) {
        if (e + G::NE * j >= G::PIN16) continue;
        const bool pv = (pvmask >> j) & 1u;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          float4 v = make_float4(fmaxf(acc[j][h][0], 0.f), fmaxf(acc[j][h][1], 0.f), fmaxf(acc[j][h][2], 0.f),
                                 fmaxf(acc[j][h][3], 0.f));
          if (PT && !pv) v = make_float4(0.f, 0.f, 0.f, 0.f);
          *reinterpret_cast<float4*>(sl + soff[j] + 8 * h) = v;
        }
      }
    };
    // project: accumulators (bias) of this wave's output-channel tiles, A fragments of chunk k from L2
    f32x4 acc[G::POUT16][G::NCTW];
    auto init_acc = [&]() {
#pragma unroll
      for (int t = 0; t < G::NCTW; ++t) {
        float4 bb = make_float4(0.f, 0.f, 0.f, 0.f);
        if (e + G::NE * t < G::NCT) bb = *reinterpret_cast<const float4*>(bp + (e + G::NE * t) * 16 + 4 * kg);
#pragma unroll
        for (int q = 0; q < G::POUT16; ++q) acc[q][t] = f32x4{bb.x, bb.y, bb.z, bb.w};
      }
    };
    init_acc();
    const _Float16* WpLo = Wp + (size_t)G::NPC * G::HIDP;
    f16x8 pah[G::NCTW], pal[G::NCTW];
    char* const spw = Sp + wr * (G::NCTW * 2048);   // PAL: this wave's A stage (tile t: hi at 2048 t, lo + 1024)
    auto load_pa = [&](int k) {
#pragma unroll
      for (int t = 0; t < G::NCTW; ++t)
        if (e + G::NE * t < G::NCT) {
          const size_t off = (size_t)((e + G::NE * t) * 16 + r16) * G::HIDP + 32 * k + 8 * kg;
          if constexpr (G::PAL) {
            __builtin_amdgcn_global_load_lds((const void*)(Wp + off),
                                             (__attribute__((address_space(3))) void*)(spw + t * 2048), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const void*)(WpLo + off),
                                             (__attribute__((address_space(3))) void*)(spw + t * 2048 + 1024), 16, 0,
                                             0);
          } else {
            pah[t] = *reinterpret_cast<const f16x8*>(Wp + off);
            pal[t] = *reinterpret_cast<const f16x8*>(WpLo + off);
          }
        }
    };
    // the B fragments of pixel tile q + 1 are read before tile q's MFMAs (each read pair's LDS latency hides behind
    // the previous tile's MFMAs instead of stalling the MFMA role)
    auto project = [&](const char* Dh) {
      if constexpr (G::PAL) {   // all pixel tiles' B fragments, then output-channel tile by tile (its A from the stage)
        f16x8 bh[G::POUT16], bl[G::POUT16];
#pragma unroll
        for (int q = 0; q < G::POUT16; ++q) {
          bh[q] = *reinterpret_cast<const f16x8*>(Dh + (q * 16 + r16) * 64 + dsx);
          bl[q] = *reinterpret_cast<const f16x8*>(Dh + G::DS_PL + (q * 16 + r16) * 64 + dsx);
        }
#pragma unroll
        for (int t = 0; t < G::NCTW; ++t) {
          if (e + G::NE * t >= G::NCT) continue;
          const f16x8 ah = *reinterpret_cast<const f16x8*>(spw + t * 2048 + 16 * lane);
          const f16x8 al = *reinterpret_cast<const f16x8*>(spw + t * 2048 + 1024 + 16 * lane);
#pragma unroll
          for (int q = 0; q < G::POUT16; ++q) acc[q][t] = mfma_x2(ah, al, bh[q], bl[q], acc[q][t]);
        }
        return;
      }
      f16x8 bh[2], bl[2];
      bh[0] = *reinterpret_cast<const f16x8*>(Dh + r16 * 64 + dsx);
      bl[0] = *reinterpret_cast<const f16x8*>(Dh + G::DS_PL + r16 * 64 + dsx);
#pragma unroll
      for (int q = 0; q < G::POUT16; ++q) {
        if (q + 1 < G::POUT16) {
          bh[(q + 1) & 1] = *reinterpret_cast<const f16x8*>(Dh + ((q + 1) * 16 + r16) * 64 + dsx);
          bl[(q + 1) & 1] = *reinterpret_cast<const f16x8*>(Dh + G::DS_PL + ((q + 1) * 16 + r16) * 64 + dsx);
        }
#pragma unroll
        for (int t = 0; t < G::NCTW; ++t)
          if (e + G::NE * t < G::NCT) acc[q][t] = mfma_x2(pah[t], pal[t], bh[q & 1], bl[q & 1], acc[q][t]);
      }
    };
    // + residual (the block input, pytorch_layers.py:93-96, added after the BN bias) -> fp32 NHWC, tile t; the residual
    // loads of four pixel tiles are issued together (one memory round trip per group, not per value)
    auto epilogue = [&](int t) {
      int b_, oy_, ox_;
      tile_of(t, b_, oy_, ox_);
      constexpr int QG = G::POUT16 < 4 ? G::POUT16 : 4;
#pragma unroll
      for (int q0 = 0; q0 < G::POUT16; q0 += QG) {
        float4 r[QG][G::NCTW];
        size_t pix_[QG];
        bool in[QG];
#pragma unroll
        for (int qq = 0; qq < QG; ++qq) {
          const int o = (q0 + qq) * 16 + r16;
          const int gy = oy_ + o / TW, gx = ox_ + o % TW;
          in[qq] = gy < OH && gx < OW;
          pix_[qq] = ((size_t)b_ * OH + gy) * OW + gx;
#pragma unroll
          for (int tt = 0; tt < G::NCTW; ++tt) {
            r[qq][tt] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (RES && in[qq] && e + G::NE * tt < G::NCT)
              r[qq][tt] = *reinterpret_cast<const float4*>(X + pix_[qq] * CIN + (e + G::NE * tt) * 16 + 4 * kg);
          }
        }
#pragma unroll
        for (int qq = 0; qq < QG; ++qq) {
          if (!in[qq]) continue;
#pragma unroll
          for (int tt = 0; tt < G::NCTW; ++tt) {
            if (e + G::NE * tt >= G::NCT) continue;
            f32x4 v = acc[q0 + qq][tt];
            if constexpr (RES) {
              v[0] += r[qq][tt].x; v[1] += r[qq][tt].y; v[2] += r[qq][tt].z; v[3] += r[qq][tt].w;
            }
            *reinterpret_cast<float4*>(Y + pix_[qq] * COUT + (e + G::NE * tt) * 16 + 4 * kg) =
                make_float4(v[0], v[1], v[2], v[3]);
          }
        }
      }
    };
    load_pa(0);
    if (wave == 0) stamp(1, 3);
    __syncthreads();   // prologue stages landed (the VALU waves waited for their LDS-DMA)
    expand(Se0, Sl0);
    __syncthreads();   // slab 0 visible
    // iteration g (parity p = g & 1): P(g - 1) from Ds[p ^ 1] and the fragments of its chunk (PT: then, at a tile's
    // last chunk, the tile's outputs); chunk g's project fragments (in flight across E(g + 1) and the barrier); E(g + 1)
    // from stage p ^ 1 into slab p ^ 1 (PT: the next tile's rows split before its first chunk, loaded after the previous
    // tile's last)
    auto iter = [&](auto par, int g) {
      using Q = std::integral_constant<int, decltype(par)::value ^ 1>;
      if (wave == 0) stamp(g, 0);
      if (g >= 1) {
        project(dsb(Q{}));
        if (PT && kmod(g - 1) == G::NCH - 1) {
          epilogue((g - 1) / G::NCH);
          init_acc();
        }
      }
      if (g >= 1) load_pa(kmod(g));
      if (wave == 0) stamp(g, 1);
      if (g + 1 < GT) {
        if (PT && kmod(g + 1) == 0) split_mask((g + 1) / G::NCH);
        expand(se(Q{}), slab(Q{}));
        if (PT && kmod(g + 1) == G::NCH - 1 && (g + 1) / G::NCH + 1 < nt) load_raw((g + 1) / G::NCH + 1);
      }
      if (wave == 0) stamp(g, 2);
      lds_barrier();
    };
#pragma unroll 1
    for (int g = 0; g < GT; g += 2) {
      iter(I0{}, g);
      iter(I1{}, g + 1);
    }
    project(dsb(I1{}));   // (GT is even: the last chunk's parity is 1)
    epilogue(nt - 1);
    if (wave == 0) stamp(0, 7);
  } else {
    // ================= VALU waves: depthwise of output pixel tiles QPV d .. QPV d + QPV - 1 -> Ds
    const int d = wr;
    int pbase[G::QPV];
#pragma unroll
    for (int i = 0; i < G::QPV; ++i) {
      const int o = (G::QPV * d + i) * 16 + r16;
      pbase[i] = (o / TW) * S * G::IW + (o % TW) * S;
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): the prologue stages landed
    __syncthreads();
    __syncthreads();   // slab 0 visible
    // iteration g (parity p): expand chunk g + 2's stage into stage p (released by E(g) in iteration g - 1) and depthwise
    // chunk g + 1's into stage p ^ 1 (released by V(g - 1)), from the registers loaded an iteration ago; the loads of
    // expand chunk g + 3 and depthwise chunk g + 2; V(g) from slab p and stage p into Ds[p]
    auto iter = [&](auto par, int g) {
      using Q = std::integral_constant<int, decltype(par)::value ^ 1>;
      if (wave == G::NE) stamp(g, 4);
      if (g + 2 < GT) dma_e(kmod(g + 2), se(par));
      if (g + 1 < GT) dma_d(kmod(g + 1), sd(Q{}));
      if (wave == G::NE) stamp(g, 5);
      const float* Sl = slab(par);
      const float* D = reinterpret_cast<const float*>(sd(par));
      char* Dh = dsb(par);
      const float4 d0 = *reinterpret_cast<const float4*>(D + 288 + 8 * kg);
      const float4 d1 = *reinterpret_cast<const float4*>(D + 288 + 8 * kg + 4);
      f32x2 a[G::QPV][4];
#pragma unroll
      for (int i = 0; i < G::QPV; ++i) {
        a[i][0] = f32x2{d0.x, d0.y}; a[i][1] = f32x2{d0.z, d0.w};
        a[i][2] = f32x2{d1.x, d1.y}; a[i][3] = f32x2{d1.z, d1.w};
      }
      // every tap's weights and the window's slab rows issued together (the VALU waves hold no accumulators): QPV + 2
      // shared rows per column (ROWS) or 3 per pixel tile
      constexpr int NR = G::ROWS ? G::QPV + 2 : 3 * G::QPV;
      float4 wv[3][3][2], sv[3][NR][2];
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          const float* wt = D + (ky * 3 + kx) * 32 + 8 * kg;
          wv[kx][ky][0] = *reinterpret_cast<const float4*>(wt);
          wv[kx][ky][1] = *reinterpret_cast<const float4*>(wt + 4);
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int p = G::ROWS ? pbase[0] + r * G::IW + kx : pbase[r / 3] + (r % 3) * G::IW + kx;
          sv[kx][r][0] = *reinterpret_cast<const float4*>(Sl + SL::at(p, 2 * kg));
          sv[kx][r][1] = *reinterpret_cast<const float4*>(Sl + SL::at(p, 2 * kg + 1));
        }
      }
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          const f32x2 w4[4] = {f32x2{wv[kx][ky][0].x, wv[kx][ky][0].y}, f32x2{wv[kx][ky][0].z, wv[kx][ky][0].w},
                               f32x2{wv[kx][ky][1].x, wv[kx][ky][1].y}, f32x2{wv[kx][ky][1].z, wv[kx][ky][1].w}};
#pragma unroll
          for (int i = 0; i < G::QPV; ++i) {
            const int r = G::ROWS ? i + ky : 3 * i + ky;
            dw_tap8(a[i], sv[kx][r][0], sv[kx][r][1], w4);
          }
        }
#pragma unroll
      for (int i = 0; i < G::QPV; ++i) {
        f16x8 bh, bl;
        relu_split8(a[i], bh, bl);
        const int o = (G::QPV * d + i) * 16 + r16;
        *reinterpret_cast<f16x8*>(Dh + o * 64 + dsx) = bh;
        *reinterpret_cast<f16x8*>(Dh + G::DS_PL + o * 64 + dsx) = bl;
      }
      if (wave == G::NE) stamp(g, 6);
      __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): the DMA pieces landed (read by every wave next)
      lds_barrier();
    };
#pragma unroll 1
    for (int g = 0; g < GT; g += 2) {
      iter(I0{}, g);
      iter(I1{}, g + 1);
    }
  }
  if constexpr (SPEF_X2_STAMP) {   // every wave: the last barrier, then the stamps over the start of tile 0's output
    __syncthreads();
    if (stamp_wg) {
      const int n = 8 * (G::NCH < 64 ? G::NCH : 64);
      if (tid < n) reinterpret_cast<uint32_t*>(Y)[tid] = Stamps[tid];
    }
  }
}
// kind 5: one tile per workgroup; kind 6: persistent tiles. Static LDS (G::LDS_BYTES), so no attribute to raise.
template <int CIN, int HID, int COUT, int S, bool EXPAND, bool RES, int TH, int TW, int NW, int WCO, int KIND, int P>
static hipError_t x2_stage3_go(X2Row<CIN, HID, COUT, S, EXPAND, RES, TH, TW, NW, WCO, KIND, P>, const X2Args& a,
                               hipStream_t s) {
  static_assert(EXPAND && P == 1, "three-stage blocks expand, one part");
  constexpr bool PT = KIND == 6;
  using G = X2pGeom<CIN, HID, COUT, S, TH, TW>;
  TileGrid g;
  const hipError_t e = tile_grid(g, a.OH, a.OW, TH, TW, a.B);
  if (e != hipSuccess) return e;
  const uint32_t grid = PT ? x2_persistent_grid(g.nwg, a.num_cu) : g.nwg;
  x2_irp_kernel<CIN, HID, COUT, S, TH, TW, RES, PT><<<grid, G::NW * 64, 0, s>>>(
      (const float*)a.x, (const _Float16*)a.we, a.be, a.wd, a.bd, (const _Float16*)a.wp, a.bp, (float*)a.y, a.H, a.W,
      a.OH, a.OW, g.tiles_x, g.tiles_y, grid, g.nwg);
  return hipGetLastError();
}

hipError_t launch_x2_stage3(const X2Block& b, const X2Plan& p, const X2Args& a, hipStream_t s) {
  return x2_visit_row<5, 6>(b, p, hipErrorNotSupported, [&](auto row) { return x2_stage3_go(row, a, s); });
}

}  // namespace spef
