// fp16x2 slab kernel (x2_irb_kernel, plan kind 0: the high-resolution blocks 1-7, with fp16 block I/O for the fp16mx
// schedule): the arithmetic and the kernel overview are in x2_common.hpp.
#include "spef_kernels.hpp"
#include "x2_common.hpp"

namespace spef {


// Geometry. Output tile TH x TW, NW waves; the depthwise/project phase gives wave w the output pixel tiles of group
// w % WP and the output-channel tiles of group w / WP (WCO groups; WCO > 1 repeats the depthwise to cut accumulators).
#ifndef SPEF_X2_ROWS0   // slab kernels: input rows shared between a wave's vertically adjacent pixel tiles
#define SPEF_X2_ROWS0 1   // interleaved A/B, bit-identical: blocks 5-6 117.8 -> 111.0 us per step
#endif
template <int CIN, int HID, int COUT, int S, int TH, int TW, bool EXPAND, int NW, int WCO>
struct X2Geom {
  static constexpr int IH = (TH - 1) * S + 3, IW = (TW - 1) * S + 3;
  static constexpr int PIN = IH * IW, PIN16 = (PIN + 15) / 16, PINP = PIN16 * 16;
  static constexpr int CINP = (CIN + 31) / 32 * 32;   // K of the expand (blob rows padded to 32, zeros)
  static constexpr int KS = CINP / 32;
  using SL = X2Slab<S, PINP>;
  static constexpr int NCH = (HID + 31) / 32, HIDP = NCH * 32;
  static constexpr int NCT = (COUT + 15) / 16;
  static constexpr int POUT16 = TH * TW / 16;
  static constexpr int WP = NW / WCO, QPW = POUT16 / WP, NCTW = NCT / WCO;
  static constexpr int EPT = (PIN16 + NW - 1) / NW;   // expand pixel tiles per wave
  static constexpr int DWS = 11 * HIDP;               // staged floats: depthwise [9][HIDP], bias, expand bias
  static constexpr int TRASH = EXPAND ? 16 * 24 : 0;   // dummy rows: expand stores of invalid input-tile pixels
  static constexpr int LDS_BYTES = (SL::FLOATS + DWS + TRASH) * 4;
  // waves per SIMD the LDS allows (workgroups per CU x NW / 4 SIMDs): the VGPR budget is held to it, so registers never
  // cost occupancy (the 8-wave 16 x 16 tiles: 2 workgroups per CU = 4 waves per SIMD = 128 VGPRs)
  static constexpr int WAVES_PER_EU = (163840 / LDS_BYTES) * NW / 4 > 8 ? 8 : (163840 / LDS_BYTES) * NW / 4;
  static_assert(CIN % 8 == 0 && COUT % 4 == 0 && HID % 8 == 0, "channel counts");
  static_assert(EXPAND || (CIN == HID && CIN == 32), "t == 1 blocks stage their 32-channel input as the hidden slab");
  static_assert(TH * TW % 16 == 0 && POUT16 % WP == 0 && NW % WCO == 0 && NCT % WCO == 0, "tile split");
  static_assert(EPT <= 32, "validity mask is 32 bits");
  static_assert(LDS_BYTES <= 163840, "LDS budget");
};

// IO: IO_IN16 = fp16 block input (the fp16mx schedule's early block outputs; the expand's B operand is then exact
// in fp16, two MFMAs per product), IO_OUT16 = fp16 block output. VALU per hidden value (the slab kernels are
// VALU-issue bound): the expand epilogue is one v_max (invalid input-tile pixels -- the
// depthwise's zero padding -- keep the zeros stored once at the start: their lanes store into a dummy LDS row), the
// depthwise 4.5 v_pk_fma_f32 per 9 taps, ReLU + split 1.5 (v_cvt_pk + v_fma_mix{lo,hi}). Each channel's fma chain is
// the same as with scalar fmaf, so the IO = 0 results equal the previous form bit for bit.
template <int CIN, int HID, int COUT, int S, int TH, int TW, bool EXPAND, bool RES, int NW, int WCO, int IO = 0>
__global__ __launch_bounds__(NW * 64) __attribute__((
    amdgpu_waves_per_eu(X2Geom<CIN, HID, COUT, S, TH, TW, EXPAND, NW, WCO>::WAVES_PER_EU))) void x2_irb_kernel(
    const void* __restrict__ X, const _Float16* __restrict__ We, const float* __restrict__ be,
    const float* __restrict__ Wd, const float* __restrict__ bd, const _Float16* __restrict__ Wp,
    const float* __restrict__ bp, void* __restrict__ Y, int H, int W, int OH, int OW, int tiles_x, int tiles_y,
    uint32_t nwg) {
  using G = X2Geom<CIN, HID, COUT, S, TH, TW, EXPAND, NW, WCO>;
  using SL = typename G::SL;
  constexpr bool IN16 = (IO & IO_IN16) != 0, OUT16 = (IO & IO_OUT16) != 0;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Sl = reinterpret_cast<float*>(smem);          // hidden chunk slab (plane layout)
  float* Ds = Sl + SL::FLOATS;                          // [9][HIDP] depthwise weights, [HIDP] bias, [HIDP] expand bias

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r16 = lane & 15, kg = lane >> 4;
  uint32_t L = xcd_remap(blockIdx.x, nwg);
  const int tx = (int)(L % (uint32_t)tiles_x);
  L /= (uint32_t)tiles_x;
  const int ty = (int)(L % (uint32_t)tiles_y);
  const int b = (int)(L / (uint32_t)tiles_y);
  const int oy0 = ty * TH, ox0 = tx * TW;
  const int iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;
  const size_t xb = (size_t)b * H * W * CIN;            // element offset of this image's input

  // ---- 1. staging: depthwise weights + biases of every chunk (LDS, once per workgroup); the input tile: B fragments
  // of this wave's expand pixel tiles pt = wave + NW j (fp32 input: hi / lo, split once; fp16 input: as loaded), in
  // registers for every chunk, or for t = 1 the tile itself as the slab. All global loads are issued before the first
  // LDS store.
  constexpr int NBX = EXPAND ? G::EPT : 1;
  f16x8 bxh[NBX][G::KS], bxl[IN16 ? 1 : NBX][G::KS];
  uint32_t pvmask = 0;
  int soff[NBX];                                        // slab store offset of this lane's pixel (h = 0), or Tr
  {
    constexpr int NDP = G::DWS / 4;                       // float4 pieces of the depthwise stage
    constexpr int NTP = EXPAND ? 0 : G::PINP * 8;         // t = 1: float4 pieces of the 32-channel input tile
    constexpr int NIT = (NDP + NTP + NW * 64 - 1) / (NW * 64);
    float4 v[NIT];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      int u = tid + NW * 64 * i;
      v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (u < NDP) {
        const int part = u / (G::HIDP / 4), g = u - part * (G::HIDP / 4);
        if (part < 10 || EXPAND)                          // t = 1: no be
          v[i] = *reinterpret_cast<const float4*>((part < 9 ? Wd + (size_t)part * G::HIDP : part == 9 ? bd : be) + 4 * g);
      } else if ((u -= NDP) < NTP) {
        const int p = u >> 3, g = u & 7;
        if (p < G::PIN) {
          const int py = p / G::IW, px = p - py * G::IW;
          const int iy = iy0 + py, ix = ix0 + px;
          if (iy >= 0 && iy < H && ix >= 0 && ix < W) v[i] = ld_act4(X, xb + ((size_t)iy * W + ix) * CIN + 4 * g, IN16);
        }
      }
    }
    if constexpr (EXPAND) {
      uint4 raw[G::EPT][G::KS][IN16 ? 1 : 2];
#pragma unroll
      for (int j = 0; j < G::EPT; ++j) {
        const int p = (wave + NW * j) * 16 + r16;
        bool ok = false;
        int iy = 0, ix = 0;
        if (p < G::PIN) {
          const int py = p / G::IW, px = p - py * G::IW;
          iy = iy0 + py;
          ix = ix0 + px;
          ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
        }
        if (ok) pvmask |= 1u << j;
        soff[j] = ok ? SL::at(p, kg) : SL::FLOATS + G::DWS + r16 * 24 + 4 * kg;
#pragma unroll
        for (int ks = 0; ks < G::KS; ++ks) {
          const int ch = 32 * ks + 8 * kg;
#pragma unroll
          for (int u = 0; u < (IN16 ? 1 : 2); ++u) raw[j][ks][u] = make_uint4(0u, 0u, 0u, 0u);
          if (ok && ch < CIN) {
            const size_t e0 = xb + ((size_t)iy * W + ix) * CIN + ch;
            if constexpr (IN16) {
              raw[j][ks][0] = *reinterpret_cast<const uint4*>(reinterpret_cast<const _Float16*>(X) + e0);
            } else {
              raw[j][ks][0] = *reinterpret_cast<const uint4*>(reinterpret_cast<const float*>(X) + e0);
              raw[j][ks][1] = *reinterpret_cast<const uint4*>(reinterpret_cast<const float*>(X) + e0 + 4);
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < G::EPT; ++j)
#pragma unroll
        for (int ks = 0; ks < G::KS; ++ks) {
          if constexpr (IN16) {
            bxh[j][ks] = __builtin_bit_cast(f16x8, raw[j][ks][0]);
          } else {
            const float4 a = __builtin_bit_cast(float4, raw[j][ks][0]), c = __builtin_bit_cast(float4, raw[j][ks][1]);
            const float v8[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
            split8(v8, bxh[j][ks], bxl[j][ks]);
          }
        }
      // invalid pixels (outside the image: the depthwise's zero padding) hold zeros for every chunk: stored once here,
      // never overwritten (their lanes' expand stores go to the dummy row)
#pragma unroll
      for (int j = 0; j < G::EPT; ++j) {
        const int pt = wave + NW * j;
        // (tiles past PIN16: the dummy tiles below, nothing to zero)
        if (pt < G::PIN16 && !((pvmask >> j) & 1u)) {
          const int p = pt * 16 + r16;
#pragma unroll
          for (int h = 0; h < 2; ++h)
            *reinterpret_cast<float4*>(Sl + SL::at(p, kg) + 8 * h) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      int u = tid + NW * 64 * i;
      if (u < NDP) {
        *reinterpret_cast<float4*>(Ds + 4 * u) = v[i];
      } else if ((u -= NDP) < NTP) {
        *reinterpret_cast<float4*>(Sl + SL::at(u >> 3, u & 7)) = v[i];
      }
    }
  }

  const int wp = wave % G::WP, wc = wave / G::WP;
  f32x4 acc[G::QPW][G::NCTW];
#pragma unroll
  for (int t = 0; t < G::NCTW; ++t) {
    const float4 bb = *reinterpret_cast<const float4*>(bp + (wc * G::NCTW + t) * 16 + 4 * kg);
#pragma unroll
    for (int q = 0; q < G::QPW; ++q) acc[q][t] = f32x4{bb.x, bb.y, bb.z, bb.w};
  }
  constexpr int NPC = G::NCT * 16;                      // project weight rows per plane
  const _Float16* WpLo = Wp + (size_t)NPC * G::HIDP;
  const _Float16* WeLo = We + (size_t)G::HIDP * G::CINP;
  // weight fragments of the chunk being computed, from L2; the next chunk's are issued right after their last use
  f16x8 eah[EXPAND ? 2 : 1][G::KS], eal[EXPAND ? 2 : 1][G::KS], pah[G::NCTW], pal[G::NCTW];
  auto load_ea = [&](int k) {
    if constexpr (EXPAND) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int ks = 0; ks < G::KS; ++ks) {
          const size_t off = (size_t)(32 * k + 16 * h + r16) * G::CINP + 32 * ks + 8 * kg;
          eah[h][ks] = *reinterpret_cast<const f16x8*>(We + off);
          eal[h][ks] = *reinterpret_cast<const f16x8*>(WeLo + off);
        }
    }
  };
  auto load_pa = [&](int k) {
#pragma unroll
    for (int t = 0; t < G::NCTW; ++t) {
      const size_t off = (size_t)((wc * G::NCTW + t) * 16 + r16) * G::HIDP + 32 * k + 8 * kg;
      pah[t] = *reinterpret_cast<const f16x8*>(Wp + off);
      pal[t] = *reinterpret_cast<const f16x8*>(WpLo + off);
    }
  };
  load_ea(0);
  load_pa(0);
  int pbase[G::QPW];
#pragma unroll
  for (int q = 0; q < G::QPW; ++q) {
    const int o = (wp * G::QPW + q) * 16 + r16;
    const int oy = o / TW, ox = o - (o / TW) * TW;
    pbase[q] = oy * S * G::IW + ox * S;
  }

#pragma unroll 1
  for (int c = 0; c < G::NCH; ++c) {
    __syncthreads();   // c == 0: the staged depthwise weights / t = 1 tile; c > 0: the slab of chunk c - 1 is consumed
    if constexpr (EXPAND) {
      // ---- expand chunk c: hidden channels 32c + 16h + 4kg + r of input-tile pixel 16 pt + r16 -> slab
      f32x4 e[G::EPT][2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float4 eb = *reinterpret_cast<const float4*>(Ds + 10 * G::HIDP + 32 * c + 16 * h + 4 * kg);
#pragma unroll
        for (int j = 0; j < G::EPT; ++j) e[j][h] = f32x4{eb.x, eb.y, eb.z, eb.w};
      }
#pragma unroll
      for (int ks = 0; ks < G::KS; ++ks)
#pragma unroll
        for (int j = 0; j < G::EPT; ++j) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            if constexpr (IN16)
              e[j][h] = mfma_x2w(eah[h][ks], eal[h][ks], bxh[j][ks], e[j][h]);
            else
              e[j][h] = mfma_x2(eah[h][ks], eal[h][ks], bxh[j][ks], bxl[IN16 ? 0 : j][ks], e[j][h]);
          }
        }
      if (c + 1 < G::NCH) load_ea(c + 1);
#pragma unroll
      for (int j = 0; j < G::EPT; ++j) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const float4 o = make_float4(fmaxf(e[j][h][0], 0.f), fmaxf(e[j][h][1], 0.f), fmaxf(e[j][h][2], 0.f),
                                       fmaxf(e[j][h][3], 0.f));
          *reinterpret_cast<float4*>(Sl + soff[j] + 8 * h) = o;
        }
      }
      __syncthreads();   // slab of chunk c complete
    }

    // ---- depthwise 3x3 (stride S, fp32, kx outer / ky inner) + BN + ReLU of this wave's output pixel tiles,
    // channels 32c + 8kg .. +7 -> hi / lo B fragments -> project accumulation
    f32x2 a[G::QPW][4];
    {
      const float4 d0 = *reinterpret_cast<const float4*>(Ds + 9 * G::HIDP + 32 * c + 8 * kg);
      const float4 d1 = *reinterpret_cast<const float4*>(Ds + 9 * G::HIDP + 32 * c + 8 * kg + 4);
#pragma unroll
      for (int q = 0; q < G::QPW; ++q) {
        a[q][0] = f32x2{d0.x, d0.y}; a[q][1] = f32x2{d0.z, d0.w};
        a[q][2] = f32x2{d1.x, d1.y}; a[q][3] = f32x2{d1.z, d1.w};
      }
    }
    // (blocks 5-6 only: block 3's 16 x 16 form, capped at 128 VGPRs for four waves per SIMD, spilled 30-44 VGPRs
    // with it and ran 184 -> 374 us per step in the fp16x2 schedule)
    if constexpr (SPEF_X2_ROWS0 && S == 1 && TW == 16 && G::QPW > 1 && NW == 4 && EXPAND && CIN >= 32) {
      // a wave's pixel tiles are consecutive output rows: per column, QPW + 2 input rows read once (tap (ky, q) is
      // row q + ky); same FMA order as below
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        float4 wv3[3][2], sr[G::QPW + 2][2];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          const float* wt = Ds + (ky * 3 + kx) * G::HIDP + 32 * c + 8 * kg;
          wv3[ky][0] = *reinterpret_cast<const float4*>(wt);
          wv3[ky][1] = *reinterpret_cast<const float4*>(wt + 4);
        }
#pragma unroll
        for (int r = 0; r < G::QPW + 2; ++r) {
          const int p = pbase[0] + r * G::IW + kx;
          sr[r][0] = *reinterpret_cast<const float4*>(Sl + SL::at(p, 2 * kg));
          sr[r][1] = *reinterpret_cast<const float4*>(Sl + SL::at(p, 2 * kg + 1));
        }
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          const float4 w0 = wv3[ky][0], w1 = wv3[ky][1];
          const f32x2 w4[4] = {f32x2{w0.x, w0.y}, f32x2{w0.z, w0.w}, f32x2{w1.x, w1.y}, f32x2{w1.z, w1.w}};
#pragma unroll
          for (int q = 0; q < G::QPW; ++q) dw_tap8(a[q], sr[q + ky][0], sr[q + ky][1], w4);
        }
      }
    } else {
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const float* wt = Ds + (ky * 3 + kx) * G::HIDP + 32 * c + 8 * kg;
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
#pragma unroll
    for (int t = 0; t < G::NCTW; ++t)
#pragma unroll
      for (int q = 0; q < G::QPW; ++q) acc[q][t] = mfma_x2(pah[t], pal[t], bh[q], bl[q], acc[q][t]);
    if (c + 1 < G::NCH) load_pa(c + 1);
  }

  // ---- epilogue: + residual (the block input, pytorch_layers.py:93-96, added after the BN bias) -> NHWC
#pragma unroll
  for (int q = 0; q < G::QPW; ++q) {
    const int o = (wp * G::QPW + q) * 16 + r16;
    const int oy = o / TW, ox = o - (o / TW) * TW;
    const int gy = oy0 + oy, gx = ox0 + ox;
    if (gy >= OH || gx >= OW) continue;
    const size_t pix = ((size_t)b * OH + gy) * OW + gx;
#pragma unroll
    for (int t = 0; t < G::NCTW; ++t) {
      const int co = (wc * G::NCTW + t) * 16 + 4 * kg;
      if (co >= COUT) continue;
      f32x4 v = acc[q][t];
      if constexpr (RES) {
        const float4 r = ld_act4(X, pix * CIN + co, IN16);
        v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
      }
      st_act4(Y, pix * COUT + co, v, OUT16);
    }
  }
}

template <int IO, int CIN, int HID, int COUT, int S, bool EXPAND, bool RES, int TH, int TW, int NW, int WCO, int P>
static hipError_t x2_slab_go(X2Row<CIN, HID, COUT, S, EXPAND, RES, TH, TW, NW, WCO, 0, P>, const X2Args& a,
                             hipStream_t s) {
  using G = X2Geom<CIN, HID, COUT, S, TH, TW, EXPAND, NW, WCO>;
  TileGrid g;
  hipError_t e = tile_grid(g, a.OH, a.OW, TH, TW, a.B);
  if (e != hipSuccess) return e;
  auto k = x2_irb_kernel<CIN, HID, COUT, S, TH, TW, EXPAND, RES, NW, WCO, IO>;
  static DevOnce attr_set;
  if ((e = lds_attr_once(attr_set, k, G::LDS_BYTES)) != hipSuccess) return e;
  k<<<g.nwg, NW * 64, G::LDS_BYTES, s>>>(a.x, (const _Float16*)a.we, a.be, a.wd, a.bd, (const _Float16*)a.wp, a.bp, a.y,
                                         a.H, a.W, a.OH, a.OW, g.tiles_x, g.tiles_y, g.nwg);
  return hipGetLastError();
}

// the plan's kind-0 row, one instantiation per block I/O form (a.io is 0..3: launch_x2_irb checks)
hipError_t launch_x2_slab(const X2Block& b, const X2Plan& p, const X2Args& a, hipStream_t s) {
  return x2_visit_row<0, 0>(b, p, hipErrorNotSupported, [&](auto row) {
    switch (a.io) {
      case 0: return x2_slab_go<0>(row, a, s);
      case 1: return x2_slab_go<IO_IN16>(row, a, s);
      case 2: return x2_slab_go<IO_OUT16>(row, a, s);
      default: return x2_slab_go<IO_IN16 | IO_OUT16>(row, a, s);
    }
  });
}

}  // namespace spef
