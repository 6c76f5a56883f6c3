// fp16x2 / fp16mx front kernel (x2_front_kernel); the arithmetic and the kernel overview are in x2_common.hpp.
#include "spef_kernels.hpp"
#include "x2_common.hpp"

namespace spef {

// ------------------------------------------------------------------------------------------ front: stem + block 1
// uint8 NHWC frames -> stem ConvBnAct 3 -> 32, 3x3 / 2 (mobilenet_v2.py:252-254; ToTensor's /255 folded into the
// weights) -> block 1 (depthwise 3x3 + project 32 -> 16, pytorch_layers.py:65-98) -> fp32 block-1 output, one kernel:
// the 32-channel stem map (8.4 MB/img at 512^2 in fp32) never reaches HBM. A u8 pixel is exact in fp16, so the stem is
// two MFMAs per product (W_hi x + W_lo x, the blob's split /255-folded operand x0). Its K runs over the 3 input rows
// of the stencil, one K step per row ky with k = 4 kx + ci (ci padded to 4; k >= 12 zero), so a lane's B fragment is
// one 16-B (kg 0) or 8-B (kg 1) LDS read of the staged input tile [row][col][4] (fp16). The stem map of the output
// tile + halo goes to the fp32 slab (zero outside the image: the depthwise's padding), then block 1 runs as in
// x2_irb_kernel.
template <int TH, int TW, int NW_ = 4>
struct X2FrontGeom {
  static constexpr int NW = NW_;
  static constexpr int PH = TH + 2, PW = TW + 2;        // stem pixels of the tile (+ block-1 halo)
  static constexpr int PIN = PH * PW, PIN16 = (PIN + 15) / 16, PINP = PIN16 * 16;
  static constexpr int IRW = 2 * PH + 1, ICL = 2 * PW + 1;   // input rows / columns of the stem stencil
  static constexpr int ICS = (ICL * 4 + 8 + 7) / 8 * 8;   // halves per staged input row (16-B rows; zero tail)
  using SL = X2Slab<1, PINP>;
  static constexpr int POUT16 = TH * TW / 16, QPW = POUT16 / NW;
  static constexpr int EPT = (PIN16 + NW - 1) / NW;
  static constexpr int XI_H = (IRW * ICS + 7) / 8 * 8;   // staged input (halves)
  static constexpr int DWS = 9 * 32 + 32;               // block-1 depthwise weights + bias (floats)
  static constexpr int TRASH = 16 * 24;                 // dummy rows: stem stores of pixels outside the stem map
  static constexpr int LDS_BYTES = XI_H * 2 + (SL::FLOATS + DWS + TRASH) * 4;
  static_assert(TW == 16 && POUT16 % NW == 0 && EPT <= 32, "front tile");
};

template <int TH, int TW, int NW_ = 4, bool OUT16 = false>
__global__ __launch_bounds__(NW_ * 64) __attribute__((amdgpu_waves_per_eu(NW_ == 4 ? 3 : 4, 8))) void x2_front_kernel(
    const uint8_t* __restrict__ X, const _Float16* __restrict__ Wsx, const float* __restrict__ bs,
    const float* __restrict__ Wd, const float* __restrict__ bd, const _Float16* __restrict__ Wp,
    const float* __restrict__ bp, void* __restrict__ Y, int H, int W, int OH, int OW, int tiles_x, int tiles_y,
    uint32_t nwg) {
  using G = X2FrontGeom<TH, TW, NW_>;
  using SL = typename G::SL;
  constexpr int NW = G::NW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  _Float16* Xi = reinterpret_cast<_Float16*>(smem);                     // [IRW][ICS] input tile, fp16
  float* Sl = reinterpret_cast<float*>(smem + G::XI_H * 2);             // stem map of the tile (+halo), plane layout
  float* Ds = Sl + SL::FLOATS;                                          // [9][32] depthwise weights, [32] bias

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r16 = lane & 15, kg = lane >> 4;
  uint32_t L = xcd_remap(blockIdx.x, nwg);
  const int tx = (int)(L % (uint32_t)tiles_x);
  L /= (uint32_t)tiles_x;
  const int ty = (int)(L % (uint32_t)tiles_y);
  const int b = (int)(L / (uint32_t)tiles_y);
  const int oy0 = ty * TH, ox0 = tx * TW;
  const int sy0 = oy0 - 1, sx0 = ox0 - 1;              // stem pixel of tile position (0, 0)
  const int iy0 = 2 * sy0 - 1, ix0 = 2 * sx0 - 1;      // input pixel of staged position (0, 0)

  // ---- staging: the input rows of the stencil as aligned dword loads (a row segment is 3 ICL bytes at any byte
  // alignment), bytes scattered to fp16 [row][col][4] over a zero-filled tile (zero outside the frame: the stem's
  // padding; the ci = 3 pad); block-1 depthwise weights + bias
  // Interior tiles (every staged row and column inside the frame, 4-byte aligned rows): the row's dwords load one per
  // lane, and lane c builds stem pixel column c from two of them (two lane shuffles + one v_alignbyte), converts the
  // three bytes exactly to fp16 (0x6400 | byte = 1024 + byte, minus 1024) and writes its 4 halves with one 8-B store.
  const bool fast = (W & 3) == 0 && ix0 >= 0 && ix0 + G::ICL <= W && iy0 >= 0 && iy0 + G::IRW <= H;
  if (fast) {
    constexpr int RPW = (G::IRW + NW - 1) / NW;
    static_assert(G::ICL <= 64 && (3 * G::ICL + 3 + 3) / 4 < 64, "one row per wave");
    const int off = (3 * ix0) & 3;                      // rows start `off` bytes into their dword (W % 4 == 0)
    const int nl = (off + 3 * G::ICL + 3) / 4;          // dwords holding the row segment
    const uint8_t* Xb = X + (size_t)b * H * W * 3;
    uint32_t v[RPW];
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const int r = wave + NW * i;
      v[i] = 0;
      if (r < G::IRW && lane < nl)
        v[i] = *reinterpret_cast<const uint32_t*>(Xb + (((size_t)(iy0 + r) * W + ix0) * 3 - off) + 4 * lane);
    }
    float4 dwv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int u = tid + NW * 64 * i;   // 72 pieces of the [9][32] weights, 8 of the bias
      dwv[i] = u < 72 ? *reinterpret_cast<const float4*>(Wd + 4 * u)
                      : u < 80 ? *reinterpret_cast<const float4*>(bd + 4 * (u - 72)) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const int q = 3 * lane + off, d = q >> 2, sh = q & 3;   // lane c = pixel column c: segment bytes q .. q + 2
    const f16x2 k1024 = {(_Float16)1024.0f, (_Float16)1024.0f};
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const int r = wave + NW * i;
      const uint32_t lo = __shfl(v[i], d, 64), hi = __shfl(v[i], d + 1 < 64 ? d + 1 : 63, 64);
      if (r < G::IRW && lane < G::ICL) {
        const uint32_t by = __builtin_amdgcn_alignbyte(hi, lo, sh);   // bytes ci 0, 1, 2 of the pixel
        const f16x2 h01 = __builtin_bit_cast(f16x2, __builtin_amdgcn_perm(0u, by, 0x0c010c00u) | 0x64006400u) - k1024;
        const f16x2 h2 = __builtin_bit_cast(f16x2, __builtin_amdgcn_perm(0u, by, 0x0c0c0c02u) | 0x64006400u) - k1024;
        *reinterpret_cast<uint2*>(Xi + r * G::ICS + 4 * lane) =
            make_uint2(__builtin_bit_cast(uint32_t, h01), __builtin_bit_cast(uint32_t, h2));
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int u = tid + NW * 64 * i;
      if (u < 80) *reinterpret_cast<float4*>(Ds + 4 * u) = dwv[i];
    }
  } else {
    constexpr int NDW = (3 * G::ICL + 3 + 3) / 4 + 1;   // dwords covering one row segment at any alignment
    constexpr int NPC = G::IRW * NDW;
    constexpr int NIT = (NPC + NW * 64 - 1) / (NW * 64);
    constexpr int NZ = G::XI_H / 8;                     // 16-B pieces of the staged tile
    const size_t img = (size_t)b * H * W * 3;
    uint32_t v[NIT];
    bool ld[NIT];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int u = tid + NW * 64 * i;
      const int r = u / NDW, j = u - r * NDW;
      const int iy = iy0 + r;
      v[i] = 0;
      ld[i] = false;
      if (u < NPC && iy >= 0 && iy < H) {
        const int64_t rb = (int64_t)(img + (size_t)iy * W * 3);
        const int64_t vs = rb + 3 * (int64_t)(ix0 > 0 ? ix0 : 0);
        const int64_t ve = rb + 3 * (int64_t)(ix0 + G::ICL < W ? ix0 + G::ICL : W);
        const int64_t a = ((rb + 3 * (int64_t)ix0) & ~(int64_t)3) + 4 * j;   // may start left of the frame row
        if (a + 4 > vs && a < ve) {
          v[i] = *reinterpret_cast<const uint32_t*>(X + a);
          ld[i] = true;
        }
      }
    }
    float4 dwv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int u = tid + NW * 64 * i;   // 72 pieces of the [9][32] weights, 8 of the bias
      dwv[i] = u < 72 ? *reinterpret_cast<const float4*>(Wd + 4 * u)
                      : u < 80 ? *reinterpret_cast<const float4*>(bd + 4 * (u - 72)) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int u = tid; u < NZ; u += NW * 64) reinterpret_cast<uint4*>(Xi)[u] = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int u = tid + NW * 64 * i;
      if (u < 80) *reinterpret_cast<float4*>(Ds + 4 * u) = dwv[i];
    }
    __syncthreads();
    // dword j's first byte is segment byte 4 j - off (off = the segment start's offset in its dword); valid bytes:
    // segment bytes [rlo, rhi), the frame row's part of the segment
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      if (!ld[i]) continue;
      const int u = tid + NW * 64 * i;
      const int r = u / NDW, j = u - r * NDW;
      const int64_t rb = (int64_t)(img + (size_t)(iy0 + r) * W * 3);
      const int off = (int)((rb + 3 * (int64_t)ix0) & 3);      // segment start within its dword
      const int rlo = ix0 < 0 ? -3 * ix0 : 0, rhi = 3 * ((ix0 + G::ICL < W ? ix0 + G::ICL : W) - ix0);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int rel = 4 * j + k - off;   // byte of the segment: column rel / 3, channel rel % 3
        if (rel < rlo || rel >= rhi) continue;
        Xi[r * G::ICS + 4 * (rel / 3) + rel % 3] = (_Float16)(float)((v[i] >> (8 * k)) & 0xffu);
      }
    }
  }
  // stem A fragments for the 3 K steps (ky) and 2 channel halves: lane (r16 = output channel, kg) holds k = 8kg + e,
  // k = 4 kx + ci. The blob's x0 is already in this order: [2 planes][3 ky][32 ch][32 k] (spef_blob.hpp).
  auto stem_a = [&](int h, int ky, f16x8& ah, f16x8& al) {
    const int off = (ky * 32 + 16 * h + r16) * 32 + 8 * kg;
    ah = *reinterpret_cast<const f16x8*>(Wsx + off);
    al = *reinterpret_cast<const f16x8*>(Wsx + 3 * 32 * 32 + off);
  };
  float sb[2][4];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float4 t = *reinterpret_cast<const float4*>(bs + 16 * h + 4 * kg);
    sb[h][0] = t.x; sb[h][1] = t.y; sb[h][2] = t.z; sb[h][3] = t.w;
  }
  __syncthreads();

  // ---- stem of the tile's stem pixels p = 16 pt + r16 -> slab (ReLU; zero outside the stem map); K steps (ky)
  // outermost so one (ky, half) A fragment pair is live at a time
  {
    f32x4 e[G::EPT][2];
    int xo[G::EPT], soff[G::EPT];
#pragma unroll
    for (int j = 0; j < G::EPT; ++j) {
      const int p = (wave + NW * j) * 16 + r16;
      const int pc = p < G::PIN ? p : G::PIN - 1;
      const int py = pc / G::PW, px = pc - (pc / G::PW) * G::PW;
      const int sy = sy0 + py, sx = sx0 + px;
      const bool ok = p < G::PIN && sy >= 0 && sy < OH && sx >= 0 && sx < OW;
      // pixels outside the stem map (the depthwise's zero padding) get zeros once; their stem results go to a dummy row
      soff[j] = ok ? SL::at(p, kg) : SL::FLOATS + G::DWS + r16 * 24 + 4 * kg;
      if (!ok && p < G::PIN) {
        *reinterpret_cast<float4*>(Sl + SL::at(p, kg)) = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(Sl + SL::at(p, kg) + 8) = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      xo[j] = 2 * py * G::ICS + 8 * px + (kg == 1 ? 8 : 0);   // stem pixel px reads input cols 2px .. 2px + 2
#pragma unroll
      for (int h = 0; h < 2; ++h) e[j][h] = f32x4{sb[h][0], sb[h][1], sb[h][2], sb[h][3]};
    }
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      f16x8 bx[G::EPT];
#pragma unroll
      for (int j = 0; j < G::EPT; ++j) {
        const _Float16* xr = Xi + xo[j] + ky * G::ICS;
        if (kg == 0) {
          bx[j] = *reinterpret_cast<const f16x8*>(xr);
        } else if (kg == 1) {
          const uint2 t = *reinterpret_cast<const uint2*>(xr);
          bx[j] = __builtin_bit_cast(f16x8, make_uint4(t.x, t.y, 0u, 0u));
        } else {
          bx[j] = __builtin_bit_cast(f16x8, make_uint4(0u, 0u, 0u, 0u));
        }
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        f16x8 ah, al;
        stem_a(h, ky, ah, al);
#pragma unroll
        for (int j = 0; j < G::EPT; ++j) {
          e[j][h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bx[j], e[j][h], 0, 0, 0);
          e[j][h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bx[j], e[j][h], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < G::EPT; ++j) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
        *reinterpret_cast<float4*>(Sl + soff[j] + 8 * h) = make_float4(
            fmaxf(e[j][h][0], 0.f), fmaxf(e[j][h][1], 0.f), fmaxf(e[j][h][2], 0.f), fmaxf(e[j][h][3], 0.f));
    }
  }
  __syncthreads();

  // ---- block 1: depthwise 3x3 (fp32, kx outer / ky inner) + BN + ReLU -> hi / lo -> project 32 -> 16
  f32x2 a[G::QPW][4];
  int pbase[G::QPW];
  {
    const float4 d0 = *reinterpret_cast<const float4*>(Ds + 288 + 8 * kg);
    const float4 d1 = *reinterpret_cast<const float4*>(Ds + 288 + 8 * kg + 4);
#pragma unroll
    for (int q = 0; q < G::QPW; ++q) {
      a[q][0] = f32x2{d0.x, d0.y}; a[q][1] = f32x2{d0.z, d0.w};
      a[q][2] = f32x2{d1.x, d1.y}; a[q][3] = f32x2{d1.z, d1.w};
      const int o = (wave * G::QPW + q) * 16 + r16;
      pbase[q] = (o / TW) * G::PW + (o % TW);
    }
  }
#pragma unroll 1   // (one kernel column in flight: fully unrolled, the 36 tap loads hoist and cost an occupancy step)
  for (int kx = 0; kx < 3; ++kx)
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const float* wt = Ds + (ky * 3 + kx) * 32 + 8 * kg;
      const float4 w0 = *reinterpret_cast<const float4*>(wt), w1 = *reinterpret_cast<const float4*>(wt + 4);
      const f32x2 w4[4] = {f32x2{w0.x, w0.y}, f32x2{w0.z, w0.w}, f32x2{w1.x, w1.y}, f32x2{w1.z, w1.w}};
#pragma unroll
      for (int q = 0; q < G::QPW; ++q) {
        const int p = pbase[q] + ky * G::PW + kx;
        dw_tap8(a[q], *reinterpret_cast<const float4*>(Sl + SL::at(p, 2 * kg)),
                *reinterpret_cast<const float4*>(Sl + SL::at(p, 2 * kg + 1)), w4);
      }
    }
  const f16x8 ph = *reinterpret_cast<const f16x8*>(Wp + r16 * 32 + 8 * kg);
  const f16x8 pl = *reinterpret_cast<const f16x8*>(Wp + 16 * 32 + r16 * 32 + 8 * kg);
  const float4 bb = *reinterpret_cast<const float4*>(bp + 4 * kg);
#pragma unroll
  for (int q = 0; q < G::QPW; ++q) {
    f16x8 bh, bl;
    relu_split8(a[q], bh, bl);
    const f32x4 v = mfma_x2(ph, pl, bh, bl, f32x4{bb.x, bb.y, bb.z, bb.w});
    const int o = (wave * G::QPW + q) * 16 + r16;
    const int gy = oy0 + o / TW, gx = ox0 + o % TW;
    if (gy < OH && gx < OW) st_act4(Y, (((size_t)b * OH + gy) * OW + gx) * 16 + 4 * kg, v, OUT16);
  }
}

#ifndef SPEF_X2_FRONT_TH
#define SPEF_X2_FRONT_TH 16
#define SPEF_X2_FRONT_NW 8
#endif
template <bool OUT16>
static hipError_t x2_front_go(const void* x, const void* wsx, const float* bs, const float* wd, const float* bd,
                              const void* wp, const float* bp, void* y, int B, int H, int W, int OH, int OW,
                              hipStream_t s) {
  constexpr int TH = SPEF_X2_FRONT_TH, TW = 16, NW = SPEF_X2_FRONT_NW;
  using G = X2FrontGeom<TH, TW, NW>;
  if (!x || !wsx || !bs || !wd || !bd || !wp || !bp || !y) return hipErrorInvalidValue;
  TileGrid g;
  hipError_t e = tile_grid(g, OH, OW, TH, TW, B);
  if (e != hipSuccess) return e;
  static DevOnce attr_set;
  if ((e = lds_attr_once(attr_set, x2_front_kernel<TH, TW, NW, OUT16>, G::LDS_BYTES)) != hipSuccess) return e;
  x2_front_kernel<TH, TW, NW, OUT16><<<g.nwg, NW * 64, G::LDS_BYTES, s>>>((const uint8_t*)x, (const _Float16*)wsx, bs,
                                                                        wd, bd, (const _Float16*)wp, bp, y, H, W, OH,
                                                                        OW, g.tiles_x, g.tiles_y, g.nwg);
  return hipGetLastError();
}
hipError_t launch_x2_front(const void* x, const void* wsx, const float* bs, const float* wd, const float* bd,
                           const void* wp, const float* bp, void* y, int B, int H, int W, int OH, int OW,
                           hipStream_t s, bool out16) {
  return out16 ? x2_front_go<true>(x, wsx, bs, wd, bd, wp, bp, y, B, H, W, OH, OW, s)
               : x2_front_go<false>(x, wsx, bs, wd, bd, wp, bp, y, B, H, W, OH, OW, s);
}

}  // namespace spef
