// fp16x2 / fp16mx last conv (x2_pw_kernel, x2_pws_kernel) with its pooled form; the arithmetic and the kernel overview
// are in x2_common.hpp.
#include "spef_kernels.hpp"
#include "x2_common.hpp"

namespace spef {

// ------------------------------------------------------------------------------------------ 1x1 conv, fp32 I/O
// C^T = W X^T as pw_kernel: a wave owns NT output-channel tiles x MT pixel tiles; 4 waves on 64 MT consecutive
// pixels; channel chunks fastest-varying so one pixel block's chunks share an XCD L2. B fragments: 8 fp32 values
// per lane from HBM / L2, split once and used by all NT channel tiles. POOL (URSONetHead's x.mean([2,3]),
// ursonet.py:30, when HW % 64 == 0): the 1280-channel map is never stored -- each wave sums the ReLU'd outputs of its
// 64 pixels (one image) over its pixel tiles and then over the 16 pixel lanes (xor shuffles, fixed order) into
// Y = partial [M / 64][N]; x2_pool_reduce_kernel adds an image's partials in order and divides by HW.
template <int NT, int MT, bool POOL>
__global__ __launch_bounds__(256) void x2_pw_kernel(const float* __restrict__ X, const _Float16* __restrict__ Wt,
                                                    const float* __restrict__ bias, float* __restrict__ Y, int64_t M,
                                                    int K, int N, int Np, int Kp, int n_chunks, uint32_t nwg) {
  const uint32_t L = xcd_remap(blockIdx.x, nwg);
  const int chunk = (int)(L % (uint32_t)n_chunks);
  const int64_t ptile = L / (uint32_t)n_chunks;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r16 = lane & 15, kg = lane >> 4;
  const int n0 = chunk * 16 * NT;
  const int64_t m0 = ptile * (64 * MT) + (int64_t)wave * 16 * MT;
  const _Float16* Wlo = Wt + (size_t)Np * Kp;
  f32x4 acc[NT][MT];
#pragma unroll
  for (int a = 0; a < NT; ++a) {
    const float4 bb = *reinterpret_cast<const float4*>(bias + n0 + 16 * a + 4 * kg);
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[a][m] = f32x4{bb.x, bb.y, bb.z, bb.w};
  }
  const float* xp[MT];
  bool mv[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int64_t p = m0 + 16 * m + r16;
    mv[m] = p < M;
    xp[m] = X + (size_t)(mv[m] ? p : 0) * K + 8 * kg;
  }
#pragma unroll 1
  for (int k0 = 0; k0 < Kp; k0 += 32) {
    const bool kv = k0 + 8 * kg < K;   // K % 8 == 0: a lane's 8 k are all in range or all out
    f16x8 bh[MT], bl[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (kv && mv[m]) {
        const float4 u0 = *reinterpret_cast<const float4*>(xp[m] + k0);
        const float4 u1 = *reinterpret_cast<const float4*>(xp[m] + k0 + 4);
        v[0] = u0.x; v[1] = u0.y; v[2] = u0.z; v[3] = u0.w; v[4] = u1.x; v[5] = u1.y; v[6] = u1.z; v[7] = u1.w;
      }
      split8(v, bh[m], bl[m]);
    }
#pragma unroll
    for (int a = 0; a < NT; ++a) {
      const size_t off = (size_t)(n0 + 16 * a + r16) * Kp + k0 + 8 * kg;
      const f16x8 ah = *reinterpret_cast<const f16x8*>(Wt + off);
      const f16x8 al = *reinterpret_cast<const f16x8*>(Wlo + off);
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[a][m] = mfma_x2(ah, al, bh[m], bl[m], acc[a][m]);
    }
  }
  if constexpr (POOL) {   // MT = 4: the wave's 64 pixels m0 .. m0 + 63, all valid when m0 < M (M % 64 == 0)
#pragma unroll
    for (int a = 0; a < NT; ++a) {
      float sm[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float t = 0.f;
#pragma unroll
        for (int m = 0; m < MT; ++m) t += fmaxf(acc[a][m][r], 0.f);
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) t += __shfl_xor(t, o, 64);
        sm[r] = t;
      }
      const int i = n0 + 16 * a + 4 * kg;
      if (r16 == 0 && i < N && m0 < M)   // (a workgroup's last waves may lie past M: no partial for them)
        *reinterpret_cast<float4*>(Y + (size_t)(m0 / 64) * N + i) = make_float4(sm[0], sm[1], sm[2], sm[3]);
    }
    return;
  }
#pragma unroll
  for (int a = 0; a < NT; ++a) {
    const int i = n0 + 16 * a + 4 * kg;
    if (i >= N) continue;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int64_t p = m0 + 16 * m + r16;
      if (p >= M) continue;
      const f32x4 v = acc[a][m];
      *reinterpret_cast<float4*>(Y + (size_t)p * N + i) =
          make_float4(fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f));
    }
  }
}

// Staged form (the last conv, K = 320): 64 pixels x 256 output channels per workgroup. The 64 x K fp32 input block is
// split into hi / lo fp16 once per workgroup and staged in LDS (80 KB at K = 320: two workgroups per CU), instead of
// once per wave and 64-channel chunk from L2 as above (4x the split VALU and 4x the activation reads); the four waves
// take 64 channels each and stream their hi / lo weight fragments from L2 one K step ahead. Same products, same
// accumulation order, same pool partials as x2_pw_kernel<4, 4, POOL> (bit-identical). LDS rows of Kp halves with the
// 16-B granule index XOR-ed by (row & 7): the 8 rows a ds_read_b128 lane group reads hit disjoint banks.
#ifndef SPEF_X2_PWS
#define SPEF_X2_PWS 1
#endif
// Waves (64 output channels each) per workgroup. 5: 1280 / 320 = 4 channel chunks, 1024 workgroups at B = 64 (two
// full rounds at two per CU instead of 2.5) -- measured 64 -> 71 us per step (ten waves per CU load the four SIMDs
// 3 / 3 / 2 / 2): kept at 4.
#ifndef SPEF_X2_PWS_NWV
#define SPEF_X2_PWS_NWV 4
#endif
template <bool POOL, int NWV = 4>
__global__ __launch_bounds__(NWV * 64) void x2_pws_kernel(const float* __restrict__ X, const _Float16* __restrict__ Wt,
                                                     const float* __restrict__ bias, float* __restrict__ Y, int64_t M,
                                                     int K, int N, int Np, int Kp, int n_chunks, uint32_t nwg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  _Float16* Xh = reinterpret_cast<_Float16*>(smem);   // [64][Kp] hi halves (swizzled granules)
  _Float16* Xl = Xh + 64 * Kp;                         // [64][Kp] lo halves
  const uint32_t L = xcd_remap(blockIdx.x, nwg);
  const int chunk = (int)(L % (uint32_t)n_chunks);
  const int64_t m0 = (int64_t)(L / (uint32_t)n_chunks) * 64;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r16 = lane & 15, kg = lane >> 4;
  const int n0 = chunk * (64 * NWV) + wave * 64;
  const _Float16* Wlo = Wt + (size_t)Np * Kp;
  // ---- stage: 64 rows x Kp / 8 granules, 8 fp32 -> hi / lo per piece (batches of 5 pieces per thread, loads first)
  {
    const int GP = Kp >> 3, NP = 64 * GP;
    for (int u0 = 0; u0 < NP; u0 += NWV * 64 * 5) {
      float4 v[5][2];
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const int u = u0 + tid + NWV * 64 * i;
        const int px = u / GP, g = u - px * GP;
        const int64_t p = m0 + px;
        v[i][0] = v[i][1] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (u < NP && p < M && 8 * g < K) {
          const float* xp = X + (size_t)p * K + 8 * g;
          v[i][0] = *reinterpret_cast<const float4*>(xp);
          v[i][1] = *reinterpret_cast<const float4*>(xp + 4);
        }
      }
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const int u = u0 + tid + NWV * 64 * i;
        if (u >= NP) break;
        const int px = u / GP, g = u - px * GP;
        const float f[8] = {v[i][0].x, v[i][0].y, v[i][0].z, v[i][0].w, v[i][1].x, v[i][1].y, v[i][1].z, v[i][1].w};
        f16x8 hi, lo;
        split8(f, hi, lo);
        const int o = px * Kp + 8 * (g ^ (px & 7));
        *reinterpret_cast<f16x8*>(Xh + o) = hi;
        *reinterpret_cast<f16x8*>(Xl + o) = lo;
      }
    }
  }
  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const float4 bb = *reinterpret_cast<const float4*>(bias + n0 + 16 * a + 4 * kg);
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[a][m] = f32x4{bb.x, bb.y, bb.z, bb.w};
  }
  f16x8 ah[4], al[4];
  auto load_a = [&](int k0) {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const size_t off = (size_t)(n0 + 16 * a + r16) * Kp + k0 + 8 * kg;
      ah[a] = *reinterpret_cast<const f16x8*>(Wt + off);
      al[a] = *reinterpret_cast<const f16x8*>(Wlo + off);
    }
  };
  load_a(0);
  __syncthreads();
#pragma unroll 1
  for (int k0 = 0; k0 < Kp; k0 += 32) {
    f16x8 bh[4], bl[4];
    const int g = (k0 >> 3) + kg;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int px = 16 * m + r16;
      const int o = px * Kp + 8 * (g ^ (px & 7));
      bh[m] = *reinterpret_cast<const f16x8*>(Xh + o);
      bl[m] = *reinterpret_cast<const f16x8*>(Xl + o);
    }
    f16x8 ch[4], cl[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      ch[a] = ah[a];
      cl[a] = al[a];
    }
    if (k0 + 32 < Kp) load_a(k0 + 32);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int m = 0; m < 4; ++m) acc[a][m] = mfma_x2(ch[a], cl[a], bh[m], bl[m], acc[a][m]);
  }
  if constexpr (POOL) {   // the 64 pixels m0 .. m0 + 63, all valid (M % 64 == 0)
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      float sm[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float t = 0.f;
#pragma unroll
        for (int m = 0; m < 4; ++m) t += fmaxf(acc[a][m][r], 0.f);
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) t += __shfl_xor(t, o, 64);
        sm[r] = t;
      }
      const int i = n0 + 16 * a + 4 * kg;
      if (r16 == 0 && i < N && m0 < M)   // (a workgroup's last waves may lie past M: no partial for them)
        *reinterpret_cast<float4*>(Y + (size_t)(m0 / 64) * N + i) = make_float4(sm[0], sm[1], sm[2], sm[3]);
    }
    return;
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = n0 + 16 * a + 4 * kg;
    if (i >= N) continue;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int64_t p = m0 + 16 * m + r16;
      if (p >= M) continue;
      const f32x4 v = acc[a][m];
      *reinterpret_cast<float4*>(Y + (size_t)p * N + i) =
          make_float4(fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f));
    }
  }
}

// Wide form of the staged kernel (SPEF_OPT_TRIM bit 0; Kp = 320, Np % 320 == 0): 128 pixels x 320 output channels per
// workgroup, each of the four waves 80 channels (5 tiles) x 128 pixels (8 tiles): 160 accumulator registers. A weight
// fragment now serves 8 pixel tiles instead of 4 and a staged pixel block 320 channels instead of 256: per launch at
// B = 64, 512^2 the workgroups read 210 MB of weights and 84 MB of activations from L2 (the 64 x 256 form: 420 + 105),
// and the 512 workgroups are one full round at two per CU (1,280 were 2.5). The pixel block is staged in two K halves of
// 160 (128 x 160 x (hi + lo) = 80 KB, the 64-pixel form's LDS size: still two workgroups per CU, 250-252 VGPRs with no
// scratch at two waves per SIMD). Every accumulator tile sees the same three MFMAs per K step in the same K order from the same
// bias, and each 64-pixel group's pool partial is the same sum (its four pixel tiles in order from 0.f, then the xor
// shuffles), written to the same [M / 64][N] rows: bit-identical to the 64-pixel form. LDS rows of 160 halves (320 B:
// rows four apart start on the same bank); the 16-B granule index is XOR-ed within its group of four by
// (-(row / 4)) & 3, which makes the 16 lanes of every ds_read_b128 lane group (rows 0-3 and 12-15 of one k group, rows
// 4-11 of its neighbour) cover the 64 banks once.
struct X2PwsWide {
  static constexpr int PT = 128, MT = PT / 16;   // pixels, pixel tiles per workgroup (and per wave)
  static constexpr int NA = 5, NC = 4 * 16 * NA;   // channel tiles per wave, channels per workgroup
  static constexpr int KP = 320, KH = KP / 2, GP = KH / 8;   // K, the staged K half, its 16-B granules per row
  static constexpr int LDS_BYTES = PT * KH * 2 * (int)sizeof(_Float16);
};
template <bool POOL, typename T>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void x2_pws_kernel(const float* __restrict__ X, const _Float16* __restrict__ Wt, const float* __restrict__ bias,
                   float* __restrict__ Y, int64_t M, int K, int N, int Np, int n_chunks, uint32_t nwg) {
  constexpr int KP = T::KP, KH = T::KH, GP = T::GP, NA = T::NA, MT = T::MT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  _Float16* Xh = reinterpret_cast<_Float16*>(smem);   // [128][KH] hi halves of the staged K half (swizzled granules)
  _Float16* Xl = Xh + T::PT * KH;                      // [128][KH] lo halves
  const uint32_t L = xcd_remap(blockIdx.x, nwg);
  const int chunk = (int)(L % (uint32_t)n_chunks);
  const int64_t m0 = (int64_t)(L / (uint32_t)n_chunks) * T::PT;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r16 = lane & 15, kg = lane >> 4;
  const int n0 = chunk * T::NC + wave * (16 * NA);
  const _Float16* Wlo = Wt + (size_t)Np * KP;
  f32x4 acc[NA][MT];
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    const float4 bb = *reinterpret_cast<const float4*>(bias + n0 + 16 * a + 4 * kg);
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[a][m] = f32x4{bb.x, bb.y, bb.z, bb.w};
  }
  f16x8 ah[NA], al[NA];
  const _Float16* wrow = Wt + (size_t)(n0 + r16) * KP + 8 * kg;
  auto load_a = [&](int k) {
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      ah[a] = *reinterpret_cast<const f16x8*>(wrow + 16 * a * KP + k);
      al[a] = *reinterpret_cast<const f16x8*>(wrow + (Wlo - Wt) + 16 * a * KP + k);
    }
  };
  const int boff = r16 * KH + 8 * (kg ^ ((0 - (r16 >> 2)) & 3));   // the lane's granule of pixel tile 0, K step 0
#pragma unroll 1
  for (int kb = 0; kb < KP; kb += KH) {
    if (kb) __syncthreads();   // the first half's fragment reads done before the second overlays it
    // ---- stage: thread (row tid / 4, granule tid % 4 + 4 j) of rows 0-63, then of rows 64-127: 8 fp32 -> hi / lo per
    // piece, a row's five loads first (four lanes read one 128-B line; the two rows of an 8-lane ds_write_b128 group
    // cover the 32 banks once)
#pragma unroll 1
    for (int h = 0; h < T::PT / 64; ++h) {
      const int px = 64 * h + (tid >> 2), q = tid & 3;
      const int64_t p = m0 + px;
      const float* xp = X + (size_t)(p < M ? p : 0) * K + kb + 8 * q;
      float4 v[GP / 4][2];
#pragma unroll
      for (int j = 0; j < GP / 4; ++j) {
        v[j][0] = v[j][1] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p < M && kb + 8 * q + 32 * j < K) {
          v[j][0] = *reinterpret_cast<const float4*>(xp + 32 * j);
          v[j][1] = *reinterpret_cast<const float4*>(xp + 32 * j + 4);
        }
      }
      const int o = px * KH + 8 * (q ^ ((0 - (px >> 2)) & 3));
#pragma unroll
      for (int j = 0; j < GP / 4; ++j) {
        const float f[8] = {v[j][0].x, v[j][0].y, v[j][0].z, v[j][0].w, v[j][1].x, v[j][1].y, v[j][1].z, v[j][1].w};
        f16x8 hi, lo;
        split8(f, hi, lo);
        *reinterpret_cast<f16x8*>(Xh + o + 32 * j) = hi;
        *reinterpret_cast<f16x8*>(Xl + o + 32 * j) = lo;
      }
    }
    load_a(kb);
    __syncthreads();
#pragma unroll 1
    for (int k0 = 0; k0 < KH; k0 += 32) {
      f16x8 bh[2], bl[2];   // pixel tile m + 1's fragments are read while tile m's MFMAs run
      bh[0] = *reinterpret_cast<const f16x8*>(Xh + boff + k0);
      bl[0] = *reinterpret_cast<const f16x8*>(Xl + boff + k0);
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        if (m + 1 < MT) {
          const int o = boff + 16 * (m + 1) * KH + k0;
          bh[(m + 1) & 1] = *reinterpret_cast<const f16x8*>(Xh + o);
          bl[(m + 1) & 1] = *reinterpret_cast<const f16x8*>(Xl + o);
        }
#pragma unroll
        for (int a = 0; a < NA; ++a) acc[a][m] = mfma_x2(ah[a], al[a], bh[m & 1], bl[m & 1], acc[a][m]);
      }
      if (k0 + 32 < KH) load_a(kb + k0 + 32);
    }
  }
  if constexpr (POOL) {   // two 64-pixel groups m0 + 64 h .. + 63, each all valid when it starts below M (M % 64 == 0)
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const int i = n0 + 16 * a + 4 * kg;
#pragma unroll
      for (int h = 0; h < MT / 4; ++h) {
        float sm[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float t = 0.f;
#pragma unroll
          for (int m = 4 * h; m < 4 * h + 4; ++m) t += fmaxf(acc[a][m][r], 0.f);
#pragma unroll
          for (int o = 1; o < 16; o <<= 1) t += __shfl_xor(t, o, 64);
          sm[r] = t;
        }
        if (r16 == 0 && i < N && m0 + 64 * h < M)
          *reinterpret_cast<float4*>(Y + (size_t)(m0 / 64 + h) * N + i) = make_float4(sm[0], sm[1], sm[2], sm[3]);
      }
    }
    return;
  }
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    const int i = n0 + 16 * a + 4 * kg;
    if (i >= N) continue;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int64_t p = m0 + 16 * m + r16;
      if (p >= M) continue;
      const f32x4 v = acc[a][m];
      *reinterpret_cast<float4*>(Y + (size_t)p * N + i) =
          make_float4(fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f));
    }
  }
}

static bool x2_pws_ok(int Kp, int Np) {
  return SPEF_X2_PWS && Kp % 64 == 0 && Kp <= 320 && Np % 256 == 0;   // (NWV 5 falls back to 4 unless Np % 320 == 0)
}
static bool x2_pws_wide_ok(int Kp, int Np) { return SPEF_X2_PWS && Kp == X2PwsWide::KP && Np % X2PwsWide::NC == 0; }

template <bool POOL>
static hipError_t x2_pws_wide_go(const void* x, const void* wt, const float* bias, float* y, int64_t M, int K, int N,
                                 int Np, hipStream_t s) {
  using T = X2PwsWide;
  const int n_chunks = Np / T::NC;
  const int64_t nwg64 = (M + T::PT - 1) / T::PT * n_chunks;
  if (nwg64 > 0x7fffffff) return hipErrorInvalidValue;
  const uint32_t nwg = (uint32_t)nwg64;
  static DevOnce attr_set;
  const hipError_t e = lds_attr_once(attr_set, x2_pws_kernel<POOL, T>, T::LDS_BYTES);
  if (e != hipSuccess) return e;
  x2_pws_kernel<POOL, T><<<nwg, 256, T::LDS_BYTES, s>>>((const float*)x, (const _Float16*)wt, bias, y, M, K, N, Np,
                                                        n_chunks, nwg);
  return hipGetLastError();
}

template <bool POOL>
static hipError_t x2_pws_go(const void* x, const void* wt, const float* bias, float* y, int64_t M, int K, int N, int Np,
                            int Kp, hipStream_t s) {
  const bool five = SPEF_X2_PWS_NWV == 5 && Np % 320 == 0;
  const int n_chunks = Np / (five ? 320 : 256);
  const int64_t nwg64 = (M + 63) / 64 * n_chunks;
  if (nwg64 > 0x7fffffff) return hipErrorInvalidValue;
  const uint32_t nwg = (uint32_t)nwg64;
  const int lds = 64 * Kp * 2 * (int)sizeof(_Float16);
  constexpr int max_lds = 64 * 320 * 2 * (int)sizeof(_Float16);   // the largest Kp
  static DevOnce attr_set4, attr_set5;
  hipError_t e = lds_attr_once(attr_set4, x2_pws_kernel<POOL, 4>, max_lds);
  if (e == hipSuccess) e = lds_attr_once(attr_set5, x2_pws_kernel<POOL, 5>, max_lds);
  if (e != hipSuccess) return e;
  if (five)
    x2_pws_kernel<POOL, 5><<<nwg, 320, lds, s>>>((const float*)x, (const _Float16*)wt, bias, y, M, K, N, Np, Kp,
                                                 n_chunks, nwg);
  else
    x2_pws_kernel<POOL, 4><<<nwg, 256, lds, s>>>((const float*)x, (const _Float16*)wt, bias, y, M, K, N, Np, Kp,
                                                 n_chunks, nwg);
  return hipGetLastError();
}

// pooled[b][c] = (sum over the image's HW / 64 wave partials, in order) / HW
__global__ __launch_bounds__(256) void x2_pool_reduce_kernel(const float* __restrict__ part, float* __restrict__ pooled,
                                                             int B, int nblk, int N, float inv_hw) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * N) return;
  const int b = (int)(i / N), c = (int)(i % N);
  const float* p = part + (size_t)b * nblk * N + c;
  float t = 0.f;
  for (int j = 0; j < nblk; ++j) t += p[(size_t)j * N];
  pooled[i] = t * inv_hw;
}

hipError_t launch_x2_pw_relu(const void* x, const void* wt, const float* bias, float* y, int64_t M, int K, int N,
                             hipStream_t s, bool wide) {
  if (M <= 0) return hipSuccess;
  const int Kp = (K + 31) & ~31, Np = (N + 15) & ~15;
  if ((K & 7) || (N & 3) || Np % 64) return hipErrorInvalidValue;
  if (wide && x2_pws_wide_ok(Kp, Np)) return x2_pws_wide_go<false>(x, wt, bias, y, M, K, N, Np, s);
  if (x2_pws_ok(Kp, Np)) return x2_pws_go<false>(x, wt, bias, y, M, K, N, Np, Kp, s);
  constexpr int NT = 4, MT = 4;
  const int n_chunks = Np / (16 * NT);
  const int64_t nwg64 = (M + 64 * MT - 1) / (64 * MT) * n_chunks;
  if (nwg64 > 0x7fffffff) return hipErrorInvalidValue;
  const uint32_t nwg = (uint32_t)nwg64;
  x2_pw_kernel<NT, MT, false><<<nwg, 256, 0, s>>>((const float*)x, (const _Float16*)wt, bias, y, M, K, N, Np, Kp,
                                                  n_chunks, nwg);
  return hipGetLastError();
}

bool x2_pw_pool_supported(int HW, int N) { return HW % 64 == 0 && N % 64 == 0; }

hipError_t launch_x2_pw_pool(const void* x, const void* wt, const float* bias, float* part, float* pooled, int B,
                             int HW, int K, int N, hipStream_t s, bool wide) {
  const int Kp = (K + 31) & ~31, Np = (N + 15) & ~15;
  if ((K & 7) || !x2_pw_pool_supported(HW, N) || B <= 0) return hipErrorInvalidValue;
  constexpr int NT = 4, MT = 4;
  const int64_t M = (int64_t)B * HW;
  hipError_t e;
  if (wide && x2_pws_wide_ok(Kp, Np)) {
    e = x2_pws_wide_go<true>(x, wt, bias, part, M, K, N, Np, s);
  } else if (x2_pws_ok(Kp, Np)) {
    e = x2_pws_go<true>(x, wt, bias, part, M, K, N, Np, Kp, s);
  } else {
    const int n_chunks = Np / (16 * NT);
    const int64_t nwg64 = (M + 64 * MT - 1) / (64 * MT) * n_chunks;
    if (nwg64 > 0x7fffffff) return hipErrorInvalidValue;
    const uint32_t nwg = (uint32_t)nwg64;
    x2_pw_kernel<NT, MT, true><<<nwg, 256, 0, s>>>((const float*)x, (const _Float16*)wt, bias, part, M, K, N, Np, Kp,
                                                   n_chunks, nwg);
    e = hipGetLastError();
  }
  if (e != hipSuccess) return e;
  x2_pool_reduce_kernel<<<(unsigned)(((int64_t)B * N + 255) / 256), 256, 0, s>>>(part, pooled, B, HW / 64, N,
                                                                                 1.0f / (float)HW);
  return hipGetLastError();
}

}  // namespace spef
