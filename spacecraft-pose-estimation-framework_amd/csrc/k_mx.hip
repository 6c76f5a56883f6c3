// fp16mx schedule, high-resolution blocks 2-4 (blob dtype 6): one fused InvertedResidual per kernel
// (src/modeling/common/pytorch_layers.py:65-98) with the precision the schedule's error budget asks for
// (tools/precision_budget.py):
//   * every weight exact to 22 bits: 1x1 weights as hi + lo fp16 MFMA operands (blob dtype 5/6 planes), depthwise
//     weights fp32, depthwise accumulation fp32 -- the weight rounding classes W1 / WD / A are what the fp16
//     schedule loses most at trained head scales;
//   * the depthwise output exact (hi + lo operand of the project: three MFMAs per product);
//   * block input / output of blocks 1-3 (the 256^2 / 128^2 maps) and the expanded hidden slab of blocks 2-4 in fp16,
//     fp32 block outputs from block 4 on (rounding classes O and H: together with the stem map rms 1.2e-4, max
//     4.2e-4 |d logit| at head std 0.3 on the parity tests' frames, against the 1e-3 bound; fp16 outputs on blocks
//     4-6 and fp16 hidden on 5-7 too: rms 1.9e-4, max 7.9e-4).
//
// Layout of the work (4 waves, output tile TH x 16, PPL = TH x 16 / 64 output pixels per lane):
//   expand   the fp16 input tile (+halo) stays in registers as MFMA B fragments (loaded once); per 32-channel hidden
//            chunk every wave runs its pixel tiles through W_hi x + W_lo x (x is exact in fp16), ReLU, converts to
//            fp16 and stores the hidden slab [pixel][32] (80-B pixel rows: conflict-free reads below). Pixels outside
//            the image hold zeros (stored once; their lanes' later stores go to a dummy row).
//   depthwise wave w owns channels 8w..8w+7 of the chunk for every output pixel: its 9 x 8 fp32 weights are
//            wave-uniform (SGPRs, one scalar load per chunk -- no LDS traffic), a lane owns PPL vertically adjacent
//            output pixels of one column and reads each of their shared input rows once (5 rows for 2 pixels at
//            stride 2, 6 rows for 4 pixels at stride 1). Lanes map to (row group, column) by the ds_read_b128 lane
//            groups (MI355X_MICROARCH.md, LDS), so a group's 16 lanes read one row's 16 columns.
//   exchange the ReLU'd sums, split hi / lo, go to a [pixel][32] exchange buffer (96-B rows, odd row groups skewed
//            by 16 B: conflict-free on both sides); after one barrier every wave reads its project B fragments.
//   project  three MFMAs per product (W_hi d_hi + W_lo d_hi + W_hi d_lo), fp32 accumulators across chunks; + residual
//            (the block input) -> fp16 (blocks 2-3) or fp32 (blocks 4-7) NHWC.
// Two barriers per chunk (slab ready; exchange ready).
#include <type_traits>

#include "spef_kernels.hpp"
#include "x2_common.hpp"   // lo_pair, mfma_x2

namespace spef {

namespace {

// ds_read_b128 lane groups: {0-3,12-15,20-27}, {4-11,16-19,28-31}, {32-35,44-47,52-59}, {36-43,48-51,60-63}.
// Lane -> (group, index within group): the depthwise lane's (row group, column).
__device__ __forceinline__ void b128_group(int lane, int& g, int& i) {
  const int h = lane >> 5, l = lane & 31;   // the upper 32 lanes repeat the lower pattern (groups 2, 3)
  int gg, ii;
  if (l < 4) { gg = 0; ii = l; }
  else if (l < 12) { gg = 1; ii = l - 4; }
  else if (l < 16) { gg = 0; ii = l - 8; }
  else if (l < 20) { gg = 1; ii = l - 8; }
  else if (l < 28) { gg = 0; ii = l - 12; }
  else { gg = 1; ii = l - 16; }
  g = gg + 2 * h;
  i = ii;
}

// The same map without branches (the lean set-up): by lane quad t = l / 4 the group bit is 0 1 1 0 1 0 0 1 and the
// index l - 4 ((t + 1) / 2).
__device__ __forceinline__ void b128_group_lean(int lane, int& g, int& i) {
  const int l = lane & 31, t = l >> 2;
  g = ((0x96 >> t) & 1) + 2 * (lane >> 5);
  i = l - 4 * ((t + 1) >> 1);
}
constexpr bool b128_group_same() {   // (the branchy form restated: a constexpr check of the table above)
  for (int l = 0; l < 32; ++l) {
    const int t = l >> 2, gg = (0x96 >> t) & 1, ii = l - 4 * ((t + 1) >> 1);
    const int rg = l < 4 ? 0 : l < 12 ? 1 : l < 16 ? 0 : l < 20 ? 1 : l < 28 ? 0 : 1;
    const int ri = l < 4 ? l : l < 12 ? l - 4 : l < 20 ? l - 8 : l < 28 ? l - 12 : l - 16;
    if (gg != rg || ii != ri) return false;
  }
  return true;
}
static_assert(b128_group_same(), "b128_group_lean");

}  // namespace

template <int CIN, int HID, int COUT, int S, int TH>
struct MxGeom {
  static constexpr int NW = 4, TW = 16;
  static constexpr int IH = (TH - 1) * S + 3, IW = (TW - 1) * S + 3;
  static constexpr int PIN = IH * IW, PIN16 = (PIN + 15) / 16, PINP = PIN16 * 16;
  static constexpr int EPT = (PIN16 + NW - 1) / NW;       // expand pixel tiles per wave
  static constexpr int NCH = (HID + 31) / 32, HIDP = NCH * 32;
  static constexpr int NCT = (COUT + 15) / 16, NPC = NCT * 16;
  static constexpr int POUT = TH * TW, PPL = POUT / 64;   // output pixels per depthwise lane (a vertical run)
  static constexpr int QPW = POUT / 16 / NW;              // project pixel tiles (output rows) per wave
  static constexpr int NR = S * (PPL - 1) + 3;            // input rows a depthwise lane reads
  static constexpr int SPB = 80;                          // slab bytes per pixel (32 fp16 + 16 B pad)
  static constexpr int DXB = 96;                          // exchange bytes per pixel (32 fp16 + 32 B pad)
  static constexpr int SLAB_B = PINP * SPB;
  static constexpr int DX_B = POUT * DXB + 16;            // one exchange plane (+ the odd-row-group skew)
  static constexpr int TRASH_B = 16 * SPB;                // dummy rows for invalid pixels' expand stores
  // the exchange planes overlay the slab (two more barriers per chunk, ~35 % less LDS: 3 workgroups per CU instead of
  // 2 at stride 2)
  static constexpr int OFF_DX = 0;
  static constexpr int OFF_TR = SLAB_B > 2 * DX_B ? SLAB_B : 2 * DX_B;
  static constexpr int LDS_BYTES = OFF_TR + TRASH_B;
  static constexpr int WAVES_PER_EU = (163840 / LDS_BYTES) > 4 ? 4 : (163840 / LDS_BYTES);   // (> 4: spills)
  static_assert(CIN <= 32 && CIN % 8 == 0, "blocks 2-7: one K = 32 step");
  static_assert(POUT % 64 == 0 && (POUT / 16) % NW == 0, "tile");
  static_assert(COUT % 4 == 0, "cout");
  static_assert(EPT <= 32, "validity mask");
};

// pixel tile 0's row of a lane's tile pixel p < 64: p / IW as one 24-bit multiply (exact for p < 64, checked below)
constexpr bool mx_div64_exact(int d) {
  for (int p = 0; p < 64; ++p)
    if (((p * (65536 / d + 1)) >> 16) != p / d) return false;
  return true;
}

// LEAN (SPEF_OPT_TRIM bit 1): the tile set-up without the 64-bit per-pixel address arithmetic -- the same loads,
// stores and sums, bit-identical to LEAN = false (the launcher takes it when an image's maps are below 2^31 bytes):
//   * the image is a buffer resource (scalar base, 32-bit per-lane byte offsets); a pixel outside the image, a lane
//     beyond the tile and a k group beyond CIN read at an offset past the resource, which returns zeros: no branch
//     and no zero moves per tile;
//   * (py, px) of a lane's pixel tiles by the compile-time step of 64 tile pixels with one carry select per tile,
//     one division (a 24-bit multiply) for tile 0;
//   * interior workgroups: no bounds checks, offsets by adds of two workgroup-uniform steps; edge workgroups:
//     unsigned compares into the 32-bit zmask, the padding zeros stored by the chunk loop's restore code;
//   * the epilogue's row bases are scalar, a lane adds one 32-bit offset.
template <int CIN, int HID, int COUT, int S, int TH, bool RES, bool IN16, bool OUT16, bool LEAN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MxGeom<CIN, HID, COUT, S, TH>::WAVES_PER_EU)))
void mx_irb_kernel(const void* __restrict__ X, const _Float16* __restrict__ We, const float* __restrict__ be,
                   const float* __restrict__ Wd, const float* __restrict__ bd, const _Float16* __restrict__ Wp,
                   const float* __restrict__ bp, void* __restrict__ Y, int H, int W, int OH, int OW, int tiles_x,
                   int tiles_y, uint32_t nwg) {
  using G = MxGeom<CIN, HID, COUT, S, TH>;
  constexpr int TW = G::TW;
  // CIN = 16 (block 2): W_hi x + W_lo x as ONE K = 32 MFMA -- A = [W_hi | W_lo] along k, B = [x ; x] (lanes kg = 2, 3
  // repeat the channels of kg = 0, 1): half the expand MFMAs of the two-product form, the same sums.
  static_assert(IN16, "fp16 block input (blocks 2-4; blocks 5-7 run the fp16x2 slab kernel)");
  constexpr bool PK = CIN == 16;
  constexpr int KX = PK ? 16 : 32;   // channel span of the B fragment's k groups
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, kg = lane >> 4;
  uint32_t L = xcd_remap(blockIdx.x, nwg);
  const int tx = (int)(L % (uint32_t)tiles_x);
  L /= (uint32_t)tiles_x;
  const int ty = (int)(L % (uint32_t)tiles_y);
  const int b = (int)(L / (uint32_t)tiles_y);
  const int oy0 = ty * TH, ox0 = tx * TW;
  const int iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;
  const size_t xb = (size_t)b * H * W * CIN;   // element offset of this image's input

  // ---- expand operands: this wave's input-tile pixel tiles pt = wave + 4 j (lane: pixel r16, channels 8kg..8kg+7);
  // the fp16 input is exact (two MFMAs per product); slab slot of input-tile pixel p: p (row-major)
  f16x8 bx[G::EPT];
  uint32_t zmask = 0;   // the lane's padding pixels (per expand tile)
  const bool edge = iy0 < 0 || ix0 < 0 || iy0 + G::IH > H || ix0 + G::IW > W;   // workgroup-uniform
  // Expand MFMA row m of half h is hidden channel 8 (m / 4) + 4 h + m % 4 of the chunk (expand weight rows and bias
  // read in that order), so a lane's two C fragments are channels 8 kg .. 8 kg + 7 and leave as one 16-B store; the
  // natural order's two 8-B stores per fragment pair were 2-way bank-conflicted (16 consecutive 80-B pixel slots).
  // The slab keeps the natural channel order; every hidden value is the same sum, bit-identical (interleaved A/B: LDS
  // conflict / active cycles of block 3 0.20 -> 0.02, blocks 2 / 4 -1.6 / -0.4 us).
  constexpr int KGB = 16;   // slab bytes per k group of a lane's store
  auto erow = [&](int h) { return 8 * (r16 >> 2) + 4 * h + (r16 & 3); };
  auto zero_slot = [&](int o) { *reinterpret_cast<uint4*>(smem + o) = make_uint4(0u, 0u, 0u, 0u); };
  int soff[G::EPT];   // slab byte offset of the lane's pixel (its first channel of h = 0), or its dummy row
  if constexpr (LEAN) {
    constexpr int CB = CIN * 2;                             // bytes per input pixel
    constexpr int DY = 64 / G::IW, DX = 64 % G::IW;         // a lane's pixel tiles are 64 tile pixels apart
    constexpr uint32_t OOB = 0x80000000u;                   // past every image (launcher): the load returns zeros
    static_assert(mx_div64_exact(G::IW), "tile 0's row by multiply");
    const int pitch = W * CB;                               // < 2^23 (launcher)
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(X)) + (size_t)b * H * W * CB, 0, H * W * CB, 0x00020000);
    auto ld = [&](uint32_t o) { return __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(xr, o, 0, 0)); };
    const int p0 = wave * 16 + r16;                         // the lane's pixel of tile j: p0 + 64 j
    const int py = (int)(__umul24(p0, 65536 / G::IW + 1) >> 16), px = p0 - __mul24(py, G::IW);
    const int kc = 8 * kg % KX;                             // the lane's first input channel
    const uint32_t kco = kc < CIN ? 2u * kc : OOB;          // k groups beyond CIN read zeros
    const int s0 = __mul24(p0, G::SPB) + KGB * kg, tr = G::OFF_TR + r16 * G::SPB + KGB * kg;
    // the image pixel (iy, ix) of the lane's tile pixel and its byte offset, stepped from tile to tile: 64 tile pixels
    // on are DY rows and DX columns, one row more and IW columns back where the column leaves the tile. The offset of
    // a pixel outside the image is the same sum modulo 2^32 (signed 24-bit multiplies), never loaded from.
    const uint32_t st = DY * pitch + DX * CB, sw = st + pitch - G::IW * CB;   // workgroup-uniform offset steps
    const int ixe = ix0 + G::IW;
    int iy = iy0 + py, ix = ix0 + px;
    uint32_t off = (uint32_t)__mul24(iy, pitch) + (uint32_t)__mul24(ix, CB) + kco;
    auto tiles = [&](auto chk) {
#pragma unroll
      for (int j = 0; j < G::EPT; ++j) {
        const bool inb = 64 * j + 63 < G::PIN || p0 + 64 * j < G::PIN;   // compile-time but for the last tile
        bool ok = inb;
        if constexpr (decltype(chk)::value)   // (& not &&: selects, no branches)
          ok = ok & ((unsigned)iy < (unsigned)H) & ((unsigned)ix < (unsigned)W);
        bx[j] = ld(off | (ok ? 0u : OOB));   // (an or, not a select of offsets: the compiler branches around those)
        soff[j] = ok ? s0 + 64 * j * G::SPB : tr;
        if constexpr (decltype(chk)::value)   // zeroed by the chunk loop (every chunk: the exchange overlays the slab)
          zmask |= (inb & !ok) ? 1u << j : 0u;
        ix += DX;
        const bool cy = ix >= ixe;
        ix -= cy ? G::IW : 0;
        off += cy ? sw : st;
        if constexpr (decltype(chk)::value) iy += DY + (cy ? 1 : 0);
      }
    };
    if (!edge) tiles(std::false_type{});   // interior workgroup: every tile pixel is in the image
    else tiles(std::true_type{});
  } else {
#pragma unroll
    for (int j = 0; j < G::EPT; ++j) {
      const int p = (wave + G::NW * j) * 16 + r16;
      bool ok = false;
      int iy = 0, ix = 0;
      if (p < G::PIN) {
        const int py = p / G::IW, px = p - py * G::IW;
        iy = iy0 + py;
        ix = ix0 + px;
        ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
      }
      const int kc = 8 * kg % KX;   // the lane's first input channel
      const size_t e0 = xb + ((size_t)iy * W + ix) * CIN + kc;
      {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (ok && kc < CIN) v = *reinterpret_cast<const uint4*>(reinterpret_cast<const _Float16*>(X) + e0);
        bx[j] = __builtin_bit_cast(f16x8, v);
      }
      const int ps = p;
      if (!ok && p < G::PIN) zmask |= 1u << j;   // (re-zeroed every chunk on edge tiles: the exchange overlays the slab)
      soff[j] = ok ? ps * G::SPB + KGB * kg : G::OFF_TR + r16 * G::SPB + KGB * kg;
      if (!ok && p < G::PIN) zero_slot(ps * G::SPB + KGB * kg);   // the depthwise's zero padding
    }
  }

  // ---- depthwise lane geometry: (row group ry, column cx) from the ds_read_b128 lane groups
  int ry, cx;
  if constexpr (LEAN) b128_group_lean(lane, ry, cx);
  else b128_group(lane, ry, cx);
  // LDS byte offsets are below 2^24: 24-bit multiplies in the lean set-up (full rate; the same products)
  auto lmul = [](int a, int k) { return LEAN ? (int)__umul24(a, k) : a * k; };
  const int dbase = lmul(S * ry * G::PPL * G::IW + S * cx, G::SPB) + 16 * wave;   // input row 0, kx 0
  constexpr int KXO[3] = {0, G::SPB, 2 * G::SPB};   // slab byte step of tap kx
  char* Dh = smem + G::OFF_DX;
  char* Dl = Dh + G::DX_B;
  const int skw = (ry & 1) * 16;

  // ---- project accumulators (bias), fragments of chunk 0
  f32x4 acc[G::QPW][G::NCT];
#pragma unroll
  for (int t = 0; t < G::NCT; ++t) {
    const float4 bb = *reinterpret_cast<const float4*>(bp + t * 16 + 4 * kg);
#pragma unroll
    for (int q = 0; q < G::QPW; ++q) acc[q][t] = f32x4{bb.x, bb.y, bb.z, bb.w};
  }
  const _Float16* WeLo = We + (size_t)G::HIDP * 32;
  const _Float16* WpLo = Wp + (size_t)G::NPC * G::HIDP;
  f16x8 eah[2], eal[2], pah[G::NCT], pal[G::NCT];
  auto load_e = [&](int k) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if constexpr (PK) {   // k groups 0, 1: W_hi channels 0-15; 2, 3: W_lo channels 0-15
        const size_t off = (size_t)(32 * k + erow(h)) * 32 + 8 * (kg & 1);
        eah[h] = *reinterpret_cast<const f16x8*>((kg < 2 ? We : WeLo) + off);
      } else {
        const size_t off = (size_t)(32 * k + erow(h)) * 32 + 8 * kg;
        eah[h] = *reinterpret_cast<const f16x8*>(We + off);
        eal[h] = *reinterpret_cast<const f16x8*>(WeLo + off);
      }
    }
  };
  auto load_p = [&](int k) {
#pragma unroll
    for (int t = 0; t < G::NCT; ++t) {
      const size_t off = (size_t)(t * 16 + r16) * G::HIDP + 32 * k + 8 * kg;
      pah[t] = *reinterpret_cast<const f16x8*>(Wp + off);
      pal[t] = *reinterpret_cast<const f16x8*>(WpLo + off);
    }
  };
  load_e(0);
  load_p(0);

#pragma unroll 1
  for (int c = 0; c < G::NCH; ++c) {
    // wave-uniform depthwise weights + bias of this wave's 8 channels (scalar loads; fp32, exact)
    const float* wdc = Wd + 32 * c + 8 * wave;
    float wd[9][8], db[8];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int e = 0; e < 8; ++e) wd[tap][e] = wdc[tap * G::HIDP + e];
    {   // the bias as two vector loads (uniform address: VGPRs, keeping the 72 weights' SGPRs free of spills)
      const float4 b0 = *reinterpret_cast<const float4*>(bd + 32 * c + 8 * (tid >> 6));
      const float4 b1 = *reinterpret_cast<const float4*>(bd + 32 * c + 8 * (tid >> 6) + 4);
      db[0] = b0.x; db[1] = b0.y; db[2] = b0.z; db[3] = b0.w; db[4] = b1.x; db[5] = b1.y; db[6] = b1.z; db[7] = b1.w;
    }

    // ---- expand chunk c -> fp16 slab
    {
      float4 eb[2];
#pragma unroll
      for (int h = 0; h < 2; ++h)
        eb[h] = *reinterpret_cast<const float4*>(be + 32 * c + 8 * kg + 4 * h);
#pragma unroll
      for (int j = 0; j < G::EPT; ++j) {
        f32x4 e[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          e[h] = f32x4{eb[h].x, eb[h].y, eb[h].z, eb[h].w};
          e[h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(eah[h], bx[j], e[h], 0, 0, 0);
          if constexpr (!PK) e[h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(eal[h], bx[j], e[h], 0, 0, 0);
        }
        // the lane's 8 hidden channels 8 kg .. 8 kg + 7
        *reinterpret_cast<uint4*>(smem + soff[j]) = make_uint4(relu_pk2(e[0][0], e[0][1]), relu_pk2(e[0][2], e[0][3]),
                                                               relu_pk2(e[1][0], e[1][1]), relu_pk2(e[1][2], e[1][3]));
      }
      if (edge && (LEAN || c > 0)) {   // the exchange overlaid the slab: restore the depthwise's zero padding
#pragma unroll
        for (int j = 0; j < G::EPT; ++j)
          if ((zmask >> j) & 1u) {
            const int pz = (wave + G::NW * j) * 16 + r16;
            zero_slot(pz * G::SPB + KGB * kg);
          }
      }
      if (c + 1 < G::NCH) load_e(c + 1);
    }
    __syncthreads();   // slab of chunk c complete (and chunk c - 1's exchange buffer consumed)

    // ---- depthwise: PPL output rows of column cx, channels 8 wave .. +7, fp32 accumulation, exact weights
    float a[G::PPL][8];
#pragma unroll
    for (int t = 0; t < G::PPL; ++t)
#pragma unroll
      for (int e = 0; e < 8; ++e) a[t][e] = db[e];
    // one input row r, tap column kx: its contributions to the lane's PPL output rows (ky = r - S t)
    auto dw_col = [&](int r, int kx, const uint4 xv) {
      const uint32_t xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
      for (int t = 0; t < G::PPL; ++t) {
        const int ky = r - S * t;
        if (ky < 0 || ky > 2) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a[t][2 * e] = fmaf(h_lo(xs[e]), wd[ky * 3 + kx][2 * e], a[t][2 * e]);
          a[t][2 * e + 1] = fmaf(h_hi(xs[e]), wd[ky * 3 + kx][2 * e + 1], a[t][2 * e + 1]);
        }
      }
    };
    auto rd = [&](int r, int kx) { return *reinterpret_cast<const uint4*>(smem + dbase + r * G::IW * G::SPB + KXO[kx]); };
    if constexpr (S == 2) {
      // stride 2 (blocks 2, 4): a row's three tap columns read together and the next row's issued before this row's
      // FMAs (up to six reads in flight per lane instead of one; the same FMAs per accumulator in the same order,
      // bit-identical: interleaved A/B, block 2 122.3 -> 119.7 us, block 4 62.5 -> 59.4). Stride 1 (block 3) has no
      // registers for the next row's buffers in its 168-register budget (3 waves per SIMD); at two waves per SIMD (180
      // registers) it measured 133 -> 148 us.
      uint4 xr[2][3];
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) xr[0][kx] = rd(0, kx);
#pragma unroll
      for (int r = 0; r < G::NR; ++r) {
        if (r + 1 < G::NR) {
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) xr[(r + 1) & 1][kx] = rd(r + 1, kx);
        }
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) dw_col(r, kx, xr[r & 1][kx]);
      }
    } else {   // stride 1 (block 3): a row's three tap columns read together (block 3 132.4 -> 123.2 us, with the
      // 16-B expand stores' register savings: 164 of its 168 registers)
#pragma unroll
      for (int r = 0; r < G::NR; ++r) {
        uint4 xr[3];
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) xr[kx] = rd(r, kx);
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) dw_col(r, kx, xr[kx]);
      }
    }
    __syncthreads();   // every wave's slab reads done before the exchange overlays it
    // ReLU, hi / lo split -> exchange buffer (pixel (row ry PPL + t, column cx), channels 8 wave ..)
#pragma unroll
    for (int t = 0; t < G::PPL; ++t) {
      uint32_t hh[4], ll[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float x0 = fmaxf(a[t][2 * e], 0.f), x1 = fmaxf(a[t][2 * e + 1], 0.f);
        hh[e] = pack_h2((_Float16)x0, (_Float16)x1);
        ll[e] = lo_pair(hh[e], x0, x1);
      }
      const int px = (ry * G::PPL + t) * TW + cx;
      const int o = (LEAN ? lmul(ry * G::PPL * TW + cx, G::DXB) + t * (TW * G::DXB) : px * G::DXB) + skw + 16 * wave;
      *reinterpret_cast<uint4*>(Dh + o) = make_uint4(hh[0], hh[1], hh[2], hh[3]);
      *reinterpret_cast<uint4*>(Dl + o) = make_uint4(ll[0], ll[1], ll[2], ll[3]);
    }
    __syncthreads();   // exchange buffer of chunk c complete (and the slab consumed)

    // ---- project: output rows q = wave QPW + i, three MFMAs per product
#pragma unroll
    for (int i = 0; i < G::QPW; ++i) {
      const int q = wave * G::QPW + i;
      // (lean: the row's part is wave-uniform, the lane's part one multiply hoisted out of the loop)
      const int o = (LEAN ? q * (TW * G::DXB) + lmul(r16, G::DXB) : (q * TW + r16) * G::DXB) +
                    ((q / G::PPL) & 1) * 16 + 16 * kg;
      const f16x8 bh = *reinterpret_cast<const f16x8*>(Dh + o);
      const f16x8 bl = *reinterpret_cast<const f16x8*>(Dl + o);
#pragma unroll
      for (int t = 0; t < G::NCT; ++t) acc[i][t] = mfma_x2(pah[t], pal[t], bh, bl, acc[i][t]);
    }
    if (c + 1 < G::NCH) load_p(c + 1);
    __syncthreads();   // exchange reads done before the next expand overlays them
  }

  // ---- epilogue: + residual (fp16 block input, added after the BN bias, pytorch_layers.py:93-96)
  if constexpr (LEAN) {
    constexpr int OB = OUT16 ? 2 : 4;                         // bytes per output element
    const uint32_t oo = (uint32_t)(r16 * COUT + 4 * kg) * OB, ro = (uint32_t)(r16 * CIN + 4 * kg) * 2;
    if (ox0 + r16 < OW) {
#pragma unroll
      for (int i = 0; i < G::QPW; ++i) {
        const int gy = oy0 + wave * G::QPW + i;
        if (gy >= OH) break;                                  // wave-uniform
        const size_t pix = ((size_t)b * OH + gy) * OW + ox0;  // scalar: the row's first pixel of this tile
        char* Yq = reinterpret_cast<char*>(Y) + pix * (COUT * OB);
        const char* Xq = reinterpret_cast<const char*>(X) + pix * (CIN * 2);
#pragma unroll
        for (int t = 0; t < G::NCT; ++t) {
          if (t * 16 + 4 * kg >= COUT) continue;
          f32x4 v = acc[i][t];
          if constexpr (RES) {
            const uint2 r = *reinterpret_cast<const uint2*>(Xq + (ro + t * 32));
            v[0] += h_lo(r.x); v[1] += h_hi(r.x); v[2] += h_lo(r.y); v[3] += h_hi(r.y);
          }
          if constexpr (OUT16)
            *reinterpret_cast<uint2*>(Yq + (oo + t * 16 * OB)) =
                make_uint2(pack_h2((_Float16)v[0], (_Float16)v[1]), pack_h2((_Float16)v[2], (_Float16)v[3]));
          else
            *reinterpret_cast<float4*>(Yq + (oo + t * 16 * OB)) = make_float4(v[0], v[1], v[2], v[3]);
        }
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < G::QPW; ++i) {
      const int q = wave * G::QPW + i;
      const int gy = oy0 + q, gx = ox0 + r16;
      if (gy >= OH || gx >= OW) continue;
      const size_t pix = ((size_t)b * OH + gy) * OW + gx;
#pragma unroll
      for (int t = 0; t < G::NCT; ++t) {
        const int co = t * 16 + 4 * kg;
        if (co >= COUT) continue;
        f32x4 v = acc[i][t];
        if constexpr (RES) {
          const uint2 r = *reinterpret_cast<const uint2*>(reinterpret_cast<const _Float16*>(X) + pix * CIN + co);
          v[0] += h_lo(r.x); v[1] += h_hi(r.x); v[2] += h_lo(r.y); v[3] += h_hi(r.y);
        }
        if constexpr (OUT16)
          *reinterpret_cast<uint2*>(reinterpret_cast<_Float16*>(Y) + pix * COUT + co) =
              make_uint2(pack_h2((_Float16)v[0], (_Float16)v[1]), pack_h2((_Float16)v[2], (_Float16)v[3]));
        else
          *reinterpret_cast<float4*>(reinterpret_cast<float*>(Y) + pix * COUT + co) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
  }
}

template <int CIN, int HID, int COUT, int S, int TH, bool RES, bool IN16, bool OUT16, bool LEAN>
static hipError_t mx_go(const void* x, const void* we, const float* be, const float* wd, const float* bd,
                        const void* wp, const float* bp, void* y, int B, int H, int W, int OH, int OW, hipStream_t s) {
  using G = MxGeom<CIN, HID, COUT, S, TH>;
  TileGrid g;
  hipError_t e = tile_grid(g, OH, OW, TH, G::TW, B);
  if (e != hipSuccess) return e;
  auto k = mx_irb_kernel<CIN, HID, COUT, S, TH, RES, IN16, OUT16, LEAN>;
  static DevOnce attr_set;
  if ((e = lds_attr_once(attr_set, k, G::LDS_BYTES)) != hipSuccess) return e;
  k<<<g.nwg, 256, G::LDS_BYTES, s>>>(x, (const _Float16*)we, be, wd, bd, (const _Float16*)wp, bp, y, H,
                                     W, OH, OW, g.tiles_x, g.tiles_y, g.nwg);
  return hipGetLastError();
}

// (cin, hidden, cout, stride, residual, fp16 input, fp16 output, tile rows): blocks 2-4 of MobileNet-V2
// (mobilenet_v2.py:240-249) in the fp16mx schedule -- fp16 block outputs for blocks 1-3 (the 256^2 / 128^2 maps),
// fp32 from block 4 on; the output tile is TH x 16. Blocks 5-7 keep an fp32 hidden tensor (the fp16x2 slab kernel,
// k_x2_irb.hip): their fp16 hidden storage would add 31 % to the schedule's logit error variance
// (tools/precision_budget.py: rms 1.21e-4 -> 1.46e-4 on the parity tests' frames) for 32 us of a ~1.3 ms step.
#define SPEF_MX_TABLE(X)                                \
  X(16, 96, 24, 2, false, true, true, 8)     /* 2 */     \
  X(24, 144, 24, 1, true, true, true, 16)    /* 3 */     \
  X(24, 144, 32, 2, false, true, false, 8)   /* 4 */

bool mx_irb_supported(int cin, int hid, int cout, int stride, bool expand, bool res, bool in16, bool out16) {
#define SPEF_MX_HAS(CI, HI, CO, ST, RS, I16, O16, TH_)                                                   \
  if (cin == CI && hid == HI && cout == CO && stride == ST && expand && res == RS && in16 == I16 && out16 == O16) \
    return true;
  SPEF_MX_TABLE(SPEF_MX_HAS)
#undef SPEF_MX_HAS
  return false;
}

// The lean set-up's 32-bit offsets: one image's input map and output map below 2^31 bytes (a lane's byte offset into
// its image; an offset of 2^31 or more reads zeros), the input row pitch and the row index below 2^23 (signed
// 24-bit multiplies). A map beyond that runs the kernel with 64-bit per-pixel addresses.
bool mx_irb_lean_fits(int cin, int cout, bool out16, int H, int W, int OH, int OW) {
  return (int64_t)H * W * cin * 2 <= 0x7fffffff && (int64_t)OH * OW * cout * (out16 ? 2 : 4) <= 0x7fffffff &&
         (int64_t)W * cin * 2 < (1 << 23) && H < (1 << 23);
}

hipError_t launch_mx_irb(int cin, int hid, int cout, int stride, bool res, bool in16, bool out16, const void* x,
                         const void* we,
                         const float* be, const float* wd, const float* bd, const void* wp, const float* bp, void* y,
                         int B, int H, int W, int OH, int OW, hipStream_t s, bool lean) {
  if (!x || !y || !we || !be || !wd || !bd || !wp || !bp) return hipErrorInvalidValue;
  lean = lean && mx_irb_lean_fits(cin, cout, out16, H, W, OH, OW);
#define SPEF_MX_CASE(CI, HI, CO, ST, RS, I16, O16, TH_)                                                  \
  if (cin == CI && hid == HI && cout == CO && stride == ST && res == RS && in16 == I16 && out16 == O16)  \
    return lean ? mx_go<CI, HI, CO, ST, TH_, RS, I16, O16, true>(x, we, be, wd, bd, wp, bp, y, B, H, W, OH, OW, s)  \
                : mx_go<CI, HI, CO, ST, TH_, RS, I16, O16, false>(x, we, be, wd, bd, wp, bp, y, B, H, W, OH, OW, s);
  SPEF_MX_TABLE(SPEF_MX_CASE)
#undef SPEF_MX_CASE
  return hipErrorNotSupported;
}

// ------------------------------------------------------------------------------------------ front: stem + block 1
// fp16mx front kernel: the fp16 schedule's front kernel (k_front.hip front_vp_kernel: input bytes re-laid as
// Lr[stem row][column dword][ky] so a stem pixel's 27 taps are 15 consecutive dwords and its MFMA B fragment 4 dword
// reads; the stem in units of (row pair, column) positions into the vertical-pair slab) with the fp16mx precision:
//   * stem weights hi + lo (two MFMAs; the u8 pixels are exact in fp16), stem map stored fp16 (rounding class S);
//   * block-1 depthwise with exact weights: the fp32 weights split into hi / lo fp16 pairs, two v_dot2_f32_f16 (or
//     v_fma_mix) per tap pair, fp32 accumulation;
//   * its ReLU'd output split hi / lo for the project (three MFMAs), block-1 output fp16.
// uint8 NHWC frames -> fp16 [B][OH][OW][16]. Wsp = the blob's OP_STEM x1 (dtype 6), Wd fp32 [9][32], Wp [2][16][32].
template <int TH, int TW, int NW>
__global__ __launch_bounds__(NW * 64) void front_mx_kernel(
    const uint8_t* __restrict__ X, const _Float16* __restrict__ wsp, const float* __restrict__ bs,
    const float* __restrict__ Wd, const float* __restrict__ bd, const _Float16* __restrict__ Wp,
    const float* __restrict__ bp, _Float16* __restrict__ Y, int H, int W, int SH_img, int SW_img,
    int tiles_x, int tiles_y, uint32_t nwg) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  constexpr int SH = TH + 2, SW = TW + 2;          // stem tile (block-1 output tile + depthwise halo)
  constexpr int IH = 2 * SH + 1, IW = 2 * SW + 1;  // input tile
  constexpr int IRS = ((IW * 3 + 3) / 4 * 4 + 4 + 15) / 16 * 16;   // input LDS row stride (bytes)
  constexpr int NCD = 3 * SW + 3;                  // column dwords per Lr row (last stem pixel's pad dword included)
  constexpr int RSL = 3 * NCD;                     // dwords per stem row of Lr
  constexpr int PR = SH / 2, NQ = PR * SW, NU = (NQ + 15) / 16, NQP = NU * 16;
  constexpr int RSB = NQP * 32 + 16;               // bytes per channel-group region of the pair slab
  constexpr int EPU = (NU + NW - 1) / NW;
  constexpr int POUT16 = TH * TW / 16, QPW = POUT16 / NW;
  static_assert(SH % 2 == 0 && TW == 16 && QPW == 2 && NCD <= 64, "geometry");
  __shared__ __attribute__((aligned(16))) uint8_t In[IH * IRS];
  __shared__ __attribute__((aligned(16))) uint32_t Lr[SH * RSL + 4];
  __shared__ __attribute__((aligned(16))) char Ps[4 * RSB];
  __shared__ __attribute__((aligned(16))) float Sw[9 * 32];          // dw weights fp32 [kx][ky][32] (exact)
  __shared__ __attribute__((aligned(16))) float Sb[32];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r16 = lane & 15, kg = lane >> 4;
  uint32_t L = xcd_remap(blockIdx.x, nwg);
  const int tx = (int)(L % (uint32_t)tiles_x);
  L /= (uint32_t)tiles_x;
  const int ty = (int)(L % (uint32_t)tiles_y);
  const int b = (int)(L / (uint32_t)tiles_y);
  const int oy0 = ty * TH, ox0 = tx * TW;
  const int sy0 = oy0 - 1, sx0 = ox0 - 1;
  const int iy0 = 2 * sy0 - 1, ix0 = 2 * sx0 - 1;

  // ---- 1. input bytes -> Lr (interior tiles) or In (edge tiles), dw weight pairs (hi / lo), biases
  const bool fast = (W & 3) == 0 && ix0 >= 0 && ix0 + IW <= W;
  {
    constexpr int RB = IW * 3;
    constexpr int DPR = (RB + 3) / 4 + 1;
    constexpr int NIT = (IH + 2 * NW - 1) / (2 * NW);
    static_assert(4 * DPR <= IRS && DPR <= 32, "LDS row holds the dword-aligned run; one half-wave per row");
    const uint8_t* Xb = X + (size_t)b * H * W * 3;
    const int img_bytes = H * W * 3;
    const int k = lane & 31;
    uint32_t v[NIT];
    int a[NIT], rs[NIT];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int r = 2 * (wave + NW * i) + (lane >> 5);
      const int iy = iy0 + r;
      rs[i] = (iy * W + ix0) * 3;
      a[i] = (rs[i] & ~3) + 4 * k;
      v[i] = 0;
      if (r < IH && k < DPR && iy >= 0 && iy < H && a[i] >= 0) {
        if (a[i] + 4 <= img_bytes) {
          v[i] = *reinterpret_cast<const uint32_t*>(Xb + a[i]);
        } else {
          for (int j = 0; j < 4; ++j)
            if (a[i] + j < img_bytes) v[i] |= (uint32_t)Xb[a[i] + j] << (8 * j);
        }
      }
    }
    // dw weights: the last wave's threads 0..71 (tap vt / 8, channels 4 (vt % 8))
    const int vt = NW * 64 - 1 - tid;
    float4 wa = make_float4(0.f, 0.f, 0.f, 0.f);
    if (vt < 72) wa = *reinterpret_cast<const float4*>(Wd + 4 * vt);   // [ky*3+kx][32]
    if (fast) {
      static_assert(TW == 16, "fast-path byte phase assumes 16-wide tiles");
#pragma unroll
      for (int i = 0; i < NIT; ++i) {
        const int r = 2 * (wave + NW * i) + (lane >> 5);
        const uint32_t vn = __shfl_down(v[i], 1, 32);
        if (r < IH && k < DPR) {
          const uint32_t p0 = __builtin_amdgcn_perm(0u, v[i], 0x0c020c01u);   // [b1, 0, b2, 0]
          const uint32_t p1 = __builtin_amdgcn_perm(vn, v[i], 0x0c040c03u);   // [b3, 0, next b0, 0]
          f16x2 h0 = __builtin_bit_cast(f16x2, p0 | 0x64006400u), h1 = __builtin_bit_cast(f16x2, p1 | 0x64006400u);
          h0 = h0 - f16x2{(_Float16)1024.0f, (_Float16)1024.0f};
          h1 = h1 - f16x2{(_Float16)1024.0f, (_Float16)1024.0f};
          const uint32_t d0 = __builtin_bit_cast(uint32_t, h0), d1 = __builtin_bit_cast(uint32_t, h1);
          uint32_t* l0 = Lr + (r >> 1) * RSL + 3 * (2 * k) + (r & 1);     // (spy = r/2, ky = r%2)
          if ((r >> 1) < SH) {
            if (k > 0) l0[-3] = d0;
            l0[0] = d1;
          }
          if (!(r & 1) && r >= 2) {                                       // (spy = r/2 - 1, ky = 2)
            uint32_t* l2 = l0 - RSL + 2;
            if (k > 0) l2[-3] = d0;
            l2[0] = d1;
          }
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < NIT; ++i) {
        const int r = 2 * (wave + NW * i) + (lane >> 5);
        if (r >= IH || k >= DPR) continue;
        const int iy = iy0 + r;
        const bool row_ok = iy >= 0 && iy < H;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int o = a[i] + j - rs[i];
          if (o < 0 || o >= RB) continue;
          const int ix = ix0 + o / 3;
          In[r * IRS + o] = (row_ok && ix >= 0 && ix < W) ? (uint8_t)(v[i] >> (8 * j)) : (uint8_t)0;
        }
      }
    }
    if (vt < 72) {   // -> [kx][ky][32]
      const int tap = vt >> 3, ky = tap / 3, kx = tap - 3 * ky;
      *reinterpret_cast<float4*>(&Sw[(kx * 3 + ky) * 32 + 4 * (vt & 7)]) = wa;
    }
    if (tid < 32) Sb[tid] = bd[tid];
    if (tid < 4) Lr[SH * RSL + tid] = 0;   // pad dwords read (zero weight) by the last position of the last row
  }
  f16x8 ahi[2], alo[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    ahi[t] = *reinterpret_cast<const f16x8*>(wsp + (16 * t + r16) * 32 + 8 * kg);
    alo[t] = *reinterpret_cast<const f16x8*>(wsp + 32 * 32 + (16 * t + r16) * 32 + 8 * kg);
  }
  const float4 sb0 = *reinterpret_cast<const float4*>(bs + 4 * kg);
  const float4 sb1 = *reinterpret_cast<const float4*>(bs + 16 + 4 * kg);
  const bool interior = sy0 >= 0 && sx0 >= 0 && sy0 + SH <= SH_img && sx0 + SW <= SW_img;
  __syncthreads();

  // ---- 2. edge tiles: In -> Lr
  if (!fast) {
    if (lane < NCD) {
      const int cd = lane;
#pragma unroll
      for (int i = 0; i < (IH + NW - 1) / NW; ++i) {
        const int r = wave + NW * i;
        if (r >= IH) break;
        const uint8_t* src = In + r * IRS + 2 * cd;
        const uint32_t bv = (uint32_t)src[0] | ((uint32_t)src[1] << 16);
        f16x2 hv = __builtin_bit_cast(f16x2, bv | 0x64006400u);
        hv = hv - f16x2{(_Float16)1024.0f, (_Float16)1024.0f};
        const uint32_t dv = __builtin_bit_cast(uint32_t, hv);
        if (r & 1) {
          Lr[((r - 1) >> 1) * RSL + 3 * cd + 1] = dv;
        } else {
          if ((r >> 1) < SH) Lr[(r >> 1) * RSL + 3 * cd] = dv;
          if (r >= 2) Lr[((r >> 1) - 1) * RSL + 3 * cd + 2] = dv;
        }
      }
    }
    __syncthreads();
  }

  // ---- 3. stem on MFMA (hi + lo weights) -> pair slab Ps (ReLU, fp16; zero outside the stem map)
#pragma unroll
  for (int j = 0; j < EPU; ++j) {
    const int u = wave + NW * j;
    if (u >= NU) break;
    const int q = 16 * u + r16;
    const int qc = q < NQ ? q : NQ - 1;
    const int pr = qc / SW, col = qc - pr * SW;
    const uint32_t* lb = Lr + 2 * pr * RSL + 9 * col + 4 * kg;
    f16x8 bx[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t* p = lb + h * RSL;
      bx[h] = __builtin_bit_cast(f16x8, u32x4{p[0], p[1], p[2], p[3]});
    }
    f32x4 e[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      e[h][0] = f32x4{sb0.x, sb0.y, sb0.z, sb0.w};
      e[h][1] = f32x4{sb1.x, sb1.y, sb1.z, sb1.w};
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        e[h][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi[t], bx[h], e[h][t], 0, 0, 0);
        e[h][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(alo[t], bx[h], e[h][t], 0, 0, 0);
      }
    }
    uint4 d[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
      d[t] = make_uint4(relu_pk2(e[0][t][0], e[1][t][0]), relu_pk2(e[0][t][1], e[1][t][1]),
                        relu_pk2(e[0][t][2], e[1][t][2]), relu_pk2(e[0][t][3], e[1][t][3]));
    if (!interior) {
      const int gy = sy0 + 2 * pr, gx = sx0 + col;
      const bool cx = gx >= 0 && gx < SW_img;
      const uint32_t m = ((cx && gy >= 0 && gy < SH_img) ? 0x0000ffffu : 0u) |
                         ((cx && gy + 1 >= 0 && gy + 1 < SH_img) ? 0xffff0000u : 0u);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        d[t].x &= m; d[t].y &= m; d[t].z &= m; d[t].w &= m;
      }
    }
    char* er = Ps + q * 32 + (kg & 1) * 16;
    *reinterpret_cast<u32x4*>(er + (kg >> 1) * RSB) = u32x4{d[0].x, d[0].y, d[0].z, d[0].w};
    *reinterpret_cast<u32x4*>(er + (2 + (kg >> 1)) * RSB) = u32x4{d[1].x, d[1].y, d[1].z, d[1].w};
  }
  const f16x8 pah = *reinterpret_cast<const f16x8*>(Wp + r16 * 32 + 8 * kg);
  const f16x8 pal = *reinterpret_cast<const f16x8*>(Wp + 16 * 32 + r16 * 32 + 8 * kg);
  const float4 pb = *reinterpret_cast<const float4*>(bp + 4 * kg);
  __syncthreads();

  // ---- 4. block 1: depthwise (rows oy = 2 wave, oy + 1), exact weights -> hi / lo -> project 32 -> 16 (+BN)
  {
    const int oy = 2 * wave, ox = r16;
    const char* pbase = Ps + kg * RSB + (wave * SW + ox) * 32;
    float a0[8], a1[8];
    {
      const float4 u0 = *reinterpret_cast<const float4*>(Sb + 8 * kg);
      const float4 u1 = *reinterpret_cast<const float4*>(Sb + 8 * kg + 4);
      a0[0] = u0.x; a0[1] = u0.y; a0[2] = u0.z; a0[3] = u0.w; a0[4] = u1.x; a0[5] = u1.y; a0[6] = u1.z; a0[7] = u1.w;
#pragma unroll
      for (int e = 0; e < 8; ++e) a1[e] = a0[e];
    }
    auto rd8 = [&](const void* p, uint32_t v[8]) {
      const uint4 x = *reinterpret_cast<const uint4*>(p), y = *(reinterpret_cast<const uint4*>(p) + 1);
      v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w; v[4] = y.x; v[5] = y.y; v[6] = y.z; v[7] = y.w;
    };
    // rows oy (a0) and oy + 1 (a1) of column ox: stem rows oy .. oy + 3 are the pairs pc (oy, oy + 1), pn (oy + 2,
    // oy + 3); fp32 weights, one v_fma_mix per tap and channel
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      uint32_t pc[8], pn[8];
      rd8(pbase + kx * 32, pc);
      rd8(pbase + (SW + kx) * 32, pn);
      float w[3][8];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const float4 u0 = *reinterpret_cast<const float4*>(&Sw[(kx * 3 + ky) * 32 + 8 * kg]);
        const float4 u1 = *reinterpret_cast<const float4*>(&Sw[(kx * 3 + ky) * 32 + 8 * kg + 4]);
        w[ky][0] = u0.x; w[ky][1] = u0.y; w[ky][2] = u0.z; w[ky][3] = u0.w;
        w[ky][4] = u1.x; w[ky][5] = u1.y; w[ky][6] = u1.z; w[ky][7] = u1.w;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        a0[e] = fmaf(h_lo(pc[e]), w[0][e], a0[e]);
        a1[e] = fmaf(h_hi(pc[e]), w[0][e], a1[e]);
        a0[e] = fmaf(h_hi(pc[e]), w[1][e], a0[e]);
        a1[e] = fmaf(h_lo(pn[e]), w[1][e], a1[e]);
        a0[e] = fmaf(h_lo(pn[e]), w[2][e], a0[e]);
        a1[e] = fmaf(h_hi(pn[e]), w[2][e], a1[e]);
      }
    }
    f32x4 acc[2] = {f32x4{pb.x, pb.y, pb.z, pb.w}, f32x4{pb.x, pb.y, pb.z, pb.w}};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float* av = h ? a1 : a0;
      uint32_t hh[4], ll[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float x0 = fmaxf(av[2 * e], 0.f), x1 = fmaxf(av[2 * e + 1], 0.f);
        hh[e] = pack_h2((_Float16)x0, (_Float16)x1);
        ll[e] = lo_pair(hh[e], x0, x1);
      }
      acc[h] = mfma_x2(pah, pal, __builtin_bit_cast(f16x8, make_uint4(hh[0], hh[1], hh[2], hh[3])),
                     __builtin_bit_cast(f16x8, make_uint4(ll[0], ll[1], ll[2], ll[3])), acc[h]);
    }
    const int gy = oy0 + oy, gx = ox0 + ox;
    _Float16* yr = Y + (((size_t)b * SH_img + gy) * SW_img + gx) * 16 + 4 * kg;
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (gy + h < SH_img && gx < SW_img)
        *reinterpret_cast<uint2*>(yr + (size_t)h * SW_img * 16) =
            make_uint2(pack_h2((_Float16)acc[h][0], (_Float16)acc[h][1]), pack_h2((_Float16)acc[h][2], (_Float16)acc[h][3]));
  }
}

hipError_t launch_mx_front(const void* x, const void* wsp, const float* bs, const float* wd, const float* bd,
                           const void* wp, const float* bp, void* y, int B, int H, int W, int OH, int OW,
                           hipStream_t s) {
  constexpr int TH = 16, TW = 16, NW = 8;
  if (!x || !wsp || !bs || !wd || !bd || !wp || !bp || !y) return hipErrorInvalidValue;
  const int tiles_x = (OW + TW - 1) / TW, tiles_y = (OH + TH - 1) / TH;
  const int64_t ntiles64 = (int64_t)tiles_x * tiles_y * B;
  if (ntiles64 > 0x7fffffff) return hipErrorInvalidValue;
  if ((int64_t)H * W * 3 + 4 > 0x7fffffff) return hipErrorInvalidValue;   // 32-bit in-frame byte offsets
  front_mx_kernel<TH, TW, NW><<<(uint32_t)ntiles64, NW * 64, 0, s>>>(
      (const uint8_t*)x, (const _Float16*)wsp, bs, wd, bd, (const _Float16*)wp, bp, (_Float16*)y, H, W, OH, OW, tiles_x,
      tiles_y, (uint32_t)ntiles64);
  return hipGetLastError();
}

}  // namespace spef
