// Fused InvertedResidual block (src/modeling/common/pytorch_layers.py:65-98) on gfx950:
//   expand 1x1 + BN + ReLU  ->  depthwise 3x3 (stride S) + BN + ReLU  ->  project 1x1 + BN  (+ x)
// in ONE kernel. The 6x-wide hidden tensor never leaves the CU: per output tile, the input tile (+halo) is
// staged in LDS once, the hidden channels are produced 32 at a time into a double-buffered LDS slab by MFMA,
// the depthwise stencil reads that slab and produces the project GEMM's B fragment directly in registers,
// and the project accumulates over hidden chunks in MFMA accumulators. HBM traffic per block = read x
// (+ halo re-reads, mostly L2 hits) + write y; weights stream from L2.
//
// Rounding points are identical to the unfused kernels (fp16/bf16 after expand, after depthwise, after
// project), and so is the accumulation order: the fused block is bit-identical to the unfused schedule.
//
// MFMA 16x16x32 C^T formulation (see k_gemm.hip): A = weights [out ch][k], B = activations [k][pixel],
// lane l holds B[k = 8(l>>4)+e][pixel l&15] = 16 contiguous bytes of an LDS pixel row.
//
// Work split (NW waves): the expand distributes the input-tile pixel tiles over all waves; the depthwise +
// project phase gives wave w the output pixel tiles of group w % WP and the output-channel tiles of group
// w / WP (WCO groups; WCO > 1 duplicates the cheap depthwise to cut per-wave accumulators on wide blocks).
// Synchronisation: ONE barrier per hidden chunk. Es is double-buffered; the per-chunk depthwise weight slab
// (9x32 weights, dw bias, expand bias; fp32) is triple-buffered and filled one chunk ahead.
#include "spef_common.hpp"
#include <type_traits>
#include "spef_kernels.hpp"

namespace spef {

// Vertical-pair depthwise (VP, the fp16 slab-kernel variants of blocks 8-13): the hidden slab holds, per position (row pair pr,
// column), one dword per channel = (row 2pr, row 2pr+1) -- the depthwise takes two taps of a kernel column with one
// v_dot2_f32_f16 and the third with one v_fma_mix. The unfused dw_kernel uses the same order for these blocks
// (irb_dw_mode), so both schedules stay bit-identical. (Stride 2 measured slower: a 3-row window straddles two
// pairs, so every output row reads 1.5x the slab bytes, and the odd input-tile height wastes half a pair row.)
// Blocks 8-13 (hid 384, 576) run the same pair order in the role-split kernel (k_irw.hip); their slab-kernel variants
// follow it so every schedule of those blocks stays bit-identical.
// Packed-fp16 depthwise (PK, fp16 blocks 2-7): 4 v_pk_fma_f16 per tap for a lane's 8 channels (two
// channels per op, fp16 accumulation from the fp16-rounded bias, one rounding per fused tap) instead of 8 v_fma_mix
// -- half the depthwise VALU of the VALU-issue-bound high-resolution blocks. The ReLU'd sums are the project MFMA's B
// fragment as they are (no convert). Error budget (tools/dw_acc_budget.py, float64 restatement at 512^2): URSONet
// logits 5.26e-4 -> 5.76e-4 max |d| against fp32 with the stride-2 blocks packed, 5.25e-4 with every block packed,
// inside the north star's 1e-3 (tests/test_dw_precision.py). The unfused dw_kernel<DW_PK16>
// evaluates the same operations in the same order (bit-identical).
// Blocks 2-7 (hid 96-192). The role-split blocks 8-13 (k_irw.hip, hid 384 / 576) keep the vertical pairs: there the
// plain slab's read pattern costs more than the VALU saved (measured +10 to +29 us per role-split kernel). Block 3
// needs the wave-uniform form below (PKU) to gain: with a lane per channel group its plain slab lost 15 us.
constexpr bool irb_pk(bool f16, int hid, bool expand, int stride) { return f16 && expand && hid <= 192; }
constexpr bool irb_vp(bool f16, int hid, bool expand, int stride) {
  return f16 && expand && hid <= 576 && stride == 1 && !irb_pk(f16, hid, expand, stride);
}
// PK with wave-uniform depthwise weights (PKU; the 4-wave, single-slab PK configurations): in the depthwise phase wave
// g owns channels 8g..8g+7 of the chunk for every output pixel of the tile (a lane per pixel, or per vertical pixel
// pair on the 8x16 stride-1 tiles), so a tap's 8 weights are one wave-uniform 16-B scalar load used straight from
// SGPRs by v_pk_fma_f16 -- no LDS weight slab and none of its 9 ds_read_b128 per chunk and wave. The ReLU'd sums go
// to an LDS buffer from which each wave reads its project B fragments after one barrier (the barrier before the next
// expand is then redundant, so the barrier count is unchanged). Block 3's 16x16 tile (a lane per 4 rows of a column)
// puts the buffer over the hidden slab after one more barrier: a separate 24 KB buffer would cost a workgroup per CU. Same operations in the same order as
// the lane-per-channel-group PK path and dw_kernel<DW_PK16>.
constexpr bool irb_pku(bool pk, int nw, bool dbuf, bool stw, int s, int th, int tw) {
  return pk && nw == 4 && !dbuf && !stw && (th * tw == 64 || (th * tw >= 128 && tw == 16 && s == 1));
}
// PKU buffer row (halves): 96 B = 6 granules, 2 mod 4 -> conflict-free ds_read_b128; 80 B on 128-pixel tiles, where
// the wider rows would cost a workgroup per CU (256-pixel tiles: 24 KB over the slab)
constexpr int irb_dsu(int pout) { return pout == 128 ? 40 : 48; }

template <int CIN, int HID, int COUT, int S, int TH, int TW, bool EXPAND, bool RES, int NW, int WCO, bool DBUF,
          bool STW, int DWB = 4, bool VP = false, bool PKU = false>
struct IrbGeom {
  static constexpr int IH = (TH - 1) * S + 3, IW = (TW - 1) * S + 3;
  static constexpr int PIN = IH * IW;
  static constexpr int PIN16 = (PIN + 15) / 16;
  static constexpr int PINP = PIN16 * 16;
  // VP slab: 4 channel-group regions (channels 8g..8g+7, 32 B per position); regions 16 B apart mod 256 B so the
  // depthwise's ds_read_b128 lane groups (kg 0/1 and 2/3 mixed) hit distinct bank slots
  static constexpr int PR = (IH + 1) / 2;        // row pairs of the input tile
  static constexpr int NQ = PR * IW;             // pair positions
  static constexpr int NU = (NQ + 15) / 16;      // expand units: 16 positions = 2 MFMA pixel tiles (even, odd row)
  static constexpr int NQP = NU * 16;
  static constexpr int RS = NQP * 32 + 16;       // bytes per channel-group region
  static constexpr int EPU = (NU + NW - 1) / NW; // expand units per wave
  static constexpr int VSLAB = 3 * 64;           // dwords per chunk: [kx][(w0,w1) x 32 | (w1,w2) x 32]
  static constexpr bool K16 = CIN == 16;          // 16-channel input: K = 16 MFMA, no K padding in LDS
  static constexpr int CINP = K16 ? 16 : (CIN + 31) / 32 * 32;
  // Row strides: a multiple of 16 B that is 2 mod 4 granules makes ds_read_b128 of 16 consecutive rows
  // conflict-free over all four lane groups (MI355X_MICROARCH.md §LDS); +16 B rows leave a 2-way conflict
  // but less LDS. The wide padding is used only when it costs no workgroups per CU.
  static constexpr int NBUF = EXPAND ? (DBUF ? 2 : 1) : 0;
  static constexpr int NCH_ = (HID + 31) / 32;
  static constexpr int SLAB = 9 * 32;             // depthwise weights [9][32] of one hidden chunk (DWB bytes each)
  static constexpr int SLAB_PIECES = SLAB * DWB / 16;   // 16-B pieces of one slab
  static constexpr int BIAS = 2 * NCH_ * 32;      // floats: dw bias + expand bias of every hidden channel
  // STW: per-chunk expand / project weights staged once per workgroup in LDS (3 + 2 buffers) instead of every
  // wave fetching its own fragments from L2 (8x less L2 traffic for an 8-wave workgroup)
  static constexpr int WKP = (CIN + 31) / 32 * 32;      // blob row length of the expand weights
  static constexpr int WEK = K16 ? 16 : WKP;            // elements of a row the MFMA needs
  static constexpr int WES = K16 ? 24 : WKP + 16;       // LDS row strides (conflict-free for b128 reads)
  static constexpr int WPS = 48;
  static constexpr int NCTP = (COUT + 15) / 16 * 16;
  static constexpr int WE_ELEMS = STW && EXPAND ? 3 * 32 * WES : 0;
  static constexpr int WP_ELEMS = STW ? 2 * NCTP * WPS : 0;
  static constexpr int WE_PIECES = STW && EXPAND ? 32 * WEK / 8 : 0;
  static constexpr int WP_PIECES = STW ? NCTP * 4 : 0;
  static constexpr int W_PPT = (WE_PIECES + WP_PIECES + NW * 64 - 1) / (NW * 64);   // 16-B pieces per thread
  static constexpr int bytes_for(int xs, int es) {
    return VP ? (PINP * xs + WE_ELEMS + WP_ELEMS) * 2 + NBUF * 4 * RS + 2 * VSLAB * 4 + BIAS * 4
              : (PINP * xs + NBUF * PINP * es + WE_ELEMS + WP_ELEMS) * 2 +
                    (PKU ? (TH * TW == 256 ? 0 : TH * TW * irb_dsu(TH * TW) * 2) : 2 * SLAB * DWB) + BIAS * 4;
  }
  // Xs / slab row strides: the first of (conflict-free, +16 B, unpadded Xs) that reaches the most workgroups per
  // CU. The LDS, not the VGPRs, sets the slab kernels' occupancy (3-5 waves per SIMD), and an unpadded input tile
  // only costs bank conflicts on the few expand B-fragment reads.
  static constexpr int occ_for(int xs, int es) { return 163840 / bytes_for(xs, es); }
  static constexpr int LAYOUT = occ_for(CINP + 16, 48) >= occ_for(CINP + 8, 40)
                                    ? (occ_for(CINP + 16, 48) >= occ_for(CINP, 40) ? 0 : 2)
                                    : (occ_for(CINP + 8, 40) >= occ_for(CINP, 40) ? 1 : 2);
  static constexpr int XS = LAYOUT == 0 ? CINP + 16 : LAYOUT == 1 ? CINP + 8 : CINP;   // Xs row stride (elements)
  static constexpr int ES = EXPAND ? (LAYOUT == 0 ? 48 : 40) : XS; // hidden-chunk row stride
  static constexpr int EPT = (PIN16 + NW - 1) / NW;   // expand pixel tiles per wave
  static constexpr int NCH = (HID + 31) / 32;
  static constexpr int HIDP = NCH * 32;        // project K (blob pads to 32)
  static constexpr bool NT_Y = S == 2 && COUT == 64;   // nontemporal output stores (block 7)
  static constexpr int POUT = TH * TW;
  static constexpr int POUT16 = POUT / 16;
  static constexpr int WP = NW / WCO;          // pixel-tile groups in the depthwise/project phase
  static constexpr int QPW = POUT16 / WP;      // output pixel tiles per wave
  static constexpr int NCT = (COUT + 15) / 16;
  static constexpr int NCTW = NCT / WCO;       // output-channel tiles per wave
  static constexpr int KS = K16 ? 1 : CINP / 32;
  // depthwise row pairs: a wave's consecutive pixel tiles are vertically adjacent rows (16-wide, stride 1)
  static constexpr bool PAIR = S == 1 && TW == 16 && QPW % 2 == 0;
  static constexpr int LDS_BYTES = bytes_for(XS, ES);
  static_assert(POUT % 16 == 0 && POUT16 % WP == 0 && NW % WCO == 0 && NCT % WCO == 0, "tile split");
  static_assert(CIN % 8 == 0 && HID % 8 == 0 && COUT % 4 == 0, "channel counts must be multiples of 8");
  static_assert(EXPAND || HID == 32, "t == 1 blocks are supported for 32 channels (MobileNet-V2 block 1)");
  static_assert(!RES || (S == 1 && CIN == COUT), "residual needs stride 1 and cin == cout");
  static_assert(NW * 64 >= SLAB_PIECES, "slab fill needs one 16-B piece per thread");
  static_assert(SLAB % 4 == 0 && (NCH_ * 32) % 4 == 0, "float4 slabs");
  static_assert(EPT <= 32 && 2 * EPU <= 32, "validity mask is 32 bits");
  static_assert(LDS_BYTES <= 163840, "LDS budget");
  static_assert(!VP || S == 2 || (TW == 16 && TH % 2 == 0), "VP stride 1: 16-wide tiles (wave-uniform row parity)");
};

// ABL (timing ablations only, never dispatched by default): 1 = depthwise centre tap only, 2 = no expand
// MFMA, 3 = no expand epilogue / slab store, 4 = no project MFMA, 5 = no per-chunk barrier, 6 = no weight-staging
// global loads, 7 = no depthwise-slab global loads. Results are wrong for ABL != 0.
template <typename DT, int CIN, int HID, int COUT, int S, int TH, int TW, bool EXPAND, bool RES, int NW, int WCO,
          bool DBUF, bool STW, int ABL = 0>
__global__ __launch_bounds__(NW * 64) void irb_kernel(
    const typename DT::T* __restrict__ X, const typename DT::T* __restrict__ We, const float* __restrict__ be,
    const typename DT::DW* __restrict__ Wd, const float* __restrict__ bd, const typename DT::T* __restrict__ Wp,
    const float* __restrict__ bp, typename DT::T* __restrict__ Y, int H, int W, int OH, int OW, int tiles_x,
    int tiles_y, uint32_t nwg) {
  using DW = typename DT::DW;
  constexpr bool VP = irb_vp(std::is_same<DT, F16>::value, HID, EXPAND, S) && ABL == 0;
  constexpr bool PK = irb_pk(std::is_same<DT, F16>::value, HID, EXPAND, S) && ABL == 0;
  constexpr bool PKU = irb_pku(PK, NW, DBUF, STW, S, TH, TW);
  using G = IrbGeom<CIN, HID, COUT, S, TH, TW, EXPAND, RES, NW, WCO, DBUF, STW, (int)sizeof(DW), VP, PKU>;
  using T = typename DT::T;
  using x8 = typename DT::x8;
  using x4 = typename DT::x4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* Xs = reinterpret_cast<T*>(smem);
  T* Es0 = Xs + G::PINP * G::XS;                                            // hidden slab(s)
  constexpr int ES_BYTES = VP ? 4 * G::RS : G::PINP * G::ES * 2;           // one slab buffer
  T* Es1 = reinterpret_cast<T*>(reinterpret_cast<char*>(Es0) + (G::NBUF == 2 ? ES_BYTES : 0));
  T* WEs = reinterpret_cast<T*>(reinterpret_cast<char*>(Es0) + G::NBUF * ES_BYTES);   // [3][32][WES] expand weights
  T* WPs = WEs + G::WE_ELEMS;                                               // [2][NCTP][WPS] project weights
  DW* Sl = reinterpret_cast<DW*>(WPs + G::WP_ELEMS);                        // [2][SLAB] dw weights
  uint32_t* Slv = reinterpret_cast<uint32_t*>(Sl);                          // VP: [2][VSLAB] weight pairs
  // PKU: [POUT][DSU] depthwise out; 256-pixel tiles (block 3) put it over the hidden slab once every wave has read
  // the slab (one more barrier per chunk), since a separate buffer would cost a workgroup per CU
  constexpr bool DALIAS = PKU && TH * TW == 256;
  T* Dk = DALIAS ? Es0 : reinterpret_cast<T*>(Sl);
  constexpr int DSU = irb_dsu(TH * TW);
  static_assert(!DALIAS || (G::NBUF == 1 && G::POUT * DSU <= G::PINP * G::ES), "depthwise buffer over the slab");
  float* Bd = reinterpret_cast<float*>(reinterpret_cast<char*>(Sl) + (VP    ? 2 * G::VSLAB * 4
                                                                      : PKU ? (DALIAS ? 0 : G::POUT * DSU * 2)
                                                                            : 2 * G::SLAB * (int)sizeof(DW)));
  float* Be = Bd + G::NCH * 32;                                             // [HIDP] expand bias

  SPEF_TRACE(0);   // timeline probes (tools/kbench/blk_trace.hip irb): nothing in the library build
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r16 = lane & 15, kg = lane >> 4;
  uint32_t L = xcd_remap(blockIdx.x, nwg);       // neighbouring tiles (shared halo rows) on one XCD
  const int tx = (int)(L % (uint32_t)tiles_x);
  L /= (uint32_t)tiles_x;
  const int ty = (int)(L % (uint32_t)tiles_y);
  const int b = (int)(L / (uint32_t)tiles_y);
  const int oy0 = ty * TH, ox0 = tx * TW;
  const int iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;

  // Every global load below is branch-free (a load inside a divergent branch is waited for before the branch
  // joins): out-of-range pieces read a valid address and are zeroed when stored to LDS, after all loads are issued.

  // depthwise-weight slab of chunk cc: thread t < SLAB_PIECES moves one 16-B piece of [9][32]
  constexpr int EPP = 16 / (int)sizeof(DW);      // weights per piece
  // VP: piece t < 48 builds 4 weight pairs (kx = t / 16, pair (ky, ky+1) with ky = (t / 8) % 2, channels 4 (t % 8)..)
  // from two 8-B pieces of the [9][HID] fp16 weights
  const int vt = NW * 64 - 1 - tid;   // VP piece index: the last wave (fewest expand units) builds the pairs
  auto slab_ok = [&](int cc) {
    if constexpr (PKU) return false;
    if constexpr (VP) return vt < 48 && cc < G::NCH && 32 * cc + 4 * (vt & 7) < HID;
    return ABL != 7 && tid < G::SLAB_PIECES && cc < G::NCH && 32 * cc + ((tid * EPP) & 31) < HID;
  };
  auto slab_load = [&](int cc) -> uint4 {
    if constexpr (PKU) return make_uint4(0, 0, 0, 0);   // (no weight slab)
    if constexpr (VP) {
      const int kx = vt >> 4, ky = (vt >> 3) & 1;
      const bool ok = slab_ok(cc);
      const int off = ok ? (ky * 3 + kx) * HID + 4 * (vt & 7) + 32 * cc : 0;
      const uint2 a = *reinterpret_cast<const uint2*>(Wd + off);
      const uint2 b = *reinterpret_cast<const uint2*>(Wd + (ok ? off + 3 * HID : 0));
      return make_uint4(a.x, a.y, b.x, b.y);
    }
    const int f = tid * EPP, tap = f >> 5, ch = 32 * cc + (f & 31);
    return *reinterpret_cast<const uint4*>(Wd + (slab_ok(cc) ? tap * HID + ch : 0));
  };
  auto slab_store = [&](int cc, uint4 v) {
    if constexpr (PKU) return;
    if constexpr (VP) {
      if (vt < 48) {
        const int kx = vt >> 4, ky = (vt >> 3) & 1;
        uint4 d = make_uint4((v.x & 0xffffu) | (v.z << 16), (v.x >> 16) | (v.z & 0xffff0000u),
                             (v.y & 0xffffu) | (v.w << 16), (v.y >> 16) | (v.w & 0xffff0000u));
        if (!slab_ok(cc)) d = make_uint4(0, 0, 0, 0);
        *reinterpret_cast<uint4*>(Slv + (cc & 1) * G::VSLAB + kx * 64 + ky * 32 + 4 * (vt & 7)) = d;
      }
      return;
    }
    if (tid < G::SLAB_PIECES)
      *reinterpret_cast<uint4*>(Sl + (cc & 1) * G::SLAB + tid * EPP) = slab_ok(cc) ? v : make_uint4(0, 0, 0, 0);
  };

  // weight staging: pieces [0, WE_PIECES) = expand rows of chunk ce, then project rows of chunk cp
  x8 wst[G::W_PPT > 0 ? G::W_PPT : 1];
  auto wst_src = [&](int i, int ce, int cp) -> const T* {   // nullptr: piece not present (zero)
    const int p = ABL == 6 ? 1 << 30 : tid + NW * 64 * i;
    if (p < G::WE_PIECES) {
      const int row = p / (G::WEK / 8), g = p - row * (G::WEK / 8);
      const int h = 32 * ce + row;
      return ce < G::NCH && h < (HID + 15) / 16 * 16 ? We + (size_t)h * G::WKP + 8 * g : nullptr;
    }
    if (p < G::WE_PIECES + G::WP_PIECES) {
      const int q = p - G::WE_PIECES, row = q >> 2, g = q & 3;
      return cp < G::NCH ? Wp + (size_t)row * G::HIDP + 32 * cp + 8 * g : nullptr;
    }
    return nullptr;
  };
  auto wst_load = [&](int ce, int cp) {
    if constexpr (STW) {
#pragma unroll
      for (int i = 0; i < G::W_PPT; ++i) {
        const T* s = wst_src(i, ce, cp);
        wst[i] = load8<DT>(s ? s : We);
      }
    }
  };
  auto wst_store = [&](int ce, int cp) {
    if constexpr (STW) {
#pragma unroll
      for (int i = 0; i < G::W_PPT; ++i) {
        const int p = tid + NW * 64 * i;
        const x8 v = wst_src(i, ce, cp) ? wst[i] : zero8<DT>();
        if (p < G::WE_PIECES) {
          const int row = p / (G::WEK / 8), g = p - row * (G::WEK / 8);
          *reinterpret_cast<x8*>(WEs + (ce % 3) * 32 * G::WES + row * G::WES + 8 * g) = v;
        } else if (p < G::WE_PIECES + G::WP_PIECES) {
          const int q = p - G::WE_PIECES, row = q >> 2, g = q & 3;
          *reinterpret_cast<x8*>(WPs + (cp & 1) * G::NCTP * G::WPS + row * G::WPS + 8 * g) = v;
        }
      }
    }
  };

  // ---- 1. prologue: the input tile (+halo; outside the image and K padding -> 0), depthwise slab 0, expand
  // weights of chunk 0 and all biases -- every global load issued first, one wait, then the LDS stores
  {
    constexpr int GPR = G::CINP / 8;        // 16-B groups per LDS row (CIN 16: 2)
    constexpr int CG = CIN / 8;             // valid groups
    const T* Xb = X + (size_t)b * H * W * CIN;
    constexpr int NU = G::PINP * GPR, NIT = (NU + NW * 64 - 1) / (NW * 64);
    x8 xin[NIT];
    uint32_t okm = 0;
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int u = tid + NW * 64 * i;
      const int p = u / GPR, g = u - p * GPR;
      const int py = p / G::IW, px = p - py * G::IW;
      const int iy = iy0 + py, ix = ix0 + px;
      const bool ok = u < NU && p < G::PIN && g < CG && iy >= 0 && iy < H && ix >= 0 && ix < W;
      xin[i] = load8<DT>(Xb + (ok ? SPEF_KB_XOFF(((size_t)iy * W + ix) * CIN + g * 8) : 0));
      okm |= (uint32_t)ok << i;
    }
    const uint4 sl0 = slab_load(0);
    if constexpr (STW && EXPAND) wst_load(0, G::NCH);   // expand weights of chunk 0 (project weights follow later)
    constexpr int NBI = (G::NCH * 32 + NW * 64 - 1) / (NW * 64);
    float bdv[NBI], bev[NBI];
#pragma unroll
    for (int j = 0; j < NBI; ++j) {
      const int u = tid + NW * 64 * j, uc = u < HID ? u : HID - 1;
      bdv[j] = bd[uc];
      bev[j] = EXPAND ? be[uc] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int u = tid + NW * 64 * i;
      if (u < NU) {
        const int p = u / GPR, g = u - p * GPR;
        *reinterpret_cast<x8*>(Xs + p * G::XS + g * 8) = ((okm >> i) & 1u) ? xin[i] : zero8<DT>();
      }
    }
    slab_store(0, sl0);
    if constexpr (STW && EXPAND) wst_store(0, 0);
#pragma unroll
    for (int j = 0; j < NBI; ++j) {   // all biases, once
      const int u = tid + NW * 64 * j;
      if (u < G::NCH * 32) {
        if constexpr (PK) reinterpret_cast<_Float16*>(Bd)[u] = (_Float16)(u < HID ? bdv[j] : 0.f);   // fp16 bias
        else Bd[u] = u < HID ? bdv[j] : 0.f;
        if constexpr (EXPAND) Be[u] = u < HID ? bev[j] : 0.f;
      }
    }
  }
  wst_load(1, 0);      // in flight across the first expand
  SPEF_TRACE(1);
  __syncthreads();
  SPEF_TRACE(2);

  // per-lane validity of its expand pixels (inside the tile and the image): the depthwise zero padding
  // interior tiles (whole input tile inside the image) need no padding mask in the expand epilogue
  const bool interior = iy0 >= 0 && ix0 >= 0 && iy0 + G::IH <= H && ix0 + G::IW <= W;
  uint32_t pvmask = 0;
  if (VP && !interior) {       // VP: bits 2j / 2j+1 = even / odd row pixel of unit j
#pragma unroll
    for (int j = 0; j < G::EPU; ++j) {
      const int q = (wave + NW * j) * 16 + r16;
      if (q < G::NQ) {
        const int pr = q / G::IW, col = q - pr * G::IW;
        const int iy = iy0 + 2 * pr, ix = ix0 + col;
        const bool cx = ix >= 0 && ix < W;
        if (cx && iy >= 0 && iy < H) pvmask |= 1u << (2 * j);
        if (cx && 2 * pr + 1 < G::IH && iy + 1 >= 0 && iy + 1 < H) pvmask |= 2u << (2 * j);
      }
    }
  } else if (EXPAND && !interior) {   // only edge tiles mask (workgroup-uniform branch)
#pragma unroll
    for (int j = 0; j < G::EPT; ++j) {
      const int p = (wave + NW * j) * 16 + r16;
      if (p < G::PIN) {
        const int py = p / G::IW, px = p - py * G::IW;
        const int iy = iy0 + py, ix = ix0 + px;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) pvmask |= 1u << j;
      }
    }
  }
  const int wp = wave % G::WP, wc = wave / G::WP;
  int oyq[G::QPW], oxq[G::QPW];
#pragma unroll
  for (int qi = 0; qi < G::QPW; ++qi) {
    const int o = (wp * G::QPW + qi) * 16 + r16;
    oyq[qi] = o / TW;
    oxq[qi] = o - oyq[qi] * TW;
  }

  // Per-lane LDS element offsets, computed once: every other slab / input-tile access of this lane is one of these
  // plus a compile-time constant, which the ds_read / ds_write immediate offset field carries (no per-tap address
  // registers).
  int dwoff[G::QPW];   // top-left tap of output tile qi's 3x3 window in a hidden slab, this lane's 8 channels
#pragma unroll
  for (int qi = 0; qi < G::QPW; ++qi) dwoff[qi] = (oyq[qi] * S * G::IW + oxq[qi] * S) * G::ES + 8 * kg;
  const int xoff = (wave * 16 + r16) * G::XS + (G::K16 ? 4 : 8) * kg;   // expand B fragment of pixel tile `wave`
  const int eoff = (wave * 16 + r16) * G::ES + 4 * kg;                   // its expand output in the slab

  f32x4 acc[G::QPW][G::NCTW];   // project accumulators start at the folded-BN bias
#pragma unroll
  for (int t = 0; t < G::NCTW; ++t) {
    const float4 bb = *reinterpret_cast<const float4*>(bp + (wc * G::NCTW + t) * 16 + 4 * kg);
#pragma unroll
    for (int qi = 0; qi < G::QPW; ++qi) acc[qi][t] = f32x4{bb.x, bb.y, bb.z, bb.w};
  }

  // expand weight fragments (no STW) are prefetched one chunk ahead into registers (they were loaded at the top of
  // their own chunk and waited for right away by the expand). Branch-free: a missing second half of a partial chunk
  // (rows past the blob's HID rounded to 16) reloads the first half and is zeroed at use.
  constexpr int WKP = (CIN + 31) / 32 * 32;
  constexpr int NP16 = (HID + 15) / 16 * 16;
  x8 ca0[G::KS], ca1[G::KS];
  x4 cq0 = {}, cq1 = {};
  // (row offsets are workgroup-uniform: scalar arithmetic plus one per-lane base, no per-lane 64-bit multiplies)
  const T* we_lane = We + r16 * WKP + (G::K16 ? 4 : 8) * kg;
  auto ew_load = [&](int cc, x4& q0_, x4& q1_, x8* a0_, x8* a1_) {
    cc = cc < G::NCH ? cc : G::NCH - 1;
    const int h1 = 32 * cc + 16 < NP16 ? 32 * cc + 16 : 32 * cc;
    const T* p0 = we_lane + 32 * cc * WKP;
    const T* p1 = we_lane + h1 * WKP;
    if constexpr (G::K16) {
      q0_ = *reinterpret_cast<const x4*>(p0);
      q1_ = *reinterpret_cast<const x4*>(p1);
    } else {
#pragma unroll
      for (int ks = 0; ks < G::KS; ++ks) {
        a0_[ks] = load8<DT>(p0 + 32 * ks);
        a1_[ks] = load8<DT>(p1 + 32 * ks);
      }
    }
  };
  if constexpr (EXPAND && !STW) ew_load(0, cq0, cq1, ca0, ca1);

  constexpr bool TRC = 3 * G::NCH + 3 < SPEF_TRACE_SLOTS;   // per-chunk probes only where the slots suffice
#pragma unroll 1
  for (int c = 0; c < G::NCH; ++c) {
    if constexpr (TRC) SPEF_TRACE(3 + 3 * c);
    const uint4 slab_next = slab_load(c + 1);      // issued now, stored after this chunk's depthwise
    const DW* sl = Sl + (c & 1) * G::SLAB;
    // project weight fragments of this chunk (no STW): issued before the expand so their latency hides under it
    x8 pa[G::NCTW];
    if constexpr (!STW) {
      const T* wpp = Wp + (size_t)(wc * G::NCTW * 16 + r16) * G::HIDP + 32 * c + 8 * kg;
#pragma unroll
      for (int t = 0; t < G::NCTW; ++t) pa[t] = load8<DT>(wpp + (size_t)t * 16 * G::HIDP);
    }
    const T* Es;
    if constexpr (EXPAND) {
      if constexpr (G::NBUF == 1 && !(PKU && !DALIAS)) {
        if (c > 0) __syncthreads();   // single hidden slab: all depthwise reads of chunk c-1 done (PKU: the barrier
      }                               // between its depthwise and project already separates them)
      T* Ew = (c & 1) ? Es1 : Es0;
      const int vh = HID - 32 * c < 32 ? HID - 32 * c : 32;   // valid hidden channels in this chunk
      // ---- 2. expand: E[p][h] = relu(sum_k X[p][k] We[32c+h][k] + be) for all tile pixels
      // expand weights are stored [Np][Kp] with Kp = CIN rounded up to 32 (blob layout)
      x8 a0[G::KS], a1[G::KS];
      x4 q0 = {}, q1 = {};
      if constexpr (STW) {
        const T* w0 = WEs + (c % 3) * 32 * G::WES + r16 * G::WES;
        if constexpr (G::K16) {
          q0 = *reinterpret_cast<const x4*>(w0 + 4 * kg);
          q1 = *reinterpret_cast<const x4*>(w0 + 16 * G::WES + 4 * kg);
        } else {
#pragma unroll
          for (int ks = 0; ks < G::KS; ++ks) {
            a0[ks] = *reinterpret_cast<const x8*>(w0 + 32 * ks + 8 * kg);
            a1[ks] = *reinterpret_cast<const x8*>(w0 + 16 * G::WES + 32 * ks + 8 * kg);
          }
        }
      } else {
        x8 na0[G::KS], na1[G::KS];
        x4 nq0 = {}, nq1 = {};
        ew_load(c + 1, nq0, nq1, na0, na1);   // next chunk's fragments, in flight across this chunk
        if constexpr (G::K16) {
          q0 = cq0;
          q1 = vh > 16 ? cq1 : x4{};
          cq0 = nq0;
          cq1 = nq1;
        } else {
#pragma unroll
          for (int ks = 0; ks < G::KS; ++ks) {
            a0[ks] = ca0[ks];
            a1[ks] = vh > 16 ? ca1[ks] : zero8<DT>();
            ca0[ks] = na0[ks];
            ca1[ks] = na1[ks];
          }
        }
      }
      const float4 eb0 = *reinterpret_cast<const float4*>(Be + 32 * c + 4 * kg);
      const float4 eb1 = *reinterpret_cast<const float4*>(Be + 32 * c + 16 + 4 * kg);
      // All of this wave's B fragments first, then the MFMAs and epilogues: the compiler cannot move an Xs read
      // above the previous tile's slab store (both live in the same LDS array), so reading per tile serialised one
      // LDS round trip + MFMA latency per tile.
      // (Only while the fragments fit in 12 VGPRs: measured slower for blocks 4 and 17, where they do not.)
      constexpr int NBX = G::K16 ? 1 : G::KS;
      if constexpr (VP) {
        // unit j = 16 pair positions q; lane r16 computes the even- and odd-row pixel of its position (two MFMA
        // pixel tiles) and stores each channel's pair as one dword
        using BX = typename std::conditional<G::K16, x4, x8>::type;
        constexpr bool VBATCH = G::EPU * 2 * NBX * (G::K16 ? 2 : 4) <= 16;
        BX vbx[G::EPU][2][NBX];
        auto read_vbx = [&](int j) {
          const int q = (wave + NW * j) * 16 + r16;
          const int qc = q < G::NQ ? q : G::NQ - 1;
          const int pr = qc / G::IW, col = qc - pr * G::IW;
          const int p0 = 2 * pr * G::IW + col;
          const int p1 = (G::IH % 2 == 0 || 2 * pr + 1 < G::IH) ? p0 + G::IW : p0;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const T* xr = Xs + (h ? p1 : p0) * G::XS;
            if constexpr (G::K16) {
              vbx[j][h][0] = *reinterpret_cast<const x4*>(xr + 4 * kg);
            } else {
#pragma unroll
              for (int ks = 0; ks < G::KS; ++ks) vbx[j][h][ks] = *reinterpret_cast<const x8*>(xr + 8 * kg + 32 * ks);
            }
          }
        };
#pragma unroll
        for (int j = 0; j < G::EPU; ++j) {
          if (!VBATCH || wave + NW * j >= G::NU) break;
          read_vbx(j);
        }
#pragma unroll
        for (int j = 0; j < G::EPU; ++j) {
          const int u = wave + NW * j;
          if (u >= G::NU) break;
          if (!VBATCH) read_vbx(j);
          f32x4 e[2][2];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            e[h][0] = f32x4{eb0.x, eb0.y, eb0.z, eb0.w};
            e[h][1] = f32x4{eb1.x, eb1.y, eb1.z, eb1.w};
            if constexpr (G::K16) {
              e[h][0] = DT::mfma16(q0, vbx[j][h][0], e[h][0]);
              e[h][1] = DT::mfma16(q1, vbx[j][h][0], e[h][1]);
            } else {
#pragma unroll
              for (int ks = 0; ks < G::KS; ++ks) {
                e[h][0] = DT::mfma(a0[ks], vbx[j][h][ks], e[h][0]);
                e[h][1] = DT::mfma(a1[ks], vbx[j][h][ks], e[h][1]);
              }
            }
          }
          uint4 d[2];
#pragma unroll
          for (int t = 0; t < 2; ++t)
            d[t] = make_uint4(relu_pk2(e[0][t][0], e[1][t][0]), relu_pk2(e[0][t][1], e[1][t][1]),
                              relu_pk2(e[0][t][2], e[1][t][2]), relu_pk2(e[0][t][3], e[1][t][3]));
          if (!interior) {   // zero the halves of pixels outside the image (the depthwise padding)
            const uint32_t m = (((pvmask >> (2 * j)) & 1u) ? 0x0000ffffu : 0u) |
                               (((pvmask >> (2 * j)) & 2u) ? 0xffff0000u : 0u);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
              d[t].x &= m; d[t].y &= m; d[t].z &= m; d[t].w &= m;
            }
          }
          // channels 4kg.. -> region kg/2, channels 16+4kg.. -> region 2+kg/2; 16-B half (kg & 1) of the record
          typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
          char* er = reinterpret_cast<char*>(Ew) + (u * 16 + r16) * 32 + (kg & 1) * 16;
          *reinterpret_cast<u32x4*>(er + (kg >> 1) * G::RS) = u32x4{d[0].x, d[0].y, d[0].z, d[0].w};
          *reinterpret_cast<u32x4*>(er + (2 + (kg >> 1)) * G::RS) = u32x4{d[1].x, d[1].y, d[1].z, d[1].w};
        }
      } else {
      constexpr bool BATCH = G::EPT * NBX * (G::K16 ? 2 : 4) <= 12;
      typename std::conditional<G::K16, x4, x8>::type bxs[G::EPT][NBX];
      auto read_bx = [&](int j) {
        const int pt = wave + NW * j;
        if constexpr (G::K16) {
          bxs[j][0] = *reinterpret_cast<const x4*>(Xs + xoff + (pt - wave) * 16 * G::XS);
        } else {
#pragma unroll
          for (int ks = 0; ks < G::KS; ++ks)
            bxs[j][ks] = *reinterpret_cast<const x8*>(Xs + xoff + (pt - wave) * 16 * G::XS + 32 * ks);
        }
      };
#pragma unroll
      for (int j = 0; j < G::EPT; ++j) {
        if (!BATCH) break;
        const int pt = wave + NW * j;
        if (pt >= G::PIN16) break;
        read_bx(j);
      }
#pragma unroll
      for (int j = 0; j < G::EPT; ++j) {
        const int pt = wave + NW * j;
        if (pt >= G::PIN16) break;
        if (!BATCH) read_bx(j);
        f32x4 e0 = {eb0.x, eb0.y, eb0.z, eb0.w}, e1 = {eb1.x, eb1.y, eb1.z, eb1.w};   // bias as MFMA C
        if constexpr (ABL == 2) {
        } else if constexpr (G::K16) {
          e0 = DT::mfma16(q0, bxs[j][0], e0);
          e1 = DT::mfma16(q1, bxs[j][0], e1);
        } else {
#pragma unroll
          for (int ks = 0; ks < G::KS; ++ks) {
            e0 = DT::mfma(a0[ks], bxs[j][ks], e0);
            e1 = DT::mfma(a1[ks], bxs[j][ks], e1);
          }
        }
        x4 o0 = relu_cvt4<DT>(e0), o1 = relu_cvt4<DT>(e1);
        uint2 u0 = *reinterpret_cast<uint2*>(&o0), u1 = *reinterpret_cast<uint2*>(&o1);
        if (!interior) {   // zero the expand outputs of pixels outside the image (the depthwise padding)
          const uint32_t m0 = ((pvmask >> j) & 1u) ? 0xffffffffu : 0u;
          u0.x &= m0; u0.y &= m0; u1.x &= m0; u1.y &= m0;
        }
        // channels >= HID of a partial chunk are already 0: zero weight rows and zero bias
        T* er = Ew + eoff + (pt - wave) * 16 * G::ES;
        if constexpr (ABL != 3) {
          *reinterpret_cast<uint2*>(er) = u0;
          *reinterpret_cast<uint2*>(er + 16) = u1;
        }
      }
      }
      Es = Ew;
    } else {
      Es = Xs;
    }
    wst_store(c + 1, c);      // expand weights of chunk c+1, project weights of chunk c
    if constexpr (TRC) SPEF_TRACE(4 + 3 * c);
    if constexpr (ABL != 5) __syncthreads();
    if constexpr (TRC) SPEF_TRACE(5 + 3 * c);
    wst_load(c + 2, c + 1);   // next stage in flight across this depthwise/project and the next expand
    if constexpr (STW) {
      const T* wpp = WPs + (c & 1) * G::NCTP * G::WPS + (wc * G::NCTW * 16 + r16) * G::WPS + 8 * kg;
#pragma unroll
      for (int t = 0; t < G::NCTW; ++t) pa[t] = *reinterpret_cast<const x8*>(wpp + t * 16 * G::WPS);
    }

    // ---- 3. depthwise 3x3 on this hidden chunk -> project B fragment in registers; 4. project MFMA
    // Tap order everywhere (here, the front kernel, the unfused dw_kernel): kx outer, ky inner -- the fused
    // and unfused schedules accumulate in the same order and stay bit-identical.
    // (no channel-validity branch below: channels >= HID of a partial chunk are zero in the slab, the depthwise
    // weights and bias, so they yield ReLU(0) = +0 exactly like an explicit zero fragment)
    if constexpr (PKU) {
      const int g = __builtin_amdgcn_readfirstlane(wave);   // this wave's channel group in the depthwise phase
      const uint4* wsrc = reinterpret_cast<const uint4*>(Wd + 32 * c + 8 * g);   // wave-uniform: scalar loads
      // channels >= HID of a partial last chunk (hid 144: chunk 4, groups 2-3) have no weights in the [9][HID] tensor:
      // zero taps and bias instead of reading the next tap's row (wave-uniform branch)
      const bool gv = 32 * c + 8 * g < HID;
      uint4 wt[9];
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) wt[tap] = gv ? wsrc[tap * (HID / 8)] : make_uint4(0, 0, 0, 0);
      const uint4 bh = gv ? *reinterpret_cast<const uint4*>(reinterpret_cast<const _Float16*>(Bd) + 32 * c + 8 * g)
                          : make_uint4(0, 0, 0, 0);
      const f16x2 b2[4] = {__builtin_bit_cast(f16x2, bh.x), __builtin_bit_cast(f16x2, bh.y),
                           __builtin_bit_cast(f16x2, bh.z), __builtin_bit_cast(f16x2, bh.w)};
      if constexpr (G::POUT == 64) {
        const int oy = lane / TW, ox = lane % TW;
        f16x2 a[4] = {b2[0], b2[1], b2[2], b2[3]};
        const T* e0 = Es + (oy * S * G::IW + ox * S) * G::ES + 8 * g;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
          for (int ky = 0; ky < 3; ++ky)
            pk_fma4(a, *reinterpret_cast<const uint4*>(e0 + (ky * G::IW + kx) * G::ES), wt[ky * 3 + kx]);
        *reinterpret_cast<uint4*>(Dk + lane * DSU + 8 * g) = relu_pk4(a);
      } else if constexpr (G::POUT == 256) {   // 16x16 stride-1 tile: lane = (row quad, column), 4 rows per lane
        const int rq = lane >> 4, ox = lane & 15;
        f16x2 a[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i) a[j][i] = b2[i];
        const T* e0 = Es + (4 * rq * G::IW + ox) * G::ES + 8 * g;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          uint4 v[6];
#pragma unroll
          for (int r = 0; r < 6; ++r) v[r] = *reinterpret_cast<const uint4*>(e0 + (r * G::IW + kx) * G::ES);
#pragma unroll
          for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int j = 0; j < 4; ++j) pk_fma4(a[j], v[j + ky], wt[ky * 3 + kx]);
        }
        uint4 o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = relu_pk4(a[j]);
        __syncthreads();   // every wave's slab reads done: Dk overwrites the slab
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<uint4*>(Dk + ((4 * rq + j) * 16 + ox) * DSU + 8 * g) = o[j];
      } else {   // 8x16 stride-1 tile: lane = (row pair, column), rows 2rp and 2rp + 1 share the column's 4 input rows
        const int rp = lane >> 4, ox = lane & 15;
        f16x2 a0[4] = {b2[0], b2[1], b2[2], b2[3]}, a1[4] = {b2[0], b2[1], b2[2], b2[3]};
        const T* e0 = Es + (2 * rp * G::IW + ox) * G::ES + 8 * g;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          uint4 v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = *reinterpret_cast<const uint4*>(e0 + (r * G::IW + kx) * G::ES);
#pragma unroll
          for (int ky = 0; ky < 3; ++ky) {
            pk_fma4(a0, v[ky], wt[ky * 3 + kx]);
            pk_fma4(a1, v[ky + 1], wt[ky * 3 + kx]);
          }
        }
        *reinterpret_cast<uint4*>(Dk + (2 * rp * 16 + ox) * DSU + 8 * g) = relu_pk4(a0);
        *reinterpret_cast<uint4*>(Dk + ((2 * rp + 1) * 16 + ox) * DSU + 8 * g) = relu_pk4(a1);
      }
      __syncthreads();   // every channel group of every pixel in Dk
#pragma unroll
      for (int qi = 0; qi < G::QPW; ++qi) {
        const x8 bf = *reinterpret_cast<const x8*>(Dk + ((wp * G::QPW + qi) * 16 + r16) * DSU + 8 * kg);
#pragma unroll
        for (int t = 0; t < G::NCTW; ++t) acc[qi][t] = DT::mfma(pa[t], bf, acc[qi][t]);
      }
    } else if constexpr (PK && G::PAIR) {
      // stride 1: two vertically adjacent output rows per step share each kernel column's 4 input rows and 3 weights
#pragma unroll
      for (int qi = 0; qi < G::QPW; qi += 2) {
        const uint4 bh = *reinterpret_cast<const uint4*>(reinterpret_cast<const _Float16*>(Bd) + 32 * c + 8 * kg);
        f16x2 a0[4] = {__builtin_bit_cast(f16x2, bh.x), __builtin_bit_cast(f16x2, bh.y),
                       __builtin_bit_cast(f16x2, bh.z), __builtin_bit_cast(f16x2, bh.w)};
        f16x2 a1[4] = {a0[0], a0[1], a0[2], a0[3]};
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          uint4 w[3], v[4];
#pragma unroll
          for (int ky = 0; ky < 3; ++ky) w[ky] = *reinterpret_cast<const uint4*>(sl + (ky * 3 + kx) * 32 + 8 * kg);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = *reinterpret_cast<const uint4*>(Es + dwoff[qi] + (r * G::IW + kx) * G::ES);
#pragma unroll
          for (int ky = 0; ky < 3; ++ky) {
            pk_fma4(a0, v[ky], w[ky]);
            pk_fma4(a1, v[ky + 1], w[ky]);
          }
        }
        const x8 bf0 = __builtin_bit_cast(x8, relu_pk4(a0)), bf1 = __builtin_bit_cast(x8, relu_pk4(a1));
#pragma unroll
        for (int t = 0; t < G::NCTW; ++t) {
          acc[qi][t] = DT::mfma(pa[t], bf0, acc[qi][t]);
          acc[qi + 1][t] = DT::mfma(pa[t], bf1, acc[qi + 1][t]);
        }
      }
    } else if constexpr (PK) {
#pragma unroll
      for (int qi = 0; qi < G::QPW; ++qi) {
        const uint4 bh = *reinterpret_cast<const uint4*>(reinterpret_cast<const _Float16*>(Bd) + 32 * c + 8 * kg);
        f16x2 a[4] = {__builtin_bit_cast(f16x2, bh.x), __builtin_bit_cast(f16x2, bh.y),
                      __builtin_bit_cast(f16x2, bh.z), __builtin_bit_cast(f16x2, bh.w)};
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
          for (int ky = 0; ky < 3; ++ky)
            pk_fma4(a, *reinterpret_cast<const uint4*>(Es + dwoff[qi] + (ky * G::IW + kx) * G::ES),
                    *reinterpret_cast<const uint4*>(sl + (ky * 3 + kx) * 32 + 8 * kg));
        const uint4 o = relu_pk4(a);
        const x8 bf = __builtin_bit_cast(x8, o);
#pragma unroll
        for (int t = 0; t < G::NCTW; ++t) acc[qi][t] = DT::mfma(pa[t], bf, acc[qi][t]);
      }
    } else if constexpr (VP) {
      // Per kernel column kx: two taps by v_dot2 on a row pair, the third by v_fma_mix on one half. Output row
      // parity fixes the order: even rows (and every stride-2 row) dot2(ky 0,1) then fma(ky 2); odd rows
      // fma(ky 0) then dot2(ky 1,2) -- exactly dw_kernel<.., VP>'s order.
      // this lane's channels 8kg..8kg+7 live in region kg (32 B per position)
      const char* er = reinterpret_cast<const char*>(Es) + kg * G::RS;
      const uint32_t* sv = Slv + (c & 1) * G::VSLAB + 8 * kg;
      auto rd8 = [&](const char* p, uint32_t v[8]) {
        const uint4 a = *reinterpret_cast<const uint4*>(p), b = *reinterpret_cast<const uint4*>(p + 16);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
      };
      auto bias8 = [&](float a[8]) {
        const float4 u0 = *reinterpret_cast<const float4*>(Bd + 32 * c + 8 * kg);
        const float4 u1 = *reinterpret_cast<const float4*>(Bd + 32 * c + 8 * kg + 4);
        a[0] = u0.x; a[1] = u0.y; a[2] = u0.z; a[3] = u0.w; a[4] = u1.x; a[5] = u1.y; a[6] = u1.z; a[7] = u1.w;
      };
      if constexpr (G::PAIR) {
#pragma unroll
        for (int qi = 0; qi < G::QPW; qi += 2) {   // output rows oy (even) and oy + 1: pairs m = oy / 2 and m + 1
          x8 bf0, bf1;
          {   // (no channel-validity branch: channels >= HID are zero in the slab, weights and bias -> ReLU(0) = 0)
            float a0[8], a1[8];
            bias8(a0);
#pragma unroll
            for (int e = 0; e < 8; ++e) a1[e] = a0[e];
            const char* pb = er + ((oyq[qi] >> 1) * G::IW + oxq[qi]) * 32;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
              uint32_t pc[8], pn[8], w01[8], w12[8];
              rd8(pb + kx * 32, pc);
              rd8(pb + (G::IW + kx) * 32, pn);
              rd8(reinterpret_cast<const char*>(sv + kx * 64), w01);
              rd8(reinterpret_cast<const char*>(sv + kx * 64 + 32), w12);
#pragma unroll
              for (int e = 0; e < 8; ++e) {   // (row oy + 1 first: its fma reads the shared bias, then dot2c
                a1[e] = fmaf(h_hi(pc[e]), h_lo(w01[e]), a1[e]);   // accumulates in place without a copy)
                a0[e] = dot2h(pc[e], w01[e], a0[e]);
                a0[e] = fmaf(h_lo(pn[e]), h_hi(w12[e]), a0[e]);
                a1[e] = dot2h(pn[e], w12[e], a1[e]);
              }
            }
            bf0 = relu_cvt8<DT>(a0);
            bf1 = relu_cvt8<DT>(a1);
          }
#pragma unroll
          for (int t = 0; t < G::NCTW; ++t) {
            acc[qi][t] = DT::mfma(pa[t], bf0, acc[qi][t]);
            acc[qi + 1][t] = DT::mfma(pa[t], bf1, acc[qi + 1][t]);
          }
        }
      } else {
#pragma unroll
        for (int qi = 0; qi < G::QPW; ++qi) {
          x8 bf;
          {
            float a8[8];
            bias8(a8);
            // stride 2: pair m = oy (rows 2oy, 2oy+1) + low half of m + 1; stride 1 (TW = 16): the wave's row
            const int oy = S == 1 ? __builtin_amdgcn_readfirstlane(oyq[qi]) : oyq[qi];
            const bool odd = S == 1 && (oy & 1);
            const char* pb = er + ((S == 2 ? oy : oy >> 1) * G::IW + S * oxq[qi]) * 32;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
              uint32_t pc[8], pn[8], w01[8], w12[8];
              rd8(pb + kx * 32, pc);
              rd8(pb + (G::IW + kx) * 32, pn);
              rd8(reinterpret_cast<const char*>(sv + kx * 64), w01);
              rd8(reinterpret_cast<const char*>(sv + kx * 64 + 32), w12);
              if (!odd) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                  a8[e] = dot2h(pc[e], w01[e], a8[e]);
                  a8[e] = fmaf(h_lo(pn[e]), h_hi(w12[e]), a8[e]);
                }
              } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                  a8[e] = fmaf(h_hi(pc[e]), h_lo(w01[e]), a8[e]);
                  a8[e] = dot2h(pn[e], w12[e], a8[e]);
                }
              }
            }
            bf = relu_cvt8<DT>(a8);
          }
#pragma unroll
          for (int t = 0; t < G::NCTW; ++t) acc[qi][t] = DT::mfma(pa[t], bf, acc[qi][t]);
        }
      }
    } else if constexpr (G::PAIR && ABL == 0) {
      // Two vertically adjacent output rows per step (tiles qi, qi+1 = rows oy, oy+1 of the same 16 columns):
      // per tap column the 3 weights and the 4 input rows are read once and feed both rows -- 21 instead of
      // 36 ds_read_b128 per 2 x 16 pixels x 8 channels.
#pragma unroll
      for (int qi = 0; qi < G::QPW; qi += 2) {
        x8 bf0, bf1;
        {
          float a0[8], a1[8];
          {
            const float4 u0 = *reinterpret_cast<const float4*>(Bd + 32 * c + 8 * kg);
            const float4 u1 = *reinterpret_cast<const float4*>(Bd + 32 * c + 8 * kg + 4);
            a0[0] = u0.x; a0[1] = u0.y; a0[2] = u0.z; a0[3] = u0.w;
            a0[4] = u1.x; a0[5] = u1.y; a0[6] = u1.z; a0[7] = u1.w;
#pragma unroll
            for (int e = 0; e < 8; ++e) a1[e] = a0[e];
          }
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            DW8<DT> w[3];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) w[ky].load(sl + (ky * 3 + kx) * 32 + 8 * kg);
            x8 v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
              v[r] = *reinterpret_cast<const x8*>(Es + dwoff[qi] + (r * G::IW + kx) * G::ES);
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                a0[e] = fmaf((float)v[ky][e], w[ky][e], a0[e]);
                a1[e] = fmaf((float)v[ky + 1][e], w[ky][e], a1[e]);
              }
          }
          bf0 = relu_cvt8<DT>(a0);
          bf1 = relu_cvt8<DT>(a1);
        }
#pragma unroll
        for (int t = 0; t < G::NCTW; ++t) {
          acc[qi][t] = DT::mfma(pa[t], bf0, acc[qi][t]);
          acc[qi + 1][t] = DT::mfma(pa[t], bf1, acc[qi + 1][t]);
        }
      }
    } else
#pragma unroll
    for (int qi = 0; qi < G::QPW; ++qi) {
      x8 bf;
      {
        float a8[8];
        {
          const float4 u0 = *reinterpret_cast<const float4*>(Bd + 32 * c + 8 * kg);
          const float4 u1 = *reinterpret_cast<const float4*>(Bd + 32 * c + 8 * kg + 4);
          a8[0] = u0.x; a8[1] = u0.y; a8[2] = u0.z; a8[3] = u0.w;
          a8[4] = u1.x; a8[5] = u1.y; a8[6] = u1.z; a8[7] = u1.w;
        }
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
          for (int ky = 0; ky < 3; ++ky) {
            if (ABL == 1 && !(ky == 1 && kx == 1)) continue;
            const x8 v = *reinterpret_cast<const x8*>(Es + dwoff[qi] + (ky * G::IW + kx) * G::ES);
            DW8<DT> wt;   // fp16 weights: one ds_read_b128 per tap, consumed by v_fma_mix directly
            wt.load(sl + (ky * 3 + kx) * 32 + 8 * kg);
#pragma unroll
            for (int e = 0; e < 8; ++e) a8[e] = fmaf((float)v[e], wt[e], a8[e]);
          }
        bf = relu_cvt8<DT>(a8);
      }
#pragma unroll
      for (int t = 0; t < G::NCTW; ++t) {
        if constexpr (ABL == 4) acc[qi][t][0] += (float)bf[t & 7];
        else acc[qi][t] = DT::mfma(pa[t], bf, acc[qi][t]);
      }
    }
    // next chunk's depthwise weights: buffer (c+1)&1 was last read by dw(c-1), which every wave finished
    // before the barrier of this chunk; the barrier of chunk c+1 publishes it before dw(c+1) reads it.
    slab_store(c + 1, slab_next);
  }

  // ---- 5. epilogue: + bias (+ residual from the staged input tile) -> y (NHWC)
#pragma unroll
  for (int qi = 0; qi < G::QPW; ++qi) {
    const int oy = oyq[qi], ox = oxq[qi];
    const int gy = oy0 + oy, gx = ox0 + ox;
    if (gy >= OH || gx >= OW) continue;
    T* yr = Y + (((size_t)b * OH + gy) * OW + gx) * COUT;
#pragma unroll
    for (int t = 0; t < G::NCTW; ++t) {
      const int co = (wc * G::NCTW + t) * 16 + 4 * kg;
      if (co >= COUT) continue;
      f32x4 v = acc[qi][t];
      if constexpr (RES) {
        const x4 r = *reinterpret_cast<const x4*>(Xs + ((oy + 1) * G::IW + (ox + 1)) * G::XS + co);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += (float)r[e];
      }
      x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (T)v[e];
      if constexpr (G::NT_Y)   // (block 7: measured -4 us; elsewhere the consumer reads the map from the caches)
        SPEF_KB_YSTORE(__builtin_nontemporal_store(o, reinterpret_cast<x4*>(yr + co)), o);
      else
        SPEF_KB_YSTORE(*reinterpret_cast<x4*>(yr + co) = o, o);
    }
  }
  SPEF_TRACE(SPEF_TRACE_SLOTS - 1);
}

// ------------------------------------------------------------------------------------------ dispatch
// One instantiation per MobileNet-V2 block geometry: (cin, hidden, cout, stride, tile TH x TW, expand,
// residual, waves, cout groups). Unknown geometries return hipErrorNotSupported -> the executor falls back
// to the unfused kernels.
// Variant 0 is the default; variants >= 1 are alternatives for tuning sweeps (spef_set_option
// SPEF_OPT_IRB_VARIANT); a geometry without the requested variant uses variant 0.
#define SPEF_IRB_TABLE(X)                                                   \
  X(0, 32, 32, 16, 1, 16, 16, false, false, 8, 1, true, false)    /* block 1      */ \
  X(0, 16, 96, 24, 2, 4, 16, true, false, 4, 1, false, false)     /* block 2      */ \
  X(2, 16, 96, 24, 2, 8, 16, true, false, 8, 1, false, false)                        \
  X(0, 24, 144, 24, 1, 16, 16, true, true, 4, 1, false, false)    /* block 3      */ \
  X(1, 24, 144, 24, 1, 8, 16, true, true, 8, 1, false, false)                        \
  X(2, 24, 144, 24, 1, 8, 16, true, true, 4, 1, false, false)                        \
  X(0, 24, 144, 32, 2, 8, 8, true, false, 4, 1, false, false)     /* block 4      */ \
  X(2, 24, 144, 32, 2, 8, 16, true, false, 8, 1, false, false)                       \
  X(0, 32, 192, 32, 1, 8, 16, true, true, 4, 1, false, false)     /* blocks 5-6   */ \
  X(1, 32, 192, 32, 1, 16, 16, true, true, 8, 1, false, false)                       \
  X(0, 32, 192, 64, 2, 8, 8, true, false, 4, 1, false, false)     /* block 7      */ \
  X(1, 32, 192, 64, 2, 8, 8, true, false, 8, 2, false, false)                        \
  X(2, 32, 192, 64, 2, 8, 16, true, false, 8, 1, false, false)                       \
  X(0, 64, 384, 64, 1, 16, 16, true, true, 8, 1, true, true)      /* blocks 8-10  */ \
  X(1, 64, 384, 64, 1, 8, 16, true, true, 8, 1, false, true)                         \
  X(2, 64, 384, 64, 1, 16, 16, true, true, 8, 1, false, true)                        \
  X(3, 64, 384, 64, 1, 8, 16, true, true, 4, 1, false, true)                         \
  X(0, 64, 384, 96, 1, 16, 16, true, false, 8, 1, false, true)     /* block 11     */ \
  X(2, 64, 384, 96, 1, 8, 16, true, false, 8, 1, true, true)                       \
  X(0, 96, 576, 96, 1, 16, 16, true, true, 8, 1, false, true)     /* blocks 12-13 */ \
  X(1, 96, 576, 96, 1, 8, 16, true, true, 8, 1, true, true)                          \
  X(2, 96, 576, 96, 1, 16, 16, true, true, 8, 2, false, true)                        \
  X(0, 96, 576, 160, 2, 8, 8, true, false, 8, 2, false, true)     /* block 14     */ \
  X(2, 96, 576, 160, 2, 4, 8, true, false, 4, 2, true, false)                        \
  X(0, 160, 960, 160, 1, 8, 8, true, true, 8, 2, true, true)      /* blocks 15-16 */ \
  X(2, 160, 960, 160, 1, 4, 8, true, true, 4, 2, true, true)                       \
  X(0, 160, 960, 320, 1, 8, 8, true, false, 8, 2, false, true)    /* block 17     */ \
  X(2, 160, 960, 320, 1, 4, 8, true, false, 4, 2, true, true)

template <typename DT, int CIN, int HID, int COUT, int S, int TH, int TW, bool EXPAND, bool RES, int NW, int WCO,
          bool DBUF, bool STW, int ABL = 0>
static hipError_t irb_go(const void* x, const void* we, const float* be, const void* wd, const float* bd,
                         const void* wp, const float* bp, void* y, int B, int H, int W, int OH, int OW,
                         hipStream_t s) {
  using DW = typename DT::DW;
  constexpr bool VP = irb_vp(std::is_same<DT, F16>::value, HID, EXPAND, S) && ABL == 0;
  constexpr bool PKU = irb_pku(irb_pk(std::is_same<DT, F16>::value, HID, EXPAND, S) && ABL == 0, NW, DBUF, STW, S, TH, TW);
  using G = IrbGeom<CIN, HID, COUT, S, TH, TW, EXPAND, RES, NW, WCO, DBUF, STW, (int)sizeof(DW), VP, PKU>;
  using T = typename DT::T;
  TileGrid g;
  hipError_t e = tile_grid(g, OH, OW, TH, TW, B);
  if (e != hipSuccess) return e;
  auto k = irb_kernel<DT, CIN, HID, COUT, S, TH, TW, EXPAND, RES, NW, WCO, DBUF, STW, ABL>;
  static DevOnce attr_set;
  if ((e = lds_attr_once(attr_set, k, G::LDS_BYTES)) != hipSuccess) return e;
  k<<<g.nwg, NW * 64, G::LDS_BYTES, s>>>((const T*)x, (const T*)we, be, (const DW*)wd, bd, (const T*)wp, bp, (T*)y, H, W,
                                         OH, OW, g.tiles_x, g.tiles_y, g.nwg);
  return hipGetLastError();
}

static bool irb_has(int variant, int cin, int hid, int cout, int stride, bool expand, bool res) {
#define SPEF_IRB_HAS(V, CI, HI, CO, ST, TH_, TW_, EX, RS, NW_, WC_, DB_, SW_) \
  if (variant == V && cin == CI && hid == HI && cout == CO && stride == ST && expand == EX && res == RS) return true;
  SPEF_IRB_TABLE(SPEF_IRB_HAS)
#undef SPEF_IRB_HAS
  return false;
}

template <typename DT>
// timing ablations of the variant-0 configurations (tools/explore.py ABL=1): variant 100 + 10 * ABL
#define SPEF_IRB_ABL(X)                                                                                      \
  X(1, 24, 144, 24, 1, 16, 16, true, true, 4, 1, false, false) X(2, 24, 144, 24, 1, 16, 16, true, true, 4, 1, false, false) \
  X(3, 24, 144, 24, 1, 16, 16, true, true, 4, 1, false, false) X(4, 24, 144, 24, 1, 16, 16, true, true, 4, 1, false, false) \
  X(1, 96, 576, 96, 1, 16, 16, true, true, 8, 1, false, true) X(2, 96, 576, 96, 1, 16, 16, true, true, 8, 1, false, true) \
  X(3, 96, 576, 96, 1, 16, 16, true, true, 8, 1, false, true) X(4, 96, 576, 96, 1, 16, 16, true, true, 8, 1, false, true) \
  X(1, 16, 96, 24, 2, 4, 16, true, false, 4, 1, false, false) X(2, 16, 96, 24, 2, 4, 16, true, false, 4, 1, false, false) \
  X(3, 16, 96, 24, 2, 4, 16, true, false, 4, 1, false, false) X(4, 16, 96, 24, 2, 4, 16, true, false, 4, 1, false, false) \
  X(5, 96, 576, 96, 1, 16, 16, true, true, 8, 1, false, true) X(6, 96, 576, 96, 1, 16, 16, true, true, 8, 1, false, true) \
  X(7, 96, 576, 96, 1, 16, 16, true, true, 8, 1, false, true) X(5, 24, 144, 24, 1, 16, 16, true, true, 4, 1, false, false)

static hipError_t irb_dispatch(int variant, int cin, int hid, int cout, int stride, bool expand, bool res,
                               const void* x, const void* we, const float* be, const void* wd, const float* bd,
                               const void* wp, const float* bp, void* y, int B, int H, int W, int OH, int OW,
                               hipStream_t s) {
  if (variant >= 100) {
    const int abl = (variant - 100) / 10;
#define SPEF_IRB_ABL_CASE(A, CI, HI, CO, ST, TH_, TW_, EX, RS, NW_, WC_, DB_, SW_)                         \
    if (abl == A && cin == CI && hid == HI && cout == CO && stride == ST && expand == EX && res == RS)      \
      return irb_go<DT, CI, HI, CO, ST, TH_, TW_, EX, RS, NW_, WC_, DB_, SW_, A>(x, we, be, wd, bd, wp, bp, y, B, H, \
                                                                             W, OH, OW, s);
    SPEF_IRB_ABL(SPEF_IRB_ABL_CASE)
#undef SPEF_IRB_ABL_CASE
    variant = 0;
  }
  const bool lib_default = variant < 0;   // SPEF_OPT_IRB_VARIANT unset (an explicit 0 from a sweep stays 0)
  if (!irb_has(variant, cin, hid, cout, stride, expand, res)) variant = 0;
  // Blocks 5-6 take the 16x16 / 8-wave tiles (variant 1) where those tile the map exactly (64x64 at 512^2): pipelined
  // bench 94.6k -> 95.2k img/s (interleaved, 5 pairs); on maps they do not divide, the 8x16 / 4-wave tiles. Only as
  // the library default, and only where variant 1 exists for the full geometry (expand and residual included).
  if (lib_default && irb_has(1, cin, hid, cout, stride, expand, res) && cin == 32 && hid == 192 && cout == 32 &&
      stride == 1 && OH % 16 == 0 && OW % 16 == 0)
    variant = 1;
#define SPEF_IRB_CASE(V, CI, HI, CO, ST, TH_, TW_, EX, RS, NW_, WC_, DB_, SW_)                            \
  if (variant == V && cin == CI && hid == HI && cout == CO && stride == ST && expand == EX && res == RS)   \
    return irb_go<DT, CI, HI, CO, ST, TH_, TW_, EX, RS, NW_, WC_, DB_, SW_>(x, we, be, wd, bd, wp, bp, y, B, H, W, \
                                                                           OH, OW, s);
  SPEF_IRB_TABLE(SPEF_IRB_CASE)
#undef SPEF_IRB_CASE
  return hipErrorNotSupported;
}

int irb_dw_mode(int dtype, int hid, bool expand, int stride) {
  return irb_vp(dtype == DT_F16, hid, expand, stride) ? DW_PAIRS
         : irb_pk(dtype == DT_F16, hid, expand, stride) ? DW_PK16 : DW_FP32;
}

bool irb_supported(int cin, int hid, int cout, int stride, bool expand, bool res) {
  return irb_has(0, cin, hid, cout, stride, expand, res);
}

hipError_t launch_irb(int variant, int dtype, int cin, int hid, int cout, int stride, bool expand, bool res,
                      const void* x, const void* we, const float* be, const void* wd, const float* bd, const void* wp,
                      const float* bp, void* y, int B, int H, int W, int OH, int OW, hipStream_t s) {
  return dtype == DT_F16 ? irb_dispatch<F16>(variant, cin, hid, cout, stride, expand, res, x, we, be, wd, bd, wp, bp,
                                             y, B, H, W, OH, OW, s)
                         : irb_dispatch<BF16>(0, cin, hid, cout, stride, expand, res, x, we, be, wd, bd, wp, bp, y, B,
                                              H, W, OH, OW, s);
}

}  // namespace spef
