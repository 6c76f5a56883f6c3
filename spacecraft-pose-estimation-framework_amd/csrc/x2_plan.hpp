// Which fused kernel an fp16x2 / fp16mx inverted-residual block runs on: the tile tables and the one function that
// searches them. Plain C++ (no HIP types), so a host compiler builds it alone (tools/x2_plan_dump.cpp,
// tests/test_x2_plan.py); the launchers (x2_dispatch.cpp, k_x2_irb.hip, k_x2_irw.hip, k_x2_irp.hip) map a plan to
// the template instantiation of its table row.
#pragma once
#include <stdint.h>

namespace spef {

// (cin, hidden, cout, stride, expand, residual, TH, TW, waves, cout groups, kind): MobileNet-V2's 17 blocks
// (mobilenet_v2.py:240-249). kind 0: slab kernel with `waves` waves (tiles keep the hi / lo input tile + fp32 slab at
// 2+ workgroups per CU where the geometry allows); kind 1: role-split kernel (4 + 4 waves) with the project weights
// staged in LDS; kind 2: role-split, project weights from L2 (block 17: no two depthwise waves share a channel tile).
// Cout groups: with g groups the depthwise waves split into g sets that each run the whole depthwise for their pixels
// and project onto 1/g of the output channels, so g > 1 computes the depthwise g times. Interleaved A/B at B = 64
// (tools/x2_ab.sh, per launch): blocks 8-10 81 -> 54 us and block 11 84 -> 59 us with g 2 -> 1; blocks 12-13 158
// (8x8, g 2) -> 125 (8x16, g 2) -> 89 us (8x16, g 1); blocks 15-16 93 -> 91 us (g 2 -> 1); block 17 142 us at g 4,
// 125 at g 2, 322 at g 1 (80 accumulator registers per wave: spills). URSONet step 2.11 -> 1.85 ms, keypoint mode
// 1.27 -> 1.05 ms (with the small-map table below).
// Kind 3 = kind 1 with persistent tiles (x2_irw_kernel's PT: a second tile per CU streams on without a prologue):
// the maps with more tiles than CUs at 512^2 (blocks 8-14: 512 tiles at B = 64). Kind 5 / 6: the three-stage kernel
// (x2_irp_kernel) without / with persistent tiles. Measured per step at B = 64 (tools/ktime.sh, bit-identical
// outputs): blocks 15-16 131.4 -> 101.9 us on kind 5, blocks 12-13 147.9 -> 142.0 and block 11 51.8 -> 49.1 on kind
// 6; blocks 8-10 130.7 -> 138.5 on kind 6 (their VALU role is the longer one there), so they stay on kind 3.
// Kind 3 launches x2_irw_st_kernel (the role-split kernel with the three-stage kernel's staging: LDS-DMA into static
// double buffers, in flight across the chunk barrier) unless SPEF_OPT_X2_STAGE is 0; same row, same profile key.
// Interleaved on one engine at B = 64 (tools/trim_ab.py 0 1 6 10): blocks 8-10 126.7-127.8 -> 114.0-114.6 us per step,
// block 14 63.6-64.1 -> 54.4-54.7.
#define SPEF_X2_MID(X)                                           \
  X(64, 384, 64, 1, true, true, 8, 16, 8, 1, 3)      /* 8-10 */   \
  X(64, 384, 96, 1, true, false, 8, 16, 8, 1, 6)     /* 11 */     \
  X(96, 576, 96, 1, true, true, 8, 16, 8, 1, 6)      /* 12-13 */
#define SPEF_X2_TABLE(X)                                         \
  X(32, 32, 16, 1, false, false, 8, 16, 4, 1, 0)    /* 1 */      \
  X(16, 96, 24, 2, true, false, 8, 8, 4, 1, 0)      /* 2 */      \
  X(24, 144, 24, 1, true, true, 8, 16, 4, 1, 0)     /* 3 */      \
  X(24, 144, 32, 2, true, false, 8, 8, 4, 1, 0)     /* 4 */      \
  X(32, 192, 32, 1, true, true, 8, 16, 4, 1, 0)     /* 5-6 */    \
  X(32, 192, 64, 2, true, false, 8, 8, 4, 1, 0)     /* 7 */      \
  SPEF_X2_MID(X)                                                 \
  X(96, 576, 160, 2, true, false, 4, 8, 8, 2, 3)    /* 14 */     \
  X(160, 960, 160, 1, true, true, 8, 8, 8, 1, 5)    /* 15-16 */  \
  X(160, 960, 320, 1, true, false, 8, 8, 8, 1, 5)    /* 17 */
// 16x16 tiles with 8 waves (2 workgroups per CU) where they tile the map exactly: block 3 at 512^2 (interleaved A/B,
// round 4: 165 -> 153 us per step); on maps they do not divide (60x96, 30x48 at 240x384) the partial tiles cost more
// than the occupancy gains. Blocks 5-6 left this table in round 5: behind the fp16mx front end 8 x 16 tiles measured
// 139 -> 117 us per step (round 4, fp16x2: 119 -> 115 the other way).
#define SPEF_X2_EXACT_TABLE(X)                                      \
  X(24, 144, 24, 1, true, true, 16, 16, 8, 1, 0)     /* 3 */
// Maps whose primary tiling leaves CUs idle (fewer workgroups than CUs; the role-split kernels run one workgroup
// per CU): blocks 15-17 at 240x384 (8x12 maps: 128 workgroups of 8x8 at B = 64) split the hidden dimension over P
// workgroups per tile (last field; partial sums joined by x2_split_reduce_kernel in the caller's scratch).
#define SPEF_X2_SMALL_TABLE(X)                                      \
  X(160, 960, 160, 1, true, true, 8, 8, 8, 1, 1, 2)    /* 15-16 */  \
  X(160, 960, 320, 1, true, false, 8, 8, 8, 2, 2, 2)   /* 17 */
#ifndef SPEF_X2_EXACT_ON   // A/B aid: 0 = the primary 8 x 16 tiles on exact maps too
#define SPEF_X2_EXACT_ON 1
#endif


struct X2Block {   // an inverted residual's geometry, as the tables key it
  int cin, hid, cout, stride;
  bool expand, res;
  bool is(int ci, int hi, int co, int st, bool ex, bool rs) const {
    return cin == ci && hid == hi && cout == co && stride == st && expand == ex && res == rs;
  }
};

struct X2Plan {
  bool known = false;   // the geometry has a row (every small-map and exact row's geometry is in the primary table too)
  bool found = false;   // ... and that row's kernel takes the block I/O: fp16 I/O (io != 0) is the slab kernel's only
  int kind = 0, TH = 0, TW = 0, NW = 0, WCO = 0, P = 0;   // the row: kernel kind, tile, waves, cout groups, hidden parts
  bool is(int kd, int th, int tw, int nw, int wc, int p) const {
    return kind == kd && TH == th && TW == tw && NW == nw && WCO == wc && P == p;
  }
  // profiling label; nullptr when no kernel runs
  const char* kernel_name() const {
    return !found ? nullptr : kind == 0 ? "x2_irb_kernel" : kind >= 5 ? "x2_irp_kernel" : "x2_irw_kernel";
  }
};

// The row a block runs on. B images of OH x OW output pixels; scratch: the caller has the hidden-split form's
// partial-sum buffer; io: bit 0 = fp16 input, bit 1 = fp16 output; num_cu: the device's compute units. First the
// small-map table (needs scratch and fp32 I/O; the 8 x 8 tiling leaves CUs idle and the row's tiles x parts fit the
// CUs), then the exact table (the tile divides the map), then the primary table.
inline X2Plan x2_irb_plan(const X2Block& b, int B, int OH, int OW, bool scratch, int io, int num_cu) {
  auto tiles = [&](int th, int tw) { return (int64_t)((OW + tw - 1) / tw) * ((OH + th - 1) / th) * B; };
  auto row = [&](int kd, int th, int tw, int nw, int wc, int p) {
    return X2Plan{true, kd == 0 || io == 0, kd, th, tw, nw, wc, p};
  };
#define SPEF_X2_SMALL(CI, HI, CO, ST, EX, RS, TH_, TW_, NW_, WC_, KD_, P_)                                  \
  if (b.is(CI, HI, CO, ST, EX, RS) && scratch && !io && tiles(8, 8) < num_cu && tiles(TH_, TW_) * P_ <= num_cu) \
    return row(KD_, TH_, TW_, NW_, WC_, P_);
  SPEF_X2_SMALL_TABLE(SPEF_X2_SMALL)
#undef SPEF_X2_SMALL
#define SPEF_X2_EXACT(CI, HI, CO, ST, EX, RS, TH_, TW_, NW_, WC_, KD_)                     \
  if (SPEF_X2_EXACT_ON && b.is(CI, HI, CO, ST, EX, RS) && OH % (TH_) == 0 && OW % (TW_) == 0) \
    return row(KD_, TH_, TW_, NW_, WC_, 1);
  SPEF_X2_EXACT_TABLE(SPEF_X2_EXACT)
#undef SPEF_X2_EXACT
#define SPEF_X2_PRIMARY(CI, HI, CO, ST, EX, RS, TH_, TW_, NW_, WC_, KD_) \
  if (b.is(CI, HI, CO, ST, EX, RS)) return row(KD_, TH_, TW_, NW_, WC_, 1);
  SPEF_X2_TABLE(SPEF_X2_PRIMARY)
#undef SPEF_X2_PRIMARY
  return X2Plan{};
}

// A table row's constants as a type, and the one walk from a block and its plan to them: f(X2Row<...>{}) for the plan's
// row where its kind is in [K0, K1] -- a kernel family's launcher instantiates the rows of its own kinds only -- else
// `none`. (The small-map rows' parts P are the macro's `...`; x2_row_parts() = 1 for the rows that have none.)
template <int CIN, int HID, int COUT, int S, bool EXPAND, bool RES, int TH, int TW, int NW, int WCO, int KIND, int P>
struct X2Row {};
constexpr int x2_row_parts(int p = 1) { return p; }
template <int K0, int K1, typename R, typename F>
R x2_visit_row(const X2Block& b, const X2Plan& p, R none, F f) {
#define SPEF_X2_ROW(CI, HI, CO, ST, EX, RS, TH_, TW_, NW_, WC_, KD_, ...)                          \
  if constexpr (KD_ >= K0 && KD_ <= K1)                                                          \
    if (b.is(CI, HI, CO, ST, EX, RS) && p.is(KD_, TH_, TW_, NW_, WC_, x2_row_parts(__VA_ARGS__))) \
      return f(X2Row<CI, HI, CO, ST, EX, RS, TH_, TW_, NW_, WC_, KD_, x2_row_parts(__VA_ARGS__)>{});
  SPEF_X2_SMALL_TABLE(SPEF_X2_ROW) SPEF_X2_EXACT_TABLE(SPEF_X2_ROW) SPEF_X2_TABLE(SPEF_X2_ROW)
#undef SPEF_X2_ROW
  return none;
}

// Persistent tiles (kinds 3 and 6): ceil(tiles / CUs) tiles per workgroup, and as many workgroups as that needs.
inline uint32_t x2_persistent_grid(uint32_t nwg, int num_cu) {
  const uint32_t per = (nwg + (uint32_t)num_cu - 1) / (uint32_t)num_cu;
  return (nwg + per - 1) / per;
}

}  // namespace spef
