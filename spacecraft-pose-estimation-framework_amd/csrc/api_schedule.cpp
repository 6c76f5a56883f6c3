// The layer executor and its entry points (include/spef.h: forward, backbone, probe, observe).
//
// A scheduler walks the blob's op list (stem -> 17 inverted residuals -> last 1x1 -> head) over four NHWC activation
// buffers sized at spef_reserve time, and decides which kernel runs for every op. run_backbone is the float one; it
// only walks, and calls one step function per stage and schedule family:
//   stem       front_step (uint8 frames, fused with block 1: fp16 / bf16, fp16x2, fp16mx) | stem_step
//   blocks     irb_step_x2 (fp16x2 / fp16mx: always fused) | irb_step_fused16 (fp16 / bf16) | irb_step_unfused (fp32,
//              and fp16 / bf16 with SPEF_OPT_FUSE_BLOCKS=0 or below SPEF_OPT_FUSE_MIN_HW; bit-identical)
//   last conv  last_step: fused with the global mean where the family has such a kernel, else conv (+ mean_hw)
// run_backbone_q8 is the int8 one (one family, fused or one kernel per conv).
#include <math.h>

#include <initializer_list>

#include "spef_ctx.hpp"

namespace {

// The activation a scheduler has reached: buffer, NHWC geometry, and whether it is stored fp16 (fp16mx: blocks 1-3).
struct Act {
  void* p;
  int h, w, ch;
  bool f16;
};

inline void advance(Act& a, void* y, int h, int w, uint32_t ch, bool f16 = false) { a = Act{y, h, w, (int)ch, f16}; }

// A workspace buffer that none of `busy` occupies.
void* free_buf(const spef_ctx* c, std::initializer_list<const void*> busy) {
  for (void* b : c->buf) {
    bool used = false;
    for (const void* u : busy) used |= (u == b);
    if (!used) return b;
  }
  return nullptr;
}

// The six tensors of an op as the float launchers take them (w1 is fp32 for fp16x2 / fp16mx: cast at the call).
struct Wts {
  const void *w0, *w1, *w2;
  const float *b0, *b1, *b2;
};
Wts weights(const spef_ctx* c, const OpDesc& op) {
  return {ptr<void>(c, op.w0), ptr<void>(c, op.w1), ptr<void>(c, op.w2),
          ptr<float>(c, op.b0), ptr<float>(c, op.b1), ptr<float>(c, op.b2)};
}

hipError_t pw_any(spef_ctx* c, int dt, int epi, const void* x, const void* wt, const float* bias, const void* r,
                  void* y, int64_t M, int K, int N, hipStream_t s) {
  if (dt == DT_F32) return launch_gemm_f32(epi, x, wt, bias, r, y, M, K, N, s);
  return c->gemm ? launch_gemm_pw(dt, epi, x, wt, bias, r, y, M, K, N, s)
                 : launch_pw(dt, epi, x, wt, bias, r, y, M, K, N, s);
}

const char* pw_key(int dt, int epi, int N) {
  // mirrors pw_dispatch's tile choice so keys name the kernel instantiation rocprof reports
  static thread_local std::string k;
  const int n16 = ((N + 15) & ~15) / 16;
  int nt = 1, mt = 4;
  if (n16 == 1) { nt = 1; mt = 4; }
  else if (n16 == 2) { nt = 2; mt = 4; }
  else if (n16 == 4) { nt = 4; mt = 4; }
  else if (n16 % 6 == 0) { nt = 6; mt = 2; }
  else if (n16 % 5 == 0) { nt = 5; mt = 2; }
  else if (n16 % 4 == 0) { nt = 4; mt = 4; }
  else if (n16 % 3 == 0) { nt = 3; mt = 4; }
  else if (n16 % 2 == 0) { nt = 2; mt = 4; }
  k = std::string("pw_kernel<") + (dt == DT_F16 ? "F16" : "BF16") + "," + std::to_string(nt) + "," +
      std::to_string(mt) + "," + std::to_string(epi) + ">";
  return k.c_str();
}

const char* pw_any_key(spef_ctx* c, int dt, int epi, int N) {
  if (dt == DT_F32) return gemm_f32_key(N);
  return c->gemm ? gemm_key(dt, epi, N) : pw_key(dt, epi, N);
}

// algorithmic HBM bytes of one pointwise launch: read X, write Y (+ read residual), weights + bias once
double pw_bytes(int64_t M, uint32_t K, uint32_t N, bool res) {
  const double kp = (K + 31) & ~31u, np_ = (N + 15) & ~15u;
  return (double)M * K * 2 + (double)M * N * 2 * (res ? 2 : 1) + np_ * kp * 2 + np_ * 4;
}

// One run of the float scheduler: the call's arguments and the schedule family of the loaded blob.
// mode: 0 = full (pool into c->pooled), 1 = stop after op `stop`, 2 = unfused last conv (fp32 map into feat_f32 where
// given, else into a workspace buffer).
struct Run {
  spef_ctx* c;
  hipStream_t s;
  const void* input;
  int layout, B, mode, stop;
  float* feat_f32;
  const spef_observer* obs;   // fp32 schedule only: after each launch the observer is enqueued on the buffer just
                              // written (spef_amd.quant.calibrate's taps; spef_observe)
  int dt;
  bool f32;    // fp32 schedule: one kernel per conv (k_f32.hip), no fused kernels
  bool x2;     // fp16x2 kernels: fused split-fp16 blocks (k_x2_*.hip)
  bool mx;     // fp16mx: the same weights; the block outputs with <= 24 channels (blocks 1-3: the 256^2 / 128^2 maps,
               // DESIGN.md section 5) are stored fp16, every other block output fp32
  double es;   // activation bytes per element (profiler byte counts)
  bool out16(const OpDesc& o) const { return mx && o.cout <= 24; }
};

hipError_t observe(const Run& r, int tap, const void* p, int64_t n, bool u8 = false) {
  const int obs_blocks = num_cus() * 5;   // 32 KiB of LDS each: five workgroups per CU
  return prof_launch(r.c, r.s, u8 ? "observe_kernel<u8>" : "observe_kernel<f32>", (double)n * (u8 ? 1 : 4), 0.0, [&] {
    return launch_observe(r.obs->tap(tap), p, n, u8, obs_blocks, r.s);
  });
}

// One profiled 1x1 conv of the one-kernel-per-conv schedule: y [M][N] = epi(x [M][K] * wt + bias (+ res)).
hipError_t pw_launch(const Run& r, int epi, const void* x, const void* wt, const float* bias, const void* res, void* y,
                     int64_t M, uint32_t K, uint32_t N) {
  return prof_launch(r.c, r.s, pw_any_key(r.c, r.dt, epi, N), pw_bytes(M, K, N, res != nullptr) * r.es / 2,
                     2.0 * M * K * N, [&] {
    return pw_any(r.c, r.dt, epi, x, wt, bias, res, y, M, (int)K, (int)N, r.s);
  });
}

// ---------------------------------------------------------------------------------------------------- stem
// The stem and block 1 run as one front kernel: a fused family, uint8 frames, the block-1 geometry the kernels are
// built for, and the caller does not want the stem's own output.
bool front_fusable(const Run& r, const OpDesc& op, const OpDesc* nx) {
  return !r.f32 && r.c->fuse && r.layout == IN_U8_NHWC && !(r.mode == 1 && r.stop == 0) && nx && nx->kind == OP_IRB &&
         nx->cin == 32 && nx->hidden == 32 && nx->cout == 16 && nx->expand == 1 && nx->stride == 1 && op.cout == 32 &&
         op.x0 != kAbsent;
}

// fp16 / bf16: front_kernel. fp16x2 / fp16mx: stem (MFMA, exact u8 operand) + block 1 in one kernel, fp32 (fp16mx:
// fp16) output.
int front_step(const Run& r, const OpDesc& op, const OpDesc& nx, Act& a) {
  spef_ctx* c = r.c;
  hipStream_t s = r.s;
  const int B = r.B, h = a.h, w = a.w, OH = conv_out(h, 2), OW = conv_out(w, 2);
  void* y = c->buf[0];
  const double px = (double)B * OH * OW;
  const bool o16 = r.out16(nx);
  const bool mxf = r.mx && o16 && c->mx_kernels && op.x1 != kAbsent;
  const Wts b1 = weights(c, nx);
  const float* bs = ptr<float>(c, op.b0);
  const char* key = !r.x2 ? "front_kernel<stem+block1>"
                           : mxf ? "mx_front_kernel<stem+block1>" : "x2_front_kernel<stem+block1>";
  HIP_TRY(prof_launch(c, s, key, (double)B * h * w * 3 + px * 16 * ((r.x2 && !o16) ? 4 : 2),
                      px * (2 * 27 * 32 + 18 * 32 + 2 * 32 * 16), [&] {
    if (!r.x2)
      return launch_front(r.dt, r.input, ptr<void>(c, op.x0), bs, b1.w1, b1.b1, b1.w2, b1.b2, y, B, h, w, OH, OW, s);
    if (mxf)
      return launch_mx_front(r.input, ptr<void>(c, op.x1), bs, (const float*)b1.w1, b1.b1, b1.w2, b1.b2, y, B, h, w, OH,
                             OW, s);
    return launch_x2_front(r.input, ptr<void>(c, op.x0), bs, (const float*)b1.w1, b1.b1, b1.w2, b1.b2, y, B, h, w, OH,
                           OW, s, o16);
  }));
  advance(a, y, OH, OW, nx.cout, o16);
  return SPEF_OK;
}

int stem_step(const Run& r, const OpDesc& op, Act& a) {
  spef_ctx* c = r.c;
  hipStream_t s = r.s;
  const int B = r.B, h = a.h, w = a.w, OH = conv_out(h, 2), OW = conv_out(w, 2);
  void* y = c->buf[0];
  const double px = (double)B * OH * OW;
  const double in_b = (double)B * h * w * 3 * (r.layout == IN_U8_NHWC ? 1 : 4);
  if (r.obs) HIP_TRY(observe(r, 0, r.input, (int64_t)B * h * w * 3, r.layout == IN_U8_NHWC));
  HIP_TRY(prof_launch(c, s, r.layout == IN_U8_NHWC ? "stem_kernel<u8>" : "stem_kernel<f32>",
                      in_b + px * 32 * r.es, px * 2 * 27 * 32, [&] {
    return launch_stem(r.x2 ? (int)DT_F32 : r.dt, r.layout, r.input, ptr<float>(c, op.w0), ptr<float>(c, op.b0), y, B,
                       h, w, OH, OW, s);
  }));
  if (r.obs) HIP_TRY(observe(r, 1, y, (int64_t)B * OH * OW * op.cout));
  advance(a, y, OH, OW, op.cout);
  return SPEF_OK;
}

// ---------------------------------------------------------------------------------------------------- blocks
// One inverted residual at the cursor: the op's geometry as the launchers take it, and the batch's pixel counts.
struct Block {
  int cin, hid, cout, stride;
  bool expand, res;
  int OH, OW;
  int64_t M, M2;   // input / output pixels of the batch
  Block(const OpDesc& op, int B, const Act& a)
      : cin((int)op.cin), hid((int)op.hidden), cout((int)op.cout), stride((int)op.stride), expand(op.expand != 1),
        res(op.flags & 1u), OH(conv_out(a.h, stride)), OW(conv_out(a.w, stride)), M((int64_t)B * a.h * a.w),
        M2((int64_t)B * OH * OW) {}
};

// flops of a fused block: expand (where there is one), depthwise, project
double irb_flops(const OpDesc& op, const Block& g) {
  return 2.0 * g.M * op.cin * op.hidden * (g.expand ? 1 : 0) + 18.0 * g.M2 * op.hidden +
         2.0 * g.M2 * op.hidden * op.cout;
}

// fp16x2 / fp16mx: one fused kernel per block, no unfused form.
int irb_step_x2(const Run& r, const OpDesc& op, const Block& g, Act& a) {
  spef_ctx* c = r.c;
  hipStream_t s = r.s;
  const int B = r.B, h = a.h, w = a.w, OH = g.OH, OW = g.OW;
  void* x = a.p;
  const bool cur16 = a.f16;
  void* y = free_buf(c, {x});
  const double hp = (op.hidden + 31) & ~31u;
  const bool o16 = r.out16(op);
  const int io = (cur16 ? 1 : 0) | (o16 ? 2 : 0);
  // a third activation buffer (each holds the largest map) is the hidden-split form's partial-sum scratch
  float* scratch = (float*)free_buf(c, {x, y});
  // one plan: the support check, the profiling label and the launch all read it
  const X2Block blk{g.cin, g.hid, g.cout, g.stride, g.expand, g.res};
  const int cus = num_cus();
  const X2Plan plan = x2_irb_plan(blk, B, OH, OW, scratch != nullptr, io, cus);
  if (!plan.known) return fail(SPEF_ERR_ARG, "fp16x2 schedule: unsupported inverted-residual geometry");
  const double ib = cur16 ? 2 : 4, ob = o16 ? 2 : 4;
  // compulsory bytes: the block input once (a stride-1 residual IS that input: not counted twice), the output,
  // the weights once (the fp16 formula of irb_step_fused16 counts the same way)
  const double bytes = (double)g.M * op.cin * ib + (double)g.M2 * op.cout * ob +
                       (g.expand ? hp * ((op.cin + 31) & ~31u) * 4 : 0) + hp * 48 +
                       ((op.cout + 15) & ~15u) * (hp * 4 + 4);
  char key[96];
  const bool mxk = r.mx && c->mx_kernels &&
                   mx_irb_supported(g.cin, g.hid, g.cout, g.stride, g.expand, g.res, cur16, o16);
  // "_wide": the lean set-up was asked for and a map is too large for its 32-bit offsets
  const bool mxlean = (c->trim & 2) != 0;
  const char* kn = mxk ? (mxlean && !mx_irb_lean_fits(g.cin, g.cout, o16, h, w, OH, OW) ? "mx_irb_kernel_wide"
                                                                                       : "mx_irb_kernel")
                       : plan.kernel_name();
  snprintf(key, sizeof(key), "%s<%u,%u,%u,s%u>", kn ? kn : "x2_irb_kernel", op.cin, op.hidden, op.cout, op.stride);
  const Wts wt = weights(c, op);
  HIP_TRY(prof_launch(c, s, key, bytes, irb_flops(op, g), [&] {
    if (mxk)
      return launch_mx_irb(g.cin, g.hid, g.cout, g.stride, g.res, cur16, o16, x, wt.w0, wt.b0, (const float*)wt.w1,
                           wt.b1, wt.w2, wt.b2, y, B, h, w, OH, OW, s, mxlean);
    return launch_x2_irb(blk, plan, {x, wt.w0, wt.b0, (const float*)wt.w1, wt.b1, wt.w2, wt.b2, y, B, h, w, OH, OW,
                                     scratch, io, cus, c->x2_stage}, s);
  }));
  advance(a, y, OH, OW, op.cout, o16);
  return SPEF_OK;
}

// fp16 / bf16 blocks run fused when fusion is on, the map is large enough and a fused kernel covers the geometry.
bool fused16_applies(const Run& r, const Block& g, const Act& a) {
  return !r.f32 && r.c->fuse && (int64_t)a.h * a.w >= r.c->fuse_min_hw &&
         irb_supported(g.cin, g.hid, g.cout, g.stride, g.expand, g.res);
}

// fp16 / bf16: the pipelined kernel (SPEF_OPT_WAVESPEC 2) where it covers the geometry, else the wave-specialised
// one (>= 1), else the LDS-slab kernel.
int irb_step_fused16(const Run& r, const OpDesc& op, const Block& g, Act& a) {
  spef_ctx* c = r.c;
  hipStream_t s = r.s;
  const int B = r.B, h = a.h, w = a.w, dt = r.dt, OH = g.OH, OW = g.OW;
  void* x = a.p;
  void* y = free_buf(c, {x});
  const double bytes = (double)g.M * op.cin * 2 + (double)g.M2 * op.cout * 2 +
                       (g.expand ? pw_bytes(0, op.cin, op.hidden, false) : 0) + 40.0 * op.hidden +
                       pw_bytes(0, op.hidden, op.cout, false);
  const bool pipe3 = c->wavespec >= 2 && irp_supported(g.cin, g.hid, g.cout, g.stride, g.expand, g.res);
  const bool wspec = !pipe3 && c->wavespec && irw_supported(g.cin, g.hid, g.cout, g.stride, g.expand, g.res);
  char key[96];
  snprintf(key, sizeof(key), "%s<%u,%u,%u,s%u>", pipe3 ? "irp_kernel" : wspec ? "irw_kernel" : "irb_kernel",
           op.cin, op.hidden, op.cout, op.stride);
  const Wts wt = weights(c, op);
  HIP_TRY(prof_launch(c, s, key, bytes, irb_flops(op, g), [&] {
    if (pipe3)
      return launch_irp(c->irb_variant, dt, g.cin, g.hid, g.cout, g.stride, g.res, x, wt.w0, wt.b0, wt.w1, wt.b1, wt.w2,
                        wt.b2, y, B, h, w, OH, OW, s);
    if (wspec)
      return launch_irw(c->irb_variant, dt, g.cin, g.hid, g.cout, g.stride, g.res, x, wt.w0, wt.b0, wt.w1, wt.b1, wt.w2,
                        wt.b2, y, B, h, w, OH, OW, s);
    return launch_irb(c->irb_variant, dt, g.cin, g.hid, g.cout, g.stride, g.expand, g.res, x, wt.w0, wt.b0, wt.w1,
                      wt.b1, wt.w2, wt.b2, y, B, h, w, OH, OW, s);
  }));
  advance(a, y, OH, OW, op.cout);
  return SPEF_OK;
}

// One kernel per conv (fp32 always; fp16 / bf16 as the reference schedule). The only step that knows the observer;
// blk is the 1-based index of the block (its taps).
int irb_step_unfused(const Run& r, const OpDesc& op, const Block& g, int blk, Act& a) {
  spef_ctx* c = r.c;
  hipStream_t s = r.s;
  const spef_observer* obs = r.obs;
  const int B = r.B, h = a.h, w = a.w, dt = r.dt, OH = g.OH, OW = g.OW;
  const double es = r.es;
  const int64_t M = g.M, M2 = g.M2;
  const bool res = g.res, expand = g.expand;
  void* x = a.p;
  const Wts wt = weights(c, op);
  const int tap0 = 2 + 3 * (blk - 1);   // quant, expand, dw of this block
  if (obs && blk >= 2) HIP_TRY(observe(r, tap0, x, M * op.cin));
  void* h1 = x;
  if (expand) {
    h1 = free_buf(c, {x});
    HIP_TRY(pw_launch(r, EPI_RELU, x, wt.w0, wt.b0, nullptr, h1, M, op.cin, op.hidden));
    if (obs) HIP_TRY(observe(r, tap0 + 1, h1, M * op.hidden));
  }
  void* h2 = free_buf(c, {x, h1});
  const double opx = (double)B * OH * OW;
  const int dw_mode = irb_dw_mode(dt, g.hid, expand, g.stride);
  static const char* const dw_names[2][3] = {{"dw_kernel<1>", "dw_kernel<1,pairs>", "dw_kernel<1,pk16>"},
                                             {"dw_kernel<2>", "dw_kernel<2,pairs>", "dw_kernel<2,pk16>"}};
  HIP_TRY(prof_launch(c, s, dw_names[op.stride == 1 ? 0 : 1][dw_mode],
                      ((double)B * h * w + opx) * op.hidden * es + 40.0 * op.hidden, opx * op.hidden * 18.0, [&] {
    return launch_dw(dt, h1, wt.w1, wt.b1, h2, B, h, w, g.hid, g.stride, OH, OW, dw_mode, s);
  }));
  void* y = res ? free_buf(c, {x, h2}) : free_buf(c, {h2});
  if (obs) HIP_TRY(observe(r, tap0 + 2, h2, M2 * op.hidden));
  if (obs && res) {
    // the project output BEFORE the join goes into the block's shared quantizer as well: project without the
    // residual, observe, then y += x -- the one fp32 add EPI_RES makes after the bias, so y is bit-identical
    HIP_TRY(pw_launch(r, EPI_NONE, h2, wt.w2, wt.b2, nullptr, y, M2, op.hidden, op.cout));
    if (blk >= 2) HIP_TRY(observe(r, tap0, y, M2 * op.cout));
    HIP_TRY(prof_launch(c, s, "add_f32_kernel", 3.0 * M2 * op.cout * 4, (double)M2 * op.cout, [&] {
      return launch_add_f32((float*)y, (const float*)x, M2 * op.cout, s);
    }));
  } else {
    HIP_TRY(pw_launch(r, res ? EPI_RES : EPI_NONE, h2, wt.w2, wt.b2, res ? x : nullptr, y, M2, op.hidden, op.cout));
  }
  advance(a, y, OH, OW, op.cout);
  return SPEF_OK;
}

// ---------------------------------------------------------------------------------------------------- last conv
// What runs, by (family, mode, feat_f32):
//   mode 0  fp16x2 / fp16mx on a map x2_pw_pool covers, fp16 / bf16 always: conv fused with the mean, the map is
//           never stored. Every other case: conv into a workspace buffer, then mean_hw.
//   mode 2  conv into feat_f32 where given (fp16 / bf16: fp32 straight from the GEMM epilogue), else into a workspace
//           buffer.
//   mode 1  (a probe past the last block) fp16x2 / fp16mx: conv into a workspace buffer; the other families stop at
//           the last block's output.
int last_conv(const Run& r, const OpDesc& op, Act& a) {
  spef_ctx* c = r.c;
  hipStream_t s = r.s;
  const int B = r.B, h = a.h, w = a.w, dt = r.dt, mode = r.mode;
  void* cur = a.p;
  const Wts wt = weights(c, op);
  const double M3 = (double)B * h * w;
  if (mode == 0 && r.x2 && x2_pw_pool_supported(h * w, (int)op.cout)) {
    float* part = (float*)free_buf(c, {cur});
    HIP_TRY(prof_launch(c, s, "x2_pw_kernel<pool>", M3 * op.cin * 4 + (double)op.cout * (op.cin * 4 + 4) +
                        (double)B * op.cout * 4, 2.0 * M3 * op.cin * op.cout, [&] {
      return launch_x2_pw_pool(cur, wt.w0, wt.b0, part, c->pooled, B, h * w, (int)op.cin, (int)op.cout, s,
                               (c->trim & 1) != 0);
    }));
    return SPEF_OK;
  }
  if (mode == 0 && !r.x2 && !r.f32) {
    const bool tiled = c->gemm && ((op.cout + 15) & ~15u) % 128 == 0;
    HIP_TRY(prof_launch(c, s, tiled ? "pool_gemm_kernel" : "pw_pool_kernel<4>",
                        M3 * op.cin * 2 + (double)op.cout * (op.cin * 2 + 4) + (double)B * op.cout * 4,
                        2.0 * M3 * op.cin * op.cout, [&] {
      return tiled ? launch_pool_gemm(dt, cur, wt.w0, wt.b0, c->pooled, B, h * w, (int)op.cin, (int)op.cout, s)
                   : launch_pw_pool(dt, cur, wt.w0, wt.b0, c->pooled, B, h * w, (int)op.cin, (int)op.cout, s);
    }));
    return SPEF_OK;
  }
  if (mode == 1 && !r.x2) return SPEF_OK;
  // the map is stored: the keypoint head's input, a feature export, or the URSONet mean's input
  const bool to_feat = mode == 2 && r.feat_f32;
  void* y = to_feat ? (void*)r.feat_f32 : free_buf(c, {cur});
  if (r.x2) {
    HIP_TRY(prof_launch(c, s, "x2_pw_kernel<4,4>", M3 * (op.cin + op.cout) * 4 + (double)op.cout * (op.cin * 4 + 4),
                        2.0 * M3 * op.cin * op.cout, [&] {
      return launch_x2_pw_relu(cur, wt.w0, wt.b0, (float*)y, (int64_t)B * h * w, (int)op.cin, (int)op.cout, s,
                               (c->trim & 1) != 0);
    }));
  } else if (r.f32) {
    const double bytes = to_feat ? (double)B * h * w * (op.cin + op.cout) * 4
                                 : M3 * (op.cin + op.cout) * 4 + (double)op.cout * (op.cin + 1) * 4;
    HIP_TRY(prof_launch(c, s, gemm_f32_key(op.cout), bytes, 2.0 * M3 * op.cin * op.cout, [&] {
      return launch_gemm_f32(EPI_RELU, cur, wt.w0, wt.b0, nullptr, y, (int64_t)B * h * w, (int)op.cin, (int)op.cout, s);
    }));
  } else if (to_feat) {
    HIP_TRY(prof_launch(c, s, gemm_key(dt, EPI_RELU_F32, op.cout), pw_bytes(B * h * w, op.cin, op.cout, false) +
                        (double)B * h * w * op.cout * 2, 2.0 * B * h * w * op.cin * op.cout, [&] {
      return launch_gemm_pw(dt, EPI_RELU_F32, cur, wt.w0, wt.b0, nullptr, y, (int64_t)B * h * w, (int)op.cin,
                            (int)op.cout, s);
    }));
  } else {
    HIP_TRY(pw_any(c, dt, EPI_RELU, cur, wt.w0, wt.b0, nullptr, y, (int64_t)B * h * w, (int)op.cin, (int)op.cout, s));
  }
  advance(a, y, h, w, op.cout);
  if (mode == 0)
    HIP_TRY(prof_launch(c, s, "mean_hw_kernel", M3 * op.cout * 4 + (double)B * op.cout * 4, M3 * op.cout, [&] {
      return launch_mean_hw((const float*)y, c->pooled, B, h * w, (int)op.cout, s);
    }));
  return SPEF_OK;
}

int last_step(const Run& r, const OpDesc& op, Act& a) {
  if (r.obs) HIP_TRY(observe(r, 2 + 3 * r.obs->n_blocks, a.p, (int64_t)r.B * a.h * a.w * a.ch));
  const int rc = last_conv(r, op, a);
  if (rc) return rc;
  if (r.obs) HIP_TRY(observe(r, 3 + 3 * r.obs->n_blocks, a.p, (int64_t)r.B * a.h * a.w * a.ch));
  return SPEF_OK;
}

// Runs the float backbone (Run has the modes); *out is the activation it ended at.
int run_backbone(spef_ctx* c, const void* input, int layout, int B, int H, int W, hipStream_t s, int mode, int stop,
                 Act* out, float* feat_f32 = nullptr, const spef_observer* obs = nullptr) {
  const int dt = (int)c->hdr.dtype;
  const bool f32 = dt == DT_F32, x2 = dt == DT_X2 || dt == DT_MX;
  const Run r{c, s, input, layout, B, mode, stop, feat_f32, obs, dt, f32, x2, dt == DT_MX, (f32 || x2) ? 4.0 : 2.0};
  Act a{nullptr, H, W, 3, false};
  int blk = 0;   // 1-based index of the current inverted residual
  int op_index = 0;
  bool skip_next = false;
  for (const OpDesc& op : c->ops) {
    int rc = SPEF_OK;
    if (skip_next) {   // block 1 already produced by the fused front kernel
      skip_next = false;
    } else if (op.kind == OP_STEM) {
      const OpDesc* nx = (&op + 1 < c->ops.data() + c->ops.size()) ? &op + 1 : nullptr;
      skip_next = front_fusable(r, op, nx);
      rc = skip_next ? front_step(r, op, *nx, a) : stem_step(r, op, a);
    } else if (op.kind == OP_IRB) {
      ++blk;
      const Block g(op, B, a);
      rc = x2 ? irb_step_x2(r, op, g, a)
              : fused16_applies(r, g, a) ? irb_step_fused16(r, op, g, a) : irb_step_unfused(r, op, g, blk, a);
    } else if (op.kind == OP_LAST) {
      rc = last_step(r, op, a);
      if (rc) return rc;
      break;
    }
    if (rc) return rc;
    if (mode == 1 && op_index == stop) break;
    ++op_index;
  }
  if (out) *out = a;
  return SPEF_OK;
}

// ---------------------------------------------------------------------------------------------------- int8
// QuantAvgPool2d + TruncTo8bit (ursonet.py:61-62, 88): the HW-pixel sum of last_conv's b_last-bit codes has
// b_last + ceil(log2 HW) bits; truncation to the pooling width drops the rest (oracle/int8_ref.py pool_shift).
inline int q8_pool_shift(const spef_ctx* c, int hw) {
  int tb = 0;
  while ((1 << tb) < hw) ++tb;
  const int sh = c->q8_last_bits + tb - c->q8_pool_bits;
  return sh > 0 ? sh : 0;
}

// The requantisation triple of an n-channel conv at blob offset `off`: int64 M [np], int64 B [np], int32 S [np].
struct Requant {
  const int64_t *M, *B;
  const int32_t* S;
};
Requant requant(const spef_ctx* c, uint64_t off, uint32_t n) {
  const int64_t* q = ptr<int64_t>(c, off);
  const uint32_t np_ = (n + 15) & ~15u;
  return {q, q + np_, reinterpret_cast<const int32_t*>(q + 2 * np_)};
}

// What every q_gemm of the backbone sets: y [M][N] = requant(x [M][K] * w), weights and triple at blob offsets.
QGemmArgs q_conv(const spef_ctx* c, int epi, const void* x, uint64_t w, uint64_t rq_off, int out_bits, void* y,
                 int64_t M, uint32_t K, uint32_t N) {
  QGemmArgs a{};
  const Requant rq = requant(c, rq_off, N);
  a.epi = epi;
  a.x = (const int8_t*)x;
  a.w = ptr<int8_t>(c, w);
  a.rqM = rq.M;
  a.rqB = rq.B;
  a.rqS = rq.S;
  a.out_bits = out_bits;
  a.y = y;
  a.M = M;
  a.K = (int)K;
  a.N = (int)N;
  return a;
}

// INT8 schedule (k_q8.hip): one kernel per conv, or one per block (k_q8irb.hip / k_q8irw.hip). Activations: stem /
// expand outputs u8, depthwise outputs offset int8 (u - 128), block outputs int8 at the next consumer's scale, last
// conv u8.
// mode: 0 = full (pooled offset-int8 codes into c->pooled), 1 = stop after op `stop`, 2 = last conv map.
// *is_unsigned tells the caller how to read the codes of *out.
int run_backbone_q8(spef_ctx* c, const void* input, int layout, int B, int H, int W, hipStream_t s, int mode,
                    int stop, Act* out, int* is_unsigned) {
  Act cur{nullptr, H, W, 3, false};
  int uns = 0;
  int op_index = 0;
  for (const OpDesc& op : c->ops) {
    const int h = cur.h, w = cur.w;
    if (op.kind == OP_QSTEM) {
      const int OH = conv_out(h, 2), OW = conv_out(w, 2);
      uint8_t* y = (uint8_t*)c->buf[0];
      const float s_img = c->q8_s_img;
      const double px = (double)B * OH * OW;
      const Requant rq = requant(c, op.b0, 32);
      HIP_TRY(prof_launch(c, s, layout == IN_U8_NHWC ? "q_stem_kernel<u8>" : "q_stem_kernel<f32>",
                          (double)B * h * w * 3 * (layout == IN_U8_NHWC ? 1 : 4) + px * 32, px * 2 * 27 * 32, [&] {
        return launch_q_stem(input, layout == IN_F32_NCHW, ptr<int8_t>(c, op.w1), s_img, qbits(op, 1),
                             ptr<int8_t>(c, op.w0), rq.M, rq.B, rq.S, qbits(op, 0), y, B, h, w, OH, OW, s);
      }));
      advance(cur, y, OH, OW, 32);
      uns = 1;
    } else if (op.kind == OP_QIRB) {
      const int64_t M = (int64_t)B * h * w;
      const int OH = conv_out(h, (int)op.stride), OW = conv_out(w, (int)op.stride);
      const int64_t M2 = (int64_t)B * OH * OW;
      const bool res = op.flags & 1u;
      void* x = cur.p;
      void* y = nullptr;
      if (c->fuse && op.x2 != kAbsent &&
          q_irb_supported((int)op.cin, (int)op.hidden, (int)op.cout, (int)op.stride, res, op.expand != 1)) {
        y = free_buf(c, {x});
        const std::array<int64_t, 3>& r3 = c->q8_res[&op - c->ops.data()];
        // role-split form for blocks 8-17 with SPEF_OPT_Q8_ROLESPLIT (bit-identical either way)
        const bool qw = c->q8_rolesplit && op.expand != 1 &&
                        q_irw_supported((int)op.cin, (int)op.hidden, (int)op.cout, (int)op.stride, res);
        char key[96];
        snprintf(key, sizeof(key), "%s<%u,%u,%u,s%u>", qw ? "q_irw_kernel" : "q_irb_kernel", op.cin, op.hidden,
                 op.cout, op.stride);
        HIP_TRY(prof_launch(c, s, key, (double)M * op.cin + (double)M2 * op.cout + (double)op.hidden * (op.cin + op.cout + 9),
                            2.0 * M * op.cin * op.hidden + 18.0 * M2 * op.hidden + 2.0 * M2 * op.hidden * op.cout, [&] {
          const QBits qb{qbits(op, 0), qbits(op, 1), qbits(op, 2)};
          if (qw)
            return launch_q_irw((int)op.cin, (int)op.hidden, (int)op.cout, (int)op.stride, res, (op.flags & 4u) != 0,
                                (const int8_t*)x, ptr<int8_t>(c, op.w0), ptr<int8_t>(c, op.w2), ptr<int32_t>(c, op.x0),
                                ptr<uint8_t>(c, op.x2), r3[0], r3[1], (int)r3[2], qb, (int8_t*)y, B, h, w, OH, OW, s);
          return launch_q_irb((int)op.cin, (int)op.hidden, (int)op.cout, (int)op.stride, res, op.expand != 1,
                              (op.flags & 4u) != 0, (const int8_t*)x,
                              ptr<int8_t>(c, op.w0), ptr<int8_t>(c, op.w2), ptr<int32_t>(c, op.x0),
                              ptr<uint8_t>(c, op.x2), r3[0], r3[1], (int)r3[2], qb, (int8_t*)y, B, h, w, OH, OW, s);
        }));
      } else {   // one kernel per conv
        void* h1 = x;
        if (op.expand != 1) {
          h1 = free_buf(c, {x});
          const QGemmArgs a = q_conv(c, QEPI_RELU, x, op.w0, op.b0, qbits(op, 0), h1, M, op.cin, op.hidden);
          HIP_TRY(prof_launch(c, s, "q_gemm<relu>", (double)M * (op.cin + op.hidden) + (double)op.hidden * op.cin,
                              2.0 * M * op.cin * op.hidden, [&] { return launch_q_gemm(a, s); }));
        }
        void* h2 = free_buf(c, {x, h1});
        const Requant rq = requant(c, op.b1, op.hidden);
        HIP_TRY(prof_launch(c, s, "q_dw_kernel", (double)(M + M2) * op.hidden + 9.0 * op.hidden,
                            18.0 * M2 * op.hidden, [&] {
          return launch_q_dw((const uint8_t*)h1, ptr<int8_t>(c, op.w1), rq.M, rq.B, rq.S, qbits(op, 1), (int8_t*)h2, B, h,
                             w, (int)op.hidden, (int)op.stride, OH, OW, s);
        }));
        y = res ? free_buf(c, {x, h2}) : free_buf(c, {h2});
        QGemmArgs a = q_conv(c, res ? QEPI_PROJ_RES : QEPI_PROJ, h2, op.w2, op.b2, qbits(op, 2), y, M2, op.hidden,
                             op.cout);
        a.init = ptr<int32_t>(c, op.x0);
        if (res) {
          const std::array<int64_t, 3>& r3 = c->q8_res[&op - c->ops.data()];
          a.r = (const int8_t*)x;
          a.rm = r3[0];
          a.rb = r3[1];
          a.rs = (int)r3[2];
        }
        HIP_TRY(prof_launch(c, s, res ? "q_gemm<proj_res>" : "q_gemm<proj>",
                            (double)M2 * (op.hidden + op.cout * (res ? 2 : 1)) + (double)op.cout * op.hidden,
                            2.0 * M2 * op.hidden * op.cout, [&] { return launch_q_gemm(a, s); }));
      }
      advance(cur, y, OH, OW, op.cout);
      uns = 0;
    } else if (op.kind == OP_QLAST) {
      const int64_t M = (int64_t)B * h * w;
      void* y = free_buf(c, {cur.p});
      const QGemmArgs a = q_conv(c, QEPI_RELU, cur.p, op.w0, op.b0, qbits(op, 0), y, M, op.cin, op.cout);
      HIP_TRY(prof_launch(c, s, "q_gemm<last>", (double)M * (op.cin + op.cout) + (double)op.cout * op.cin,
                          2.0 * M * op.cin * op.cout, [&] { return launch_q_gemm(a, s); }));
      advance(cur, y, h, w, op.cout);
      uns = 1;
      if (mode == 0) {
        const int tb = q8_pool_shift(c, h * w);
        HIP_TRY(prof_launch(c, s, "q_pool_kernel", (double)M * op.cout + (double)B * op.cout, (double)M * op.cout, [&] {
          return launch_q_pool((const uint8_t*)y, (int8_t*)c->pooled, B, h * w, (int)op.cout, tb, s);
        }));
      }
      break;
    }
    if (mode == 1 && op_index == stop) break;
    ++op_index;
  }
  if (out) *out = cur;
  if (is_unsigned) *is_unsigned = uns;
  return SPEF_OK;
}

}  // namespace

// FC constants for a pooled map of `hw` pixels (oracle/int8_ref.py head_params, same float64 expression order).
int q8_prepare_fc(spef_ctx* c, int hw) {
  if (c->q8_fc_hw == hw && c->q8_fc_init) return SPEF_OK;
  const int tb = q8_pool_shift(c, hw);
  const double s_pool = c->q8_sl * ldexp(1.0, tb) / hw;
  const double blo = -ldexp(1.0, c->q8_fc_bias_bits - 1), bhi = ldexp(1.0, c->q8_fc_bias_bits - 1) - 1;
  const size_t np_ = c->q8_sw.size();
  std::vector<int32_t> init(np_, 0);
  std::vector<float> sc(np_, 0.f);
  for (size_t i = 0; i < np_; ++i) {
    if (c->q8_sw[i] == 0.0) continue;   // padding rows
    double qb = nearbyint(c->q8_bias[i] / (s_pool * c->q8_sw[i]));
    qb = qb < blo ? blo : (qb > bhi ? bhi : qb);
    init[i] = c->q8_wsum[i] + (int32_t)qb;
    sc[i] = (float)(s_pool * c->q8_sw[i]);
  }
  if (!c->q8_fc_init) HIP_TRY(hipMalloc(&c->q8_fc_init, np_ * sizeof(int32_t)));
  if (!c->q8_fc_sc) HIP_TRY(hipMalloc(&c->q8_fc_sc, np_ * sizeof(float)));
  HIP_TRY(hipMemcpy(c->q8_fc_init, init.data(), np_ * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(c->q8_fc_sc, sc.data(), np_ * sizeof(float), hipMemcpyHostToDevice));
  c->q8_fc_hw = hw;
  c->q8_fc_tb = tb;
  return SPEF_OK;
}

extern "C" {

int spef_forward(spef_ctx* c, const void* input, int layout, int B, int H, int W, float* out0, float* out1,
                 void* stream) {
  int rc = check_ready(c, B, H, W);
  if (rc) return rc;
  if (!input || !out0) return fail(SPEF_ERR_ARG, "null input/output");
  if (layout != SPEF_IN_U8_NHWC && layout != SPEF_IN_F32_NCHW) return fail(SPEF_ERR_ARG, "bad layout");
  Dev d(c->device);
  hipStream_t s = (hipStream_t)stream;
  if (c->hdr.dtype == DT_I8) {   // INT8 path: backbone + TruncTo8bit pool + int8 FC (ursonet.py:36-93)
    if (!out1 && c->hdr.n_out1) return fail(SPEF_ERR_ARG, "null position output");
    Act map{};
    rc = run_backbone_q8(c, input, layout, B, H, W, s, 0, -1, &map, nullptr);
    if (rc) return rc;
    if (map.h * map.w != c->q8_fc_hw) return fail(SPEF_ERR_STATE, "int8 head constants not prepared (spef_reserve)");
    for (const OpDesc& op : c->ops)
      if (op.kind == OP_QFC) {
        QGemmArgs a{};
        a.epi = QEPI_FC;
        a.x = (const int8_t*)c->pooled;
        a.w = ptr<int8_t>(c, op.w0);
        a.init = c->q8_fc_init;
        a.y = out0;
        a.y1 = out1;
        a.sc = c->q8_fc_sc;
        a.n_split = (int)c->hdr.n_out0;
        a.M = B;
        a.K = (int)op.cin;
        a.N = (int)op.cout;
        HIP_TRY(prof_launch(c, s, "q_gemm<fc>", (double)B * op.cin + (double)op.cout * op.cin + (double)B * op.cout * 4,
                            2.0 * B * op.cin * op.cout, [&] { return launch_q_gemm(a, s); }));
      }
    return SPEF_OK;
  }
  if (c->hdr.head == HEAD_URSONET) {
    if (!out1 && c->hdr.n_out1) return fail(SPEF_ERR_ARG, "null position output");
    rc = run_backbone(c, input, layout, B, H, W, s, 0, -1, nullptr);
    if (rc) return rc;
    for (const OpDesc& op : c->ops)
      if (op.kind == OP_FC)
        HIP_TRY(prof_launch(c, s, "fc_kernel", ((double)B + op.cout) * op.cin * 4 + (double)B * op.cout * 4,
                            2.0 * B * op.cin * op.cout, [&] {
          return launch_fc(c->pooled, ptr<float>(c, op.w0), ptr<float>(c, op.b0), out0, (int)c->hdr.n_out0, out1,
                           (int)c->hdr.n_out1, B, (int)c->hdr.feat_c, s);
        }));
    return SPEF_OK;
  }
  // keypoint head (keypoints.py:24-27): flatten of the unpooled 1280 x fh x fw map -> Linear(122880, 24).
  // The blob stores the weight columns in NHWC flatten order, so the NHWC map is used as is.
  Act feat{};
  rc = run_backbone(c, input, layout, B, H, W, s, 2, -1, &feat, c->kpfeat);
  if (rc) return rc;
  const int64_t F = (int64_t)feat.h * feat.w * feat.ch;
  for (const OpDesc& op : c->ops)
    if (op.kind == OP_FCKP) {
      if ((int64_t)op.cin != F) return fail(SPEF_ERR_ARG, "keypoint head size does not match the feature map");
      HIP_TRY(prof_launch(c, s, "fc_splitk_kernel", ((double)B + op.cout) * F * 4, 2.0 * B * F * op.cout, [&] {
        return launch_fc_splitk(c->kpfeat, ptr<float>(c, op.w0), ptr<float>(c, op.b0), out0, (int)op.cout, B, (int)F,
                                kKpSplits, c->kppart, s);
      }));
    }
  return SPEF_OK;
}

int spef_backbone(spef_ctx* c, const void* input, int layout, int B, int H, int W, float* features, void* stream) {
  int rc = check_ready(c, B, H, W);
  if (rc) return rc;
  if (!input || !features) return fail(SPEF_ERR_ARG, "null input/output");
  Dev d(c->device);
  hipStream_t s = (hipStream_t)stream;
  if (c->hdr.dtype == DT_I8) {   // dequantized last-conv map: code * s_l
    Act feat{};
    rc = run_backbone_q8(c, input, layout, B, H, W, s, 2, -1, &feat, nullptr);
    if (rc) return rc;
    HIP_TRY(launch_q_to_f32(feat.p, features, (int64_t)B * feat.h * feat.w * feat.ch, 1, (float)c->q8_sl, s));
    return SPEF_OK;
  }
  return run_backbone(c, input, layout, B, H, W, s, 2, -1, nullptr, features);
}

int spef_feature_width(const spef_ctx* c, int* feat_c) {
  if (!c || !feat_c) return fail(SPEF_ERR_ARG, "null argument");
  if (!c->loaded) return fail(SPEF_ERR_STATE, "weights not loaded (spef_load_weights)");
  *feat_c = (int)c->hdr.feat_c;
  return SPEF_OK;
}

int spef_features(spef_ctx* c, const void* input, int layout, int B, int H, int W, float* pooled_out, void* stream) {
  int rc = check_ready(c, B, H, W);
  if (rc) return rc;
  if (!input || !pooled_out) return fail(SPEF_ERR_ARG, "null input/output");
  if (layout != SPEF_IN_U8_NHWC && layout != SPEF_IN_F32_NCHW) return fail(SPEF_ERR_ARG, "bad layout");
  if (c->hdr.head != HEAD_URSONET) return fail(SPEF_ERR_STATE, "spef_features needs a URSONet-head blob");
  if (c->hdr.dtype == DT_I8) return fail(SPEF_ERR_STATE, "spef_features: an int8 blob's pooled buffer holds codes");
  Dev d(c->device);
  hipStream_t s = (hipStream_t)stream;
  rc = run_backbone(c, input, layout, B, H, W, s, 0, -1, nullptr);   // exactly spef_forward's run up to its FC
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(pooled_out, c->pooled, (size_t)B * c->hdr.feat_c * sizeof(float), hipMemcpyDeviceToDevice, s));
  return SPEF_OK;
}

int spef_probe(spef_ctx* c, const void* input, int layout, int B, int H, int W, int stop_op, float* out, int* oc,
               int* oh, int* ow, void* stream) {
  int rc = check_ready(c, B, H, W);
  if (rc) return rc;
  if (!input || !out) return fail(SPEF_ERR_ARG, "null input/output");
  Dev d(c->device);
  hipStream_t s = (hipStream_t)stream;
  Act act{};
  if (c->hdr.dtype == DT_I8) {   // raw integer codes (stem: u8, block outputs: int8)
    int uns = 0;
    rc = run_backbone_q8(c, input, layout, B, H, W, s, 1, stop_op, &act, &uns);
    if (rc) return rc;
    HIP_TRY(launch_q_to_f32(act.p, out, (int64_t)B * act.h * act.w * act.ch, uns, 1.0f, s));
  } else {
    rc = run_backbone(c, input, layout, B, H, W, s, 1, stop_op, &act);
    if (rc) return rc;
    const int adt = c->hdr.dtype == DT_MX ? (act.f16 ? (int)DT_F16 : (int)DT_F32) : (int)c->hdr.dtype;
    HIP_TRY(launch_to_f32(adt, act.p, out, (int64_t)B * act.h * act.w * act.ch, s));
  }
  if (oc) *oc = act.ch;
  if (oh) *oh = act.h;
  if (ow) *ow = act.w;
  return SPEF_OK;
}

int spef_observe(spef_ctx* c, spef_observer* o, const void* input, int layout, int B, int H, int W, float* features,
                 void* stream) {
  if (!c || !o) return fail(SPEF_ERR_ARG, "null argument");
  if (!c->loaded) return fail(SPEF_ERR_STATE, "weights not loaded (spef_load_weights)");
  if (c->hdr.dtype != DT_F32)
    return fail(SPEF_ERR_STATE, "spef_observe needs an fp32 blob (the one-kernel-per-conv schedule)");
  int rc = check_ready(c, B, H, W);
  if (rc) return rc;
  if (!input) return fail(SPEF_ERR_ARG, "null input");
  if (layout != SPEF_IN_U8_NHWC && layout != SPEF_IN_F32_NCHW) return fail(SPEF_ERR_ARG, "bad layout");
  if (layout == SPEF_IN_F32_NCHW && ((uintptr_t)input & 3)) return fail(SPEF_ERR_ARG, "misaligned float32 input");
  if (o->device != c->device || o->geom != op_geometry(c))
    return fail(SPEF_ERR_ARG, "the observer was created for a model with another op list");
  Dev d(c->device);
  return run_backbone(c, input, layout, B, H, W, (hipStream_t)stream, 2, -1, nullptr, features, o);
}

}  // extern "C"
