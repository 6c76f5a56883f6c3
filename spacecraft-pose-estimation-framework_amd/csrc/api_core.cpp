// Core of the C ABI (include/spef.h): error reporting, context life cycle, the workspace, model info, schedule
// options and the per-launch profiler. The other api_*.cpp files hold one subsystem each; spef_ctx.hpp is what they
// share.
#include <string.h>

#include <algorithm>

#include "spef_ctx.hpp"

static thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
namespace spef {
int report_error(int code, const std::string& msg) { return fail(code, msg); }
}  // namespace spef

int num_cus() {
  static int cus[32] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  dev &= 31;
  if (!cus[dev] && hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    cus[dev] = 256;
  return cus[dev];
}

static size_t elem_size(const spef_ctx* c) {   // int8 | fp16 / bf16 | fp32 activations (fp32 and fp16x2 schedules)
  return c->hdr.dtype == DT_I8 ? 1 : (c->hdr.dtype == DT_F32 || c->hdr.dtype == DT_X2 || c->hdr.dtype == DT_MX) ? 4 : 2;
}

// Max activation elements per image over the backbone schedule for an H x W input.
static int64_t max_act_elems(const spef_ctx* c, int H, int W, int* fh, int* fw) {
  int64_t mx = 0;
  int h = H, w = W;
  for (const OpDesc& op : c->ops) {
    if (op.kind == OP_STEM || op.kind == OP_QSTEM) {
      h = conv_out(h, 2);
      w = conv_out(w, 2);
      mx = std::max<int64_t>(mx, (int64_t)h * w * op.cout);
    } else if (op.kind == OP_IRB || op.kind == OP_QIRB) {
      mx = std::max<int64_t>(mx, (int64_t)h * w * op.hidden);  // expand output
      const int oh = conv_out(h, op.stride), ow = conv_out(w, op.stride);
      mx = std::max<int64_t>(mx, (int64_t)oh * ow * op.hidden);
      mx = std::max<int64_t>(mx, (int64_t)oh * ow * op.cout);
      h = oh;
      w = ow;
    } else if (op.kind == OP_LAST || op.kind == OP_QLAST) {
      mx = std::max<int64_t>(mx, (int64_t)h * w * op.cout);  // unfused last conv (spef_backbone)
    }
  }
  if (fh) *fh = h;
  if (fw) *fw = w;
  return mx;
}

int check_ready(spef_ctx* c, int B, int H, int W) {
  if (!c) return fail(SPEF_ERR_ARG, "null context");
  if (!c->loaded) return fail(SPEF_ERR_STATE, "weights not loaded (spef_load_weights)");
  if (B <= 0 || H < 32 || W < 32) return fail(SPEF_ERR_ARG, "bad input shape");
  if (B > c->ws_B || (int64_t)H * W > (int64_t)c->ws_H * c->ws_W || H != c->ws_H || W != c->ws_W)
    return fail(SPEF_ERR_STATE, "workspace not reserved for this shape (spef_reserve)");
  return SPEF_OK;
}

void free_workspace(spef_ctx* c) {
  for (void*& b : c->buf) {
    if (b) hipFree(b);
    b = nullptr;
  }
  if (c->pooled) hipFree(c->pooled);
  c->pooled = nullptr;
  if (c->kpfeat) hipFree(c->kpfeat);
  c->kpfeat = nullptr;
  if (c->kppart) hipFree(c->kppart);
  c->kppart = nullptr;
  c->ws_B = c->ws_H = c->ws_W = 0;
  c->buf_bytes = 0;
}

// option -> context field and accepted range; `msg` is the error for a value outside [lo, hi]. flag: any non-zero
// value is 1. An option without `msg` takes every value.
struct OptionDesc {
  int option;
  int spef_ctx::*field;
  bool flag;
  int lo, hi;
  const char* msg;
};
static const OptionDesc kOptions[] = {
    {SPEF_OPT_FUSE_BLOCKS, &spef_ctx::fuse, true, 0, 0, nullptr},
    {SPEF_OPT_IRB_VARIANT, &spef_ctx::irb_variant, false, 0, 0, nullptr},
    {SPEF_OPT_TEST_FAIL_BCAST, &spef_ctx::test_fail_bcast, false, 0, 3, "SPEF_OPT_TEST_FAIL_BCAST: 0..3"},
    {SPEF_OPT_PW_GEMM, &spef_ctx::gemm, true, 0, 0, nullptr},
    {SPEF_OPT_Q8_ROLESPLIT, &spef_ctx::q8_rolesplit, false, 0, 1, "SPEF_OPT_Q8_ROLESPLIT: 0 or 1"},
    {SPEF_OPT_MX_KERNELS, &spef_ctx::mx_kernels, true, 0, 0, nullptr},
    {SPEF_OPT_TRIM, &spef_ctx::trim, false, 0, 3, "SPEF_OPT_TRIM: bits 0-1"},
    {SPEF_OPT_X2_STAGE, &spef_ctx::x2_stage, false, 0, 1, "SPEF_OPT_X2_STAGE: 0 or 1"},
    {SPEF_OPT_WAVESPEC, &spef_ctx::wavespec, false, 0, 2, "SPEF_OPT_WAVESPEC: 0, 1 or 2"},
};

extern "C" {

int spef_abi_version(void) { return SPEF_ABI_VERSION; }

const char* spef_last_error(void) { return g_err.c_str(); }

int spef_init(int device, spef_ctx** out) {
  if (!out) return fail(SPEF_ERR_ARG, "out is null");
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(SPEF_ERR_ARG, "device index out of range");
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(SPEF_ERR_ARG, std::string("SPEF kernels are built for gfx950 only, device is ") + prop.gcnArchName);
  spef_ctx* c = new spef_ctx();
  c->device = device;
  *out = c;
  return SPEF_OK;
}

int spef_destroy(spef_ctx* c) {
  if (!c) return SPEF_OK;
  Dev d(c->device);
  free_workspace(c);
  if (c->d_data) hipFree(c->d_data);
  if (c->d_ori_bins) hipFree(c->d_ori_bins);
  if (c->d_pos_grid) hipFree(c->d_pos_grid);
  if (c->kp3d) hipFree(c->kp3d);
  if (c->kp_model) hipFree(c->kp_model);
  if (c->q8_fc_init) hipFree(c->q8_fc_init);
  if (c->pre_bh) hipFree(c->pre_bh);
  if (c->pre_bv) hipFree(c->pre_bv);
  if (c->pre_tmp) hipFree(c->pre_tmp);
  if (c->roi_tab_h) hipFree(c->roi_tab_h);
  if (c->roi_tab_v) hipFree(c->roi_tab_v);
  if (c->roi_valid) hipFree(c->roi_valid);
  if (c->q8_fc_sc) hipFree(c->q8_fc_sc);
  for (hipEvent_t e : c->pool) hipEventDestroy(e);
  delete c;
  return SPEF_OK;
}

int spef_model_info(const spef_ctx* c, int* head, int* n_out0, int* n_out1, int* dtype, int* n_ops) {
  if (!c || !c->loaded) return fail(SPEF_ERR_STATE, "weights not loaded");
  if (head) *head = (int)c->hdr.head;
  if (n_out0) *n_out0 = (int)c->hdr.n_out0;
  if (n_out1) *n_out1 = (int)c->hdr.n_out1;
  if (dtype) *dtype = (int)c->hdr.dtype;
  if (n_ops) *n_ops = (int)c->ops.size();
  return SPEF_OK;
}

int spef_reserve(spef_ctx* c, int B, int H, int W) {
  if (!c) return fail(SPEF_ERR_ARG, "null context");
  if (!c->loaded) return fail(SPEF_ERR_STATE, "weights not loaded");
  if (B <= 0 || H < 32 || W < 32) return fail(SPEF_ERR_ARG, "bad shape");
  if (B <= c->ws_B && H == c->ws_H && W == c->ws_W) return SPEF_OK;
  Dev d(c->device);
  int fh = 0, fw = 0;
  const int64_t per_img = max_act_elems(c, H, W, &fh, &fw);
  if (c->hdr.head == HEAD_KEYPOINTS && (fh != (int)c->hdr.kp_fh || fw != (int)c->hdr.kp_fw))
    return fail(SPEF_ERR_ARG, "keypoint head expects a fixed feature map size (keypoints.py:20)");
  free_workspace(c);
  const size_t bytes = (size_t)per_img * B * elem_size(c) + 256;
  for (void*& b : c->buf) HIP_TRY(hipMalloc(&b, bytes));
  HIP_TRY(hipMalloc(&c->pooled, (size_t)B * c->hdr.feat_c * sizeof(float)));
  if (c->hdr.head == HEAD_KEYPOINTS) {
    HIP_TRY(hipMalloc(&c->kpfeat, (size_t)B * fh * fw * c->hdr.feat_c * sizeof(float)));
    HIP_TRY(hipMalloc(&c->kppart, (size_t)kKpSplits * B * ((c->hdr.n_out0 + 15) & ~15u) * sizeof(float)));
  }
  if (c->hdr.dtype == DT_I8) {
    const int rc = q8_prepare_fc(c, fh * fw);
    if (rc) return rc;
  }
  c->buf_bytes = bytes;
  c->ws_B = B;
  c->ws_H = H;
  c->ws_W = W;
  return SPEF_OK;
}

int spef_set_option(spef_ctx* c, int option, int value) {
  if (!c) return fail(SPEF_ERR_ARG, "null context");
  if (option == SPEF_OPT_FUSE_MIN_HW) {   // the one 64-bit field
    c->fuse_min_hw = value;
    return SPEF_OK;
  }
  for (const OptionDesc& o : kOptions) {
    if (o.option != option) continue;
    if (o.msg && (value < o.lo || value > o.hi)) return fail(SPEF_ERR_ARG, o.msg);
    c->*o.field = o.flag ? (value != 0) : value;
    return SPEF_OK;
  }
  return fail(SPEF_ERR_ARG, "unknown option");
}

int spef_profile_begin(spef_ctx* c) {
  if (!c) return fail(SPEF_ERR_ARG, "null context");
  c->recs.clear();
  c->pool_next = 0;
  c->profiling = true;
  return SPEF_OK;
}

int spef_profile_end(spef_ctx* c, char* buf, size_t cap, size_t* needed) {
  if (!c) return fail(SPEF_ERR_ARG, "null context");
  Dev d(c->device);
  c->profiling = false;
  // aggregate per kernel key: launches, total ms, algorithmic bytes, flops
  struct Agg {
    long n = 0;
    double ms = 0, bytes = 0, flops = 0;
  };
  std::vector<std::pair<std::string, Agg>> agg;
  for (auto& r : c->recs) {
    HIP_TRY(hipEventSynchronize(r.b));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, r.a, r.b));
    Agg* a = nullptr;
    for (auto& kv : agg)
      if (kv.first == r.key) a = &kv.second;
    if (!a) {
      agg.push_back({r.key, Agg{}});
      a = &agg.back().second;
    }
    a->n += 1;
    a->ms += ms;
    a->bytes += r.bytes;
    a->flops += r.flops;
  }
  std::string js = "{";
  char tmp[512];
  for (size_t i = 0; i < agg.size(); ++i) {
    snprintf(tmp, sizeof(tmp), "%s\"%s\": [%ld, %.6f, %.1f, %.1f]", i ? ", " : "", agg[i].first.c_str(),
             agg[i].second.n, agg[i].second.ms, agg[i].second.bytes, agg[i].second.flops);
    js += tmp;
  }
  js += "}";
  c->recs.clear();
  c->pool_next = 0;
  if (needed) *needed = js.size() + 1;
  if (buf && cap > 0) {
    const size_t n = std::min(cap - 1, js.size());
    memcpy(buf, js.data(), n);
    buf[n] = 0;
    if (n < js.size()) return fail(SPEF_ERR_ARG, "profile buffer too small");
  }
  return SPEF_OK;
}

}  // extern "C"
