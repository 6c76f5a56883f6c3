// What the C ABI's translation units (api_*.cpp) share: the context and observer structs, error reporting, the device
// guard, the per-launch profiler and the few helpers more than one of them calls. Internal to the library.
#pragma once
#include "../../include/spef.h"

#include <hip/hip_runtime.h>

#include <array>
#include <string>
#include <vector>

#include "spef_blob.hpp"
#include "spef_kernels.hpp"
#include "spef_tuning.hpp"

using namespace spef;

#define SPEF_INTERNAL __attribute__((visibility("hidden")))   // shared between the api_*.cpp files, not exported

static const int kKpSplits = 60;   // split-K slices of the keypoint head (K = 122880 -> 2048 per slice)

// Sets the calling thread's spef_last_error() message and returns `code` (api_core.cpp).
SPEF_INTERNAL int fail(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                                  \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) return fail(SPEF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

struct spef_ctx {
  int device = 0;
  BlobHeader hdr{};
  std::vector<OpDesc> ops;
  uint8_t* d_data = nullptr;  // device copy of the blob's data section
  size_t data_bytes = 0;
  bool loaded = false;
  // workspace
  int ws_B = 0, ws_H = 0, ws_W = 0;
  size_t buf_bytes = 0;
  void* buf[4] = {nullptr, nullptr, nullptr, nullptr};
  float* pooled = nullptr;  // [B][1280] fp32
  float* kpfeat = nullptr;  // keypoint head: fp32 NHWC feature map [B][fh*fw*1280]
  float* kppart = nullptr;  // keypoint head: split-K partials
  // keypoint decode configuration (KeyPoints, keypoints_utils.py:19-45; Camera, speed.py:18-32)
  float* kp3d = nullptr;
  double* kp_model = nullptr;  // control points [4][3] + alphas [n][4] (fp64, computed once on the host)
  int kp_n = 0;
  double camK[9] = {0};
  float cam_nu = 0.f, cam_nv = 0.f;
  EpnpDist kp_dist = {0, 0, 0, 0, 0, 0};   // spef_set_keypoint_distortion
  // decode tables
  double* d_ori_bins = nullptr;
  int n_ori_bins = 0;
  double* d_pos_grid = nullptr;
  int n_pos_bins = 0;
  int fuse = 1;              // SPEF_OPT_FUSE_BLOCKS: 0 never, 1 when input H*W >= fuse_min_hw
  int64_t fuse_min_hw = 0;   // SPEF_OPT_FUSE_MIN_HW
  int gemm = 1;              // SPEF_OPT_PW_GEMM: 1 LDS-tiled GEMM, 0 register-direct pw kernel
  int irb_variant = -1;      // SPEF_OPT_IRB_VARIANT: fused-block tile variant (tuning sweeps; -1 = library default)
  int wavespec = 2;          // SPEF_OPT_WAVESPEC: 2 = pipelined (k_irp.hip), 1 = wave-specialised (k_irw.hip)
  int q8_rolesplit = 0;      // SPEF_OPT_Q8_ROLESPLIT: int8 blocks 8-17 role-split (k_q8irw.hip)
  int test_fail_bcast = 0;   // SPEF_OPT_TEST_FAIL_BCAST (spef_tuning.hpp): failure injection in spef_bcast_weights
  int mx_kernels = 1;        // SPEF_OPT_MX_KERNELS (spef_tuning.hpp): fp16mx blocks 2-7 on k_mx.hip
  int trim = 3;              // SPEF_OPT_TRIM (spef_tuning.hpp): bit 0 = the last conv's 128 x 320 tile, bit 1 = the
                             // lean tile set-up of mx_irb_kernel
  int x2_stage = 1;          // SPEF_OPT_X2_STAGE (spef_tuning.hpp): blocks 8-10 / 14 on x2_irw_st_kernel (static staging)
  // int8 blob: host copies of the FC quantisation constants, and their per-map-size device forms
  std::vector<double> q8_sw, q8_bias;
  std::vector<int32_t> q8_wsum;
  double q8_sl = 0.0;
  int32_t* q8_fc_init = nullptr;   // [Np] 128 * sum_k q_w + q_b (q_b depends on the pooled map size)
  float* q8_fc_sc = nullptr;       // [Np] f32(s_pool * s_w)
  int q8_fc_hw = 0, q8_fc_tb = 0;
  float q8_s_img = 0.f;                        // input scale (f32 NCHW path)
  int q8_last_bits = 8, q8_pool_bits = 8, q8_fc_bias_bits = 8;   // bit_width.json: last_conv act, pooling, FC bias
  // preprocessing (Pillow BILINEAR resize): coefficient tables for the last (Hin, Win, H, W), temp image
  int pre_key[4] = {0, 0, 0, 0};
  int* pre_bh = nullptr;   // [W][2] (xmin, count), then [W][ksize_h] coefficients
  int* pre_bv = nullptr;   // [H][2] (ymin - y0, count), then [H][ksize_v]
  int pre_ksh = 0, pre_ksv = 0, pre_y0 = 0, pre_ht = 0;
  uint8_t* pre_tmp = nullptr;
  size_t pre_tmp_bytes = 0;
  // region-of-interest preprocessing (spef_preprocess_roi): per-frame coefficient tables for the last (Hin, Win, H, W),
  // grown with the batch; tile shape and the most source rows a tile can need (api_roi.cpp)
  int roi_key[4] = {0, 0, 0, 0};
  int roi_B = 0;
  int* roi_tab_h = nullptr;   // [B][W (2 + roi_kstr_h)]
  int* roi_tab_v = nullptr;   // [B][H (2 + roi_kstr_v)]
  int* roi_valid = nullptr;   // [B]
  int roi_kstr_h = 0, roi_kstr_v = 0, roi_th = 0, roi_tw = 0, roi_rows_cap = 0;
  std::vector<std::array<int64_t, 3>> q8_res;  // per op: residual-join rescale (R, RB, RS)
  // per-launch HIP-event profiling (bench.py roofline leg)
  bool profiling = false;
  struct Rec {
    std::string key;
    hipEvent_t a, b;
    double bytes, flops;
  };
  std::vector<Rec> recs;
  std::vector<hipEvent_t> pool;
  size_t pool_next = 0;
};

// Histogram observers (k_observe.hip): one record of OBS_COUNTERS + OBS_BINS uint64 per tap of the loaded model.
// Tap ids: 0 image, 1 stem, 2 + 3 (i - 1) + {0, 1, 2} = quant / expand / dw of block i (1-based), 2 + 3 n_blocks final,
// 3 + 3 n_blocks last.
struct spef_observer {
  int device = 0;
  int n_blocks = 0, n_taps = 0;
  std::vector<std::array<uint32_t, 7>> geom;   // the op list the taps were laid out for
  uint64_t* state = nullptr;
  uint64_t* tap(int t) const { return state + (size_t)t * (OBS_COUNTERS + OBS_BINS); }
};

// Pose tracker (api_handles.cpp; api_roi.cpp reads its state for spef_track_predict).
struct spef_track {
  spef_ctx* ctx = nullptr;   // profiler of the step launches
  int device = 0;
  int S = 0;
  TrackParams prm{};
  double* state = nullptr;   // [S][TRACK_STATE]
};

// A blob parsed and copied into fresh device storage, not yet owned by any context (the first half of a
// transactional load: a failure anywhere leaves the context's current model untouched). api_blob.cpp stages and
// commits; spef_bcast_weights (api_comm.cpp) stages on every receiver before any of them commits.
struct Staged {
  BlobHeader h{};
  std::vector<OpDesc> ops;
  uint8_t* dd = nullptr;
  std::vector<std::array<int64_t, 3>> q8_res;
  std::vector<double> q8_sw, q8_bias;
  std::vector<int32_t> q8_wsum;
  double q8_sl = 0.0;
  float q8_s_img = 0.f;
  int q8_last_bits = 8, q8_pool_bits = 8, q8_fc_bias_bits = 8;
  Staged() = default;
  Staged(const Staged&) = delete;
  Staged& operator=(const Staged&) = delete;
  ~Staged() {
    if (dd) hipFree(dd);
  }
};
SPEF_INTERNAL int stage_blob(spef_ctx* c, const void* blob, size_t bytes, bool on_device, Staged* st);
SPEF_INTERNAL void commit_staged(spef_ctx* c, Staged* st);   // cannot fail

struct SPEF_INTERNAL Dev {  // RAII device guard
  int prev = -1;
  explicit Dev(int d) {
    hipGetDevice(&prev);
    if (prev != d) hipSetDevice(d);
  }
  ~Dev() {
    if (prev >= 0) hipSetDevice(prev);
  }
};

static inline int conv_out(int h, int s) { return (h + 2 - 3) / s + 1; }

static inline hipEvent_t next_event(spef_ctx* c) {
  if (c->pool_next >= c->pool.size()) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    c->pool.push_back(e);
  }
  return c->pool[c->pool_next++];
}

// Launch `fn` (returns hipError_t); when profiling, bracket it with events tagged by kernel key and its
// algorithmic bytes / flops (what roofline.achieved is priced in).
template <typename F>
static hipError_t prof_launch(spef_ctx* c, hipStream_t s, const char* key, double bytes, double flops, F&& fn) {
  if (!c->profiling) return fn();
  hipEvent_t a = next_event(c), b = next_event(c);
  if (!a || !b) return hipErrorOutOfMemory;
  hipEventRecord(a, s);
  hipError_t e = fn();
  hipEventRecord(b, s);
  c->recs.push_back({key, a, b, bytes, flops});
  return e;
}

template <typename T>
static inline const T* ptr(const spef_ctx* c, uint64_t off) {
  return off == kAbsent ? nullptr : reinterpret_cast<const T*>(c->d_data + off);
}

// quantizer bit width of an int8 op (spef_blob.hpp qbits; 0 = 8)
static inline int qbits(const OpDesc& op, int i) { return op.qbits[i] ? op.qbits[i] : 8; }

// compute units of the current device (cached per device; the fp16x2 plan sizes its tiles by it)
SPEF_INTERNAL int num_cus();
SPEF_INTERNAL int check_ready(spef_ctx* c, int B, int H, int W);
SPEF_INTERNAL void free_workspace(spef_ctx* c);
// int8 FC constants for a pooled map of `hw` pixels (api_schedule.cpp; spef_reserve prepares them)
SPEF_INTERNAL int q8_prepare_fc(spef_ctx* c, int hw);
// the op list an observer's taps are laid out for (api_handles.cpp)
SPEF_INTERNAL std::vector<std::array<uint32_t, 7>> op_geometry(const spef_ctx* c);
