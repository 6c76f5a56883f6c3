// Host-side launchers of the SPEF HIP kernels (internal; the public C ABI is include/spef.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "x2_plan.hpp"

namespace spef {

// Sets the calling thread's spef_last_error() message and returns `code` (api_core.cpp).
int report_error(int code, const std::string& msg);

enum Dtype : int {
  DT_F16 = 1, DT_BF16 = 2, DT_I8 = 3, DT_F32 = 4,
  DT_X2 = 5,   // fp32 I/O, split-fp16 MFMA (k_x2_*.hip)
  DT_MX = 6    // fp16mx: the fp16x2 weights; stem map, block outputs of blocks 1-3, hidden of blocks 2-4 stored fp16
};
enum Epi : int { EPI_NONE = 0, EPI_RELU = 1, EPI_RES = 2, EPI_RELU_F32 = 3 /* ReLU, fp32 output */ };
enum InLayout : int { IN_U8_NHWC = 0, IN_F32_NCHW = 1 };

// Stem ConvBnAct 3->32, 3x3, stride 2, pad 1, BN folded, ReLU. W: fp32 [27][32] (k = ky*9+kx*3+ci).
hipError_t launch_stem(int dtype, int in_layout, const void* in, const float* w, const float* bias, void* y,
                       int B, int H, int W, int OH, int OW, hipStream_t s);

// Pointwise 1x1 conv as C^T = W * X^T on MFMA: X [M][K] NHWC, Wt [Np][Kp] (zero padded), bias fp32 [Np],
// optional residual R [M][N]; Y [M][N].
hipError_t launch_pw(int dtype, int epi, const void* x, const void* wt, const float* bias, const void* r,
                     void* y, int64_t M, int K, int N, hipStream_t s);

// Same contract, LDS-tiled double-buffered MFMA GEMM (k_gemm.hip); gemm_key names the instantiation used.
hipError_t launch_gemm_pw(int dtype, int epi, const void* x, const void* wt, const float* bias, const void* r,
                          void* y, int64_t M, int K, int N, hipStream_t s);
const char* gemm_key(int dtype, int epi, int N);

// Depthwise 3x3 conv, pad 1, stride 1|2, BN folded, ReLU. W9: [9][C] (fp16 for fp16 blobs, fp32 for bf16),
// bias fp32 [C]. mode (irb_dw_mode; fp16 only for mode > 0): DW_PAIRS = the vertical-pair tap order of the fused fp16
// stride-1 blocks, DW_PK16 = the packed-fp16 accumulation of the fused fp16 stride-2 blocks.
hipError_t launch_dw(int dtype, const void* x, const void* w9, const float* bias, void* y, int B, int H, int W,
                     int C, int stride, int OH, int OW, int mode, hipStream_t s);

// Last 1x1 conv (+BN, ReLU) fused with the global mean over HW: pooled fp32 [B][N].
hipError_t launch_pw_pool(int dtype, const void* x, const void* wt, const float* bias, float* pooled, int B,
                          int HW, int K, int N, hipStream_t s);

// Same contract, LDS-tiled GEMM with a pixel-reducing epilogue (k_pool.hip); needs round_up(N,16) % 128 == 0.
hipError_t launch_pool_gemm(int dtype, const void* x, const void* wt, const float* bias, float* pooled, int B, int HW,
                            int K, int N, hipStream_t s);

// fp32 head GEMM (f32-input MFMA): out[b][i] = sum_k X[b][k] W[i][k] + bias[i], columns [0,n0) -> out0,
// [n0, n0+n1) -> out1. W fp32 [Np][K], K % 16 == 0.
hipError_t launch_fc(const float* x, const float* w, const float* bias, float* out0, int n0, float* out1, int n1,
                     int B, int K, hipStream_t s);

// Fused InvertedResidual block (expand -> depthwise -> project [+x]) for the geometries in k_irb.hip's table.
bool irb_supported(int cin, int hid, int cout, int stride, bool expand, bool res);
// How the fused kernel of this block evaluates its depthwise: DW_FP32 (v_fma_mix, fp32 accumulation), DW_PAIRS
// (vertical pairs: v_dot2_f32_f16 + v_fma_mix) or DW_PK16 (v_pk_fma_f16: two channels per op, fp16 accumulation).
// The unfused schedule runs dw_kernel in the same mode to stay bit-identical.
enum { DW_FP32 = 0, DW_PAIRS = 1, DW_PK16 = 2 };
int irb_dw_mode(int dtype, int hid, bool expand, int stride);
hipError_t launch_irb(int variant, int dtype, int cin, int hid, int cout, int stride, bool expand, bool res, const void* x,
                      const void* we, const float* be, const void* wd, const float* bd, const void* wp,
                      const float* bp, void* y, int B, int H, int W, int OH, int OW, hipStream_t s);

// Wave-specialised fused block (expand waves feed depthwise/project waves through a double-buffered LDS slab) for
// the low-resolution geometries in k_irw.hip's table (same contract, bit-identical to the unfused kernels).
// Three-stage pipelined fused block (k_irp.hip): MFMA waves expand + project, VALU waves depthwise; same contract.
bool irp_supported(int cin, int hid, int cout, int stride, bool expand, bool res);
hipError_t launch_irp(int variant, int dtype, int cin, int hid, int cout, int stride, bool res, const void* x, const void* we,
                      const float* be, const void* wd, const float* bd, const void* wp, const float* bp, void* y, int B,
                      int H, int W, int OH, int OW, hipStream_t s);
bool irw_supported(int cin, int hid, int cout, int stride, bool expand, bool res);
hipError_t launch_irw(int variant, int dtype, int cin, int hid, int cout, int stride, bool res, const void* x, const void* we,
                      const float* be, const void* wd, const float* bd, const void* wp, const float* bp, void* y,
                      int B, int H, int W, int OH, int OW, hipStream_t s);

// Stem (u8 NHWC input) fused with inverted-residual block 1 (32 -> dw -> 16), k_front.hip. wsp: /255-folded stem
// weights split hi + lo in the activation dtype, [2][32][32] (blob OP_STEM x0).
hipError_t launch_front(int dtype, const void* x, const void* wsp, const float* bs, const void* wd, const float* bd,
                        const void* wp, const float* bp, void* y, int B, int H, int W, int OH, int OW, hipStream_t s);

// fp32 schedule (k_f32.hip, blob dtype 4): 1x1 conv on the exact fp32 MFMA, same contract as launch_pw with fp32
// activations and weights ([Np][Kp] fp32); EPI_RELU_F32 = EPI_RELU. K % 4 == 0, N % 4 == 0.
hipError_t launch_gemm_f32(int epi, const void* x, const void* wt, const float* bias, const void* r, void* y,
                           int64_t M, int K, int N, hipStream_t s);
const char* gemm_f32_key(int N);
// fp16x2 schedule (k_x2_*.hip, blob dtype 5): fused inverted residual on fp32 NHWC activations with hi + lo fp16
// operands (3 MFMAs per product). x2_irb_plan (x2_plan.hpp) picks the kernel and its tile; the two queries below
// are that plan's `known` and kernel_name() ("x2_irb_kernel" / "x2_irw_kernel" / "x2_irp_kernel", nullptr when none).
bool x2_irb_supported(int cin, int hid, int cout, int stride, bool expand, bool res);
const char* x2_irb_kernel_name(int cin, int hid, int cout, int stride, bool expand, bool res, int B, int OH, int OW,
                               bool scratch, int io, int num_cu);
// we: [2][r32(hid)][r32(cin)] fp16 (hi plane, lo plane), be fp32 [r32(hid)], wd fp32 [9][r32(hid)], bd fp32
// [r32(hid)], wp [2][r16(cout)][r32(hid)] fp16, bp fp32 [r16(cout)]; zero padded.
// scratch (nullable): B * OH * OW * cout * 2 floats for the hidden-split form of the late blocks on small maps.
// io: bit 0 = fp16 input x, bit 1 = fp16 output y (the fp16mx schedule; slab-kernel geometries, blocks 1-7, only).
// num_cu: the compute-unit count the plan was made with (the persistent-tile kernels size their grid by it).
struct X2Args {
  const void* x;
  const void* we;
  const float *be, *wd, *bd;
  const void* wp;
  const float* bp;
  void* y;
  int B, H, W, OH, OW;
  float* scratch;
  int io, num_cu;
  int stage = 1;   // SPEF_OPT_X2_STAGE: the persistent role-split rows (kind 3) on x2_irw_st_kernel (0: x2_irw_kernel)
};
// Runs the plan's row (hipErrorNotSupported when the plan found none); the plan must come from x2_irb_plan with
// this block, a.B, a.OH, a.OW, a.scratch != nullptr, a.io and a.num_cu.
hipError_t launch_x2_irb(const X2Block& b, const X2Plan& p, const X2Args& a, hipStream_t s);
// The families' part of it: the rows of the plan's kind -> the template instantiation (k_x2_irb.hip kind 0,
// k_x2_irw.hip kinds 1-3, k_x2_irp.hip kinds 5-6).
hipError_t launch_x2_slab(const X2Block& b, const X2Plan& p, const X2Args& a, hipStream_t s);
hipError_t launch_x2_split(const X2Block& b, const X2Plan& p, const X2Args& a, hipStream_t s);
hipError_t launch_x2_stage3(const X2Block& b, const X2Plan& p, const X2Args& a, hipStream_t s);
// fp16mx blocks 2-4 (k_mx.hip): fp16 input, hi + lo fp16 weights (blob dtype 5 / 6 layout), fp16 hidden slab, fp32
// depthwise, hi + lo project operand; fp16 (out16: blocks 2-3) or fp32 (block 4) output.
bool mx_irb_supported(int cin, int hid, int cout, int stride, bool expand, bool res, bool in16, bool out16);
hipError_t launch_mx_irb(int cin, int hid, int cout, int stride, bool res, bool in16, bool out16, const void* x,
                         const void* we,
                         const float* be, const float* wd, const float* bd, const void* wp, const float* bp, void* y,
                         int B, int H, int W, int OH, int OW, hipStream_t s, bool lean = true);
// lean (SPEF_OPT_TRIM bit 1): the tile set-up on scalar bases and 32-bit offsets (same sums), taken where
// mx_irb_lean_fits: an image's input and output maps below 2^31 bytes, the input row pitch and H below 2^23.
bool mx_irb_lean_fits(int cin, int cout, bool out16, int H, int W, int OH, int OW);
// fp16mx front (k_mx.hip front_mx_kernel): uint8 NHWC -> stem + block 1 -> fp16 [B][OH][OW][16]; wsp = OP_STEM x1.
hipError_t launch_mx_front(const void* x, const void* wsp, const float* bs, const float* wd, const float* bd,
                           const void* wp, const float* bp, void* y, int B, int H, int W, int OH, int OW,
                           hipStream_t s);
// uint8 NHWC frames -> stem + block 1 -> [B][OH][OW][16] (x2_front_kernel), fp32 or (out16) fp16; wsx: blob OP_STEM
// x0 of dtype 5 / 6.
hipError_t launch_x2_front(const void* x, const void* wsx, const float* bs, const float* wd, const float* bd,
                           const void* wp, const float* bp, void* y, int B, int H, int W, int OH, int OW, hipStream_t s,
                           bool out16 = false);
// 1x1 conv + BN + ReLU on fp32 activations X [M][K] with wt [2][Np][Kp] fp16 (hi, lo) -> fp32 Y [M][N]; Np % 64 == 0.
// wide: the 128-pixel x 320-channel staged tile where the shape takes it (SPEF_OPT_TRIM bit 0; same sums).
hipError_t launch_x2_pw_relu(const void* x, const void* wt, const float* bias, float* y, int64_t M, int K, int N,
                             hipStream_t s, bool wide = true);
// Same conv fused with URSONetHead's mean over HW (HW % 64 == 0, N % 64 == 0): part = workspace [B * HW / 64][N].
bool x2_pw_pool_supported(int HW, int N);
hipError_t launch_x2_pw_pool(const void* x, const void* wt, const float* bias, float* part, float* pooled, int B,
                             int HW, int K, int N, hipStream_t s, bool wide = true);
// URSONetHead mean([2,3]) over an fp32 NHWC map: pooled [B][C].
hipError_t launch_mean_hw(const float* x, float* pooled, int B, int HW, int C, hipStream_t s);

// Split-K fp32 head GEMM for very long K: part = workspace [splits][B][round_up(n,16)] floats.
hipError_t launch_fc_splitk(const float* x, const float* w, const float* bias, float* out, int n, int B, int K,
                            int splits, float* part, hipStream_t s);

// Keypoint decode: sigmoid (optional) + EPnP + dcm2quat per problem (k_epnp.hip). raw: B x 2(n+1) (origin +
// n keypoints, normalised x,y); kp3d: n x 3 fp32 (device); K: host 3x3 row-major. status |= 8 on failure.
// Brown-Conrady lens distortion of the keypoint camera (OpenCV's 5-coefficient order); on = 0: none.
struct EpnpDist {
  double k1, k2, p1, p2, k3;
  int on;
};
// model = control points [4][3] + alphas [n][4] (fp64, device), computed once by spef_set_keypoints.
hipError_t launch_epnp(const float* raw, int B, int n, const float* kp3d, const double* model, const double* K,
                       float nu, float nv, const EpnpDist& dist, int apply_sigmoid, float* kp_out, float* quat,
                       float* pos, int* status, hipStream_t s);
// Pose refinement behind EPnP (k_refine.hip): robust Levenberg-Marquardt on the reprojection error, in place on quat /
// pos. kp: B x 2(n+1) normalised keypoints (after the sigmoid); weights: null or B x n; fit [B x 4], cov [B x 36] and
// iters [B] may be null. status |= 16 (not refined), 32 (stopped at max_iters).
hipError_t launch_refine(const float* kp, const float* weights, int B, int n, const float* kp3d, const double* K,
                         float nu, float nv, const EpnpDist& dist, int max_iters, float huber_px, float* quat,
                         float* pos, float* fit, float* cov, int* iters, int* status, hipStream_t s);
// Exhaustive 3-point consensus between EPnP and the refinement (k_consensus.hip): every triple of candidate points
// (weights > 0; null: all) is solved by P3P and scored on all candidates with min(e^2, inlier_px^2). On consensus quat /
// pos are replaced by the winning hypothesis and weights_out [B x n] keeps the confidences of its inliers (0 elsewhere);
// info [B x 4] (inliers, triple, root, hypotheses scored), cost [B] and pose64 [B x 12] (the winning R row-major, then t,
// before the float32 rounding; NaN without consensus) may be null. status |= 64 (no consensus).
hipError_t launch_consensus(const float* kp, const float* weights, int B, int n, const float* kp3d, const double* K,
                            float nu, float nv, const EpnpDist& dist, float inlier_px, int min_inliers, float* quat,
                            float* pos, float* weights_out, int* info, float* cost, double* pose64, int* status,
                            hipStream_t s);

// Activation dtype -> fp32 NHWC copy (debug probes / backbone feature export).
hipError_t launch_to_f32(int dtype, const void* x, float* y, int64_t n, hipStream_t s);

// Decode (src/spe/spe_utils.py:56-101): ori softmax + Markley average; pos softmax + soft-argmax.
// status[b] |= 1 (NaN orientation moments), 2 (pos zero sum), 4 (NaN position).
// The orientation kernels write status[b] (=, not |=) and copy pos_src -> pos when pos_src is not null.
hipError_t launch_decode_ori(const float* logits, int B, int n_bins, const double* q_bins, float* soft,
                             float* quat, int* status, const float* pos_src, float* pos, hipStream_t s);
hipError_t launch_normalize_ori(const float* raw, int B, float* quat, int* status, const float* pos_src, float* pos,
                                hipStream_t s);
hipError_t launch_decode_pos(const float* logits, int B, int n_bins, const double* grid, float* soft,
                             float* pos, int* status, hipStream_t s);

// The same decodes of rows that already are PDFs (the video path's filtered PDFs: no softmax). The orientation
// kernel writes status[b] (a row without positive moment trace counts as NaN: bit 1), the position kernel ORs 2 / 4.
hipError_t launch_decode_pdf(const float* ori_pdf, const float* pos_pdf, int B, int n_ori, const double* q_bins,
                             int n_pos, const double* grid, float* quat, float* pos, int* status, hipStream_t s);

// ---- pose covariance of the soft-classification decode (k_cov.hip; the arithmetic is stated in
// spef_amd/spe/decode_cov.py) ----
struct CovParams {
  double fixed_var[2], floor_var[2];   // (theta, t): a regression head's variance; added to a classification head's diagonal
};
// cov [B][36] (theta first, then t), ori_hinv [B][16] (nullable; orientation classification only) and cov_status [B]
// (1 theta block NaN, 2 a not positive definite, 4 t block NaN) from the PDFs [B][n] and the pose they were decoded to.
// One launch, one workgroup per (row, head); a head that is not in classification mode (ori_cls / pos_cls = 0) reads
// neither its PDF nor its table nor its pose.
hipError_t launch_decode_cov(int ori_cls, int pos_cls, const float* ori_pdf, int n_ori, const double* q_bins,
                             const float* pos_pdf, int n_pos, const double* grid, const float* quat, const float* pos,
                             int B, const CovParams& prm, float* cov, float* ori_hinv, int* cov_status, hipStream_t s);

// ---- multi-hypothesis orientation decode (k_modes.hip; the algorithm is stated in spef_amd/spe/modes.py) ----
constexpr int MODES_MAX = 4;   // SPEF_MODES_MAX
struct ModesParams {
  int k_max, rounds;
  double cos_half_sep, seed_rel, min_mass, floor_var;   // cos_half_sep = cos(sep / 2)
};
// Up to k_max modes of every row of ori_pdf [B][n_ori]: mode_quat [B][k_max][4], mode_mass [B][k_max], mode_cov
// [B][k_max][9] (NaN past n_modes[b]), n_modes [B], modes_status [B] (1 = the row is not a PDF). One workgroup per row.
hipError_t launch_decode_modes(const float* ori_pdf, int n_ori, const double* q_bins, int B, const ModesParams& prm,
                               float* mode_quat, float* mode_mass, float* mode_cov, int* n_modes, int* modes_status,
                               hipStream_t s);

// ---- head fit (k_headfit.hip; the arithmetic is stated in spef_amd/solver/head_fit.py) ----
// The soft-classification targets of B poses (quat [B][4], pos [B][3], fp64) on the decode tables: ori_soft [B][n_ori] /
// pos_soft [B][n_pos] (either nullable), mask (nullable) [n_ori] = the redundant bins, status [B][2] (ori, pos: 1 = the
// row is NaN). One workgroup per (row, head).
hipError_t launch_encode_targets(const double* quat, const double* pos, int B, const double* q_bins, int n_ori,
                                 const double* grid, int n_pos, double ori_var, double pos_var, const uint8_t* mask,
                                 float* ori_soft, float* pos_soft, int* status, hipStream_t s);
enum : int { HF_SGD = 0, HF_ADAM = 1 };   // spef_headfit_optimizer
struct HeadFitShape {
  int K, n_ori, n_pos, Np, Bmax;   // Np = n_ori + n_pos rounded up to 16: the row count of W, the row pitch of G
};
struct HeadFitOpt {
  int kind;
  double momentum, beta1, beta2, eps, weight_decay;
};
// Xd = keep ? X * inv_keep : 0 over B * K elements, keep = hash(seed, counter[0], element) >= thr.
hipError_t launch_headfit_dropout(const float* X, float* Xd, int B, int K, uint32_t seed, uint32_t thr, float inv_keep,
                                  const uint32_t* counter, hipStream_t s);
// Row losses (rowloss [2][Bmax] fp64: ori, pos; rowaux [Bmax]: a regression row's sum of target^2) and G [B][Np] of the
// classification heads from the logits Zo [B][n_ori] / Zp [B][n_pos] and the targets; so / sp = the heads' scale / B.
// logits_out (nullable) [B][n_ori + n_pos].
hipError_t launch_headfit_loss(const HeadFitShape& d, const float* Zo, const float* To, const float* Zp, const float* Tp,
                               int B, int pos_reg, float so, float sp, float* G, double* rowloss, double* rowaux,
                               float* logits_out, hipStream_t s);
// Batch means -> loss_out [3] (total, ori, pos; nullable), the regression head's G, and with `train` the step counter
// (counter[0] steps completed, counter[1] this step's index) and Adam's bias corrections sc [2].
hipError_t launch_headfit_finish(const HeadFitShape& d, const double* rowloss, const double* rowaux, int B, int pos_reg,
                                 int norm_distance, double beta, const float* Zp, const float* Tp, float* G, int train,
                                 double beta1, double beta2, uint32_t* counter, float* sc, float* loss_out,
                                 hipStream_t s);
// dW = G^T Xsel (rows below n_ori contract with Xo, the others with Xp) fused with the optimizer step on W [Np][K], bias
// [Np] and their state (S2 / bS2 unused by SGD); lr: device float; grad_out (nullable) [Np * K + Np].
hipError_t launch_headfit_update(const HeadFitShape& d, const HeadFitOpt& opt, const float* G, const float* Xo,
                                 const float* Xp, int B, float* W, float* S1, float* S2, float* bias, float* bS1,
                                 float* bS2, float* grad_out, const float* lr, const float* sc, hipStream_t s);

// ---- adaptive video filter (k_video.hip; TemporalPDF.update_pdf, src/temporal/pdf_compare.py:94-134) ----
// Frames are time-major: row t * S + s is time step t of stream s. One head (ori or pos) of the filter:
struct VideoHead {
  const float* in;    // [T][S][n] soft-classification PDFs
  float* filt;        // [T][S][n] filtered PDFs
  float* dist;        // [T][S] distance to the previous filtered PDF (0 on a stream's first frame)
  float* state;       // [S][n] previous filtered PDF per stream
  float* state_sum;   // [S] its sum (fp64 sum rounded to float32)
  int* have;          // [S] 0 after a reset: the next frame passes through
  int n;              // bins (<= 8192)
  float nmix, alpha;  // TemporalPDF n and alpha
};
enum VideoMetric : int { VM_L2 = 0, VM_KL = 1, VM_JS = 2, VM_HELLINGER = 3, VM_TV = 4, VM_WASSERSTEIN = 5 };
// Sequential scan over t of both heads, one workgroup per (stream, head).
hipError_t launch_video_scan(const VideoHead& ori, const VideoHead& pos, int T, int S, int metric, hipStream_t s);
// Quaternion pole continuity per stream in time order (src/temporal/inference.py:136-144): quat_video / quat_still
// [T][S][4] in place (either may be null); poles [2][S][4] and pole_have [2][S]: 0 = still, 1 = video.
hipError_t launch_video_pole(float* quat_video, float* quat_still, float* poles, int* pole_have, int T, int S,
                             hipStream_t s);
// flags [4][S] (ori have, pos have, still pole have, video pole have): clear stream `stream`, or all with -1.
hipError_t launch_video_reset(int* flags, int S, int stream, hipStream_t s);
// Load one stream's state from device rows (a null pointer clears that part).
hipError_t launch_video_set_state(const VideoHead& ori, const VideoHead& pos, float* poles, int* pole_have, int S,
                                  int stream, const float* ori_pdf, const float* pos_pdf, const float* still_pole,
                                  const float* video_pole, hipStream_t s);

// ---- pose scoring (k_score.hip; SPEUtils.get_score, src/spe/spe_utils.py:103-159, and the statistics of
// src/tools/evaluation.py:59-99) ----
// Rows are time-major: row t * S + s belongs to group s. The logs of all (track, group) pairs:
struct ScoreLog {
  float* rows;         // [n_tracks][n_groups][capacity][5]: pos_err, pos_norm, ori_rad, ori_deg, ori_stable
  int* flags;          // [n_tracks][n_groups][capacity]: 1 dot > 1.01, 2 non-finite input, 4 zero target, 8 status
  int* count;          // [n_tracks][n_groups] rows logged (<= capacity)
  long long* dropped;  // [n_tracks][n_groups] rows that arrived after the log was full
  int n_groups, capacity;
};
constexpr unsigned SCORE_TILE = 8192;   // rows the finalize kernel sorts in LDS (32 KiB); spef_amd.score.LDS_ROWS
enum ScoreField : int {                 // spef_score_field (include/spef.h), spef_amd.score.STAT_FIELDS
  SF_N = 0, SF_N_BAD, SF_N_DROPPED, SF_ORI_SCORE, SF_POS_SCORE, SF_ESA_SCORE, SF_ORI_ERROR, SF_POS_ERROR, SF_ORI_STD,
  SF_POS_STD, SF_ORI_MEDIAN, SF_POS_MEDIAN, SF_ORI_MAD, SF_POS_MAD, SF_ORI_MIN, SF_ORI_MAX, SF_POS_MIN, SF_POS_MAX,
  SF_FLAGS, SCORE_FIELDS
};
// Score T * S rows into the logs of `track` (and rows_out [T * S][5] when not null), then advance the counts by T:
// two kernels, no host value. status (nullable): the rows' decode status.
hipError_t launch_score_step(const ScoreLog& lg, int track, const float* quat, const float* pos, const int* status,
                             const float* quat_true, const float* pos_true, int T, int S, float* rows_out,
                             hipStream_t s);
// Clear the counts of `group` in every track (all groups: -1).
hipError_t launch_score_reset(const ScoreLog& lg, int n_tracks, int group, hipStream_t s);
// stats [n_groups][n_tracks][SCORE_FIELDS] doubles. scratch: 2 * n_groups * n_tracks regions of scratch_stride floats
// (the capacity rounded up to a power of two), needed when the capacity exceeds SCORE_TILE.
hipError_t launch_score_finalize(const ScoreLog& lg, int n_tracks, float* scratch, unsigned scratch_stride,
                                 double* stats, hipStream_t s);
// Copy n log slots from `first` of (track, group) to rows [n][5] / flags [n].
hipError_t launch_score_read(const ScoreLog& lg, int track, int group, int first, int n, float* rows, int* flags,
                             hipStream_t s);

// ---- pose tracking (k_track.hip; the arithmetic is stated in spef_amd/spe/track.py) ----
constexpr int TRACK_STATE = 160;   // doubles per stream: have, coast, 0, q[4], t[3], w[3], v[3], P[144] row-major
struct TrackParams {
  double q[4], p0[4], r[2], cov_scale, gate_chi2, max_coast;
};
// T time steps of S streams, time-major rows (row t * S + s): one wave per stream. cov [T*S][36], status [T*S], d2,
// cov_out [T*S][36] and rates_out [T*S][6] may be null; quat_out / pos_out may alias quat / pos.
hipError_t launch_track_step(const TrackParams& p, double* state, const float* quat, const float* pos,
                             const float* cov, const int* status, int T, int S, float* quat_out, float* pos_out,
                             float* d2, float* cov_out, float* rates_out, int* track_status, hipStream_t s);
// The same step with up to K (1..MODES_MAX) orientation candidates per row: mode_quat [T*S][K][4], mode_mass [T*S][K],
// mode_cov [T*S][K][9] (the theta block of candidate k; cov [T*S][36] supplies the rest), n_modes [T*S]; the kernel
// picks the candidate of largest likelihood under the prediction (the heaviest valid one without a track) and writes
// its index to chosen [T*S] (-1: none). status, d2, cov_out and rates_out may be null.
hipError_t launch_track_step_modes(const TrackParams& p, double* state, const float* mode_quat, const float* mode_mass,
                                   const float* mode_cov, const int* n_modes, int K, const float* pos, const float* cov,
                                   const int* status, int T, int S, float* quat_out, float* pos_out, float* d2,
                                   float* cov_out, float* rates_out, int* track_status, int* chosen, hipStream_t s);
// Zero n doubles at state (a stream without a track); copy n doubles (get / set state).
hipError_t launch_track_reset(double* state, int64_t n, hipStream_t s);
hipError_t launch_track_copy(double* dst, const double* src, int64_t n, hipStream_t s);
// launch_track_step that also records the posterior of frame f of stream s at hist[(f * S + s) * TRACK_STATE]: the
// state row with the frame's track status in slot 2 (hist points at the first frame of the call).
hipError_t launch_track_step_hist(const TrackParams& p, double* state, double* hist, const float* quat,
                                  const float* pos, const float* cov, const int* status, int T, int S, float* quat_out,
                                  float* pos_out, float* d2, float* cov_out, float* rates_out, int* track_status,
                                  hipStream_t s);

// ---- pose smoothing (k_smooth.hip; the arithmetic is stated in spef_amd/spe/smooth.py) ----
// A workspace row of the backward pass, per history row: ok (1 / 0: P- of the next frame has a Cholesky factor),
// q-[4], t-[3], the gain G[144] and P-[144], row-major.
constexpr int SMOOTH_WS = 296;
// One frame of S history rows from the tracker's state and track_status [S].
hipError_t launch_track_history_push(double* hist_frame, const double* state, const int* track_status, int S,
                                     hipStream_t s);
hipError_t launch_track_history_count(int* out, int count, hipStream_t s);
// The backward pass over T frames of S streams; hist and ws point at the window's first frame. quat_io [T*S][4] and
// pos_io [T*S][3] hold the filter's outputs and receive the smoothed pose; cov_out [T*S][36] and rates_out [T*S][6]
// may be null (without cov_out no covariance is smoothed). Two launches: the gains, one wave per row of the first
// T - 1 frames, and the chains, one wave per stream.
hipError_t launch_track_smooth_gain(const TrackParams& p, const double* hist, double* ws, int T, int S, bool want_cov,
                                    hipStream_t s);
hipError_t launch_track_smooth_chain(const double* hist, const double* ws, int T, int S, float* quat_io, float* pos_io,
                                     float* cov_out, float* rates_out, int* smooth_status, hipStream_t s);

// ---- histogram observers of the INT8 calibration (k_observe.hip) ----
constexpr int OBS_BINS = 8192, OBS_COUNTERS = 8;   // one tap's record: OBS_COUNTERS + OBS_BINS uint64
// Add the statistic of n values at x (float32, 4-byte aligned; u8: uint8 pixels, value = u / 255) to the record `tap`,
// on at most max_blocks workgroups per launch.
hipError_t launch_observe(uint64_t* tap, const void* x, int64_t n, bool u8, int max_blocks, hipStream_t s);
// y[i] += x[i], one fp32 add each.
hipError_t launch_add_f32(float* y, const float* x, int64_t n, hipStream_t s);
hipError_t launch_observe_reset(uint64_t* st, int64_t n_words, hipStream_t s);

// ---- INT8 path (k_q8.hip; integer semantics of oracle/int8_ref.py) ----
enum QEpi : int { QEPI_RELU = 0, QEPI_PROJ = 1, QEPI_PROJ_RES = 2, QEPI_FC = 3 };

// Input quant + stem (u8 NHWC via `lut`, or f32 NCHW via round(x / s_img)) -> u8 NHWC [B][OH][OW][32].
// w28: int8 [32][28] (k = ky*9+kx*3+ci, k 27 zero); M/B/S: requant [32].
hipError_t launch_q_stem(const void* in, int f32in, const int8_t* lut, float s_img, int in_bits, const int8_t* w28,
                         const int64_t* M, const int64_t* Bq, const int32_t* S, int out_bits, uint8_t* y, int B, int H,
                         int W, int OH, int OW, hipStream_t s);
// Depthwise 3x3: u8 in, int8 [9][C] weights -> ReLU-quant, stored offset (u - 128) int8.
hipError_t launch_q_dw(const uint8_t* x, const int8_t* w9, const int64_t* M, const int64_t* Bq, const int32_t* S,
                       int out_bits, int8_t* y, int B, int H, int W, int C, int stride, int OH, int OW, hipStream_t s);
struct QGemmArgs {
  int epi;
  const int8_t* x;          // [M][K] int8 rows
  const int8_t* w;          // [Np][Kp64] int8
  const int32_t* init;      // [Np] accumulator init (offset correction, FC bias) or null
  const int64_t* rqM;       // requant [Np] (RELU / PROJ / PROJ_RES)
  const int64_t* rqB;
  const int32_t* rqS;
  const int8_t* r;          // PROJ_RES: residual [M][N] int8
  int64_t rm, rb;           // PROJ_RES: residual-join rescale
  int rs;
  void* y;                  // int8/u8 [M][N]; FC: float [M][n_split]
  float* y1;                // FC: float [M][N - n_split]
  const float* sc;          // FC: per-column output scale [Np]
  int n_split;
  int64_t M;
  int K, N;
  int out_bits = 8;         // output quantizer bit width (RELU unsigned, PROJ / PROJ_RES signed; bit_width.json)
};
hipError_t launch_q_gemm(const QGemmArgs& a, hipStream_t s);
// TruncTo8bit average pool over the whole map: u8 [B][HW][C] -> offset int8 [B][C] = ((sum) >> tb) - 128.
hipError_t launch_q_pool(const uint8_t* x, int8_t* p, int B, int HW, int C, int tb, hipStream_t s);
// Fused int8 inverted-residual block (expand blocks 2-17; k_q8irb.hip). tabs = blob OP_QIRB x2.
bool q_irb_supported(int cin, int hid, int cout, int stride, bool res, bool expand);
// Quantizer bit widths (bit_width.json, 2..8): eb / db expand / depthwise ReLU quantizers (unsigned), sb the
// shared signed quantizer the block's output is requantised to.
struct QBits {
  int eb, db, sb;
};
hipError_t launch_q_irb(int cin, int hid, int cout, int stride, bool res, bool expand, bool sh32, const int8_t* x, const int8_t* we,
                        const int8_t* wp, const int32_t* pinit, const uint8_t* tabs, int64_t rm, int64_t rb, int rs,
                        QBits qb, int8_t* y, int B, int H, int W, int OH, int OW, hipStream_t s);
// Role-split form of the same block for MobileNet-V2 blocks 8-17 (k_q8irw.hip; bit-identical, same arguments).
bool q_irw_supported(int cin, int hid, int cout, int stride, bool res);
hipError_t launch_q_irw(int cin, int hid, int cout, int stride, bool res, bool sh32, const int8_t* x, const int8_t* we,
                        const int8_t* wp, const int32_t* pinit, const uint8_t* tabs, int64_t rm, int64_t rb, int rs,
                        QBits qb, int8_t* y, int B, int H, int W, int OH, int OW, hipStream_t s);
// int8 (is_unsigned 0) or u8 codes -> fp32 code * scale.
hipError_t launch_q_to_f32(const void* x, float* y, int64_t n, int is_unsigned, float scale, hipStream_t s);

// ---- input preprocessing (k_pre.hip): Pillow BILINEAR resize with its integer coefficient tables ----
hipError_t launch_resize_h(const uint8_t* in, uint8_t* tmp, const int* bounds, const int* kk, int ksize, int B,
                           int Hin, int Win, int y0, int Ht, int Wo, hipStream_t s);
hipError_t launch_resize_v(const uint8_t* tmp, uint8_t* out, const int* bounds, const int* kk, int ksize, int B,
                           int Ht, int Ho, int Wo, hipStream_t s);

// ---- track-guided region of interest, keypoint mode (k_roi.hip; spef_amd/spe/roi.py states the arithmetic) ----
enum : int { ROI_FULL_FRAME = 1, ROI_BAD_BOX = 2 };
// The tracker's one-frame-ahead pose of n streams from their state rows (read only): quat_out [n][4], pos_out [n][3],
// have_out [n] (0: no track, the pose is zeros).
hipError_t launch_track_predict(const double* state, int n, float* quat_out, float* pos_out, int* have_out,
                                hipStream_t s);
// The box of B poses (have: null or [B]) for frames Hin x Win and a network input H x W: box_out [B][4] = (x0, y0, x1,
// y1), x1 / y1 exclusive; status [B] = ROI_FULL_FRAME where the row fell back to (0, 0, Win, Hin).
hipError_t launch_roi_boxes(const float* quat, const float* pos, const int* have, int B, int n, const float* kp3d,
                            const double* K, const EpnpDist& dist, int Hin, int Win, int H, int W, double margin,
                            double min_side, int* box_out, int* status, hipStream_t s);
// Pillow's coefficient tables per frame for crop(box).resize((W, H), BILINEAR). tab_h [B][W (2 + kstr_h)], tab_v
// [B][H (2 + kstr_v)]: bounds [out][2] then coefficients [out][kstr]; valid [B]; status (may be null) [B] = ROI_BAD_BOX
// for a box that is not inside the frame. kstr_h / kstr_v: multiples of 4, at least the full frame's ksize.
hipError_t launch_roi_coeffs(const int* box, int B, int Hin, int Win, int H, int W, int kstr_h, int kstr_v, int* tab_h,
                             int* tab_v, int* valid, int* status, hipStream_t s);
// The fused two-pass resample on tiles of TH x TW output pixels; rows_cap = the most source rows a tile can need.
size_t roi_resample_lds_bytes(int kstr_h, int kstr_v, int TH, int TW, int rows_cap);
hipError_t launch_roi_resample(const uint8_t* in, uint8_t* out, const int* tab_h, const int* tab_v, const int* valid,
                               int B, int Hin, int Win, int H, int W, int kstr_h, int kstr_v, int TH, int TW,
                               int rows_cap, hipStream_t s);
// raw [B][nk] head output -> kp_out [B][nk] normalised full-frame keypoints through box [B][4].
hipError_t launch_roi_unmap(const float* raw, const int* box, int B, int nk, float nu, float nv, int apply_sigmoid,
                            float* kp_out, hipStream_t s);

}  // namespace spef
