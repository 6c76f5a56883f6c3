/* spef.h -- C ABI of the SPEF MI355X (gfx950) inference target.
 *
 * This is the drop-in boundary for the reference's duck-typed "SPE model" interface
 *     predict(images NCHW float32 in [0,1]) -> (pose dict, latency_ms)
 * implemented by SPETorch.predict   (src/spe/spe_torch.py:41-76),
 *                SPETVMARM.predict  (src/tvm/spe_tvm.py:45),
 *                SPEJetson.predict  (src/nvidia/spe_nvidia.py:105).
 * The Python class spef_amd.spe_mi355x.SPEMi355x implements that interface on top of these entry points
 * (ctypes); INTEGRATION.md shows the binding a reference maintainer adds.
 *
 * Conventions: every function returns 0 (SPEF_OK) or a positive error code; spef_last_error() returns the
 * calling thread's last message. Tensor pointers are DEVICE pointers unless a parameter says "host".
 * `stream` is a hipStream_t (NULL = default stream). One context per GPU; a context is not thread-safe.
 */
#ifndef SPEF_H_
#define SPEF_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPEF_ABI_VERSION 4
#define SPEF_COMM_ID_BYTES 128   /* size of the RCCL unique id (ncclUniqueId) */

enum spef_status {
  SPEF_OK = 0,
  SPEF_ERR_ARG = 1,      /* invalid argument (AssertionError in the reference, spe_torch.py:55)       */
  SPEF_ERR_HIP = 2,      /* HIP runtime error                                                        */
  SPEF_ERR_BLOB = 3,     /* malformed / incompatible weight blob                                      */
  SPEF_ERR_STATE = 4,    /* weights or decode tables not loaded, workspace too small                  */
  SPEF_ERR_NUMERIC = 5,  /* NaN / zero-sum in decode (ValueError, classification_utils.py:134,253,262) */
  SPEF_ERR_COMM = 6      /* RCCL error or timeout: the communicator was aborted (ncclCommAbort)       */
};

/* input layouts of spef_forward */
enum spef_layout {
  SPEF_IN_U8_NHWC = 0,   /* uint8 frames B x H x W x 3 (ToTensor's /255 fused into the stem)          */
  SPEF_IN_F32_NCHW = 1   /* float32 B x 3 x H x W in [0,1]: the reference `images` tensor             */
};

/* decode modes (MODEL.HEAD.ORI / MODEL.HEAD.POS, src/config/train/config.py:19-20) */
enum spef_mode { SPEF_REGRESSION = 0, SPEF_CLASSIFICATION = 1, SPEF_KEYPOINTS = 2 };

typedef struct spef_ctx spef_ctx;

int spef_abi_version(void);
const char* spef_last_error(void);

/* Create a context on HIP device `device` (SPETorch.__init__, spe_torch.py:24-39). */
int spef_init(int device, spef_ctx** out);
/* Release everything (SPETorch.delete_model, spe_torch.py:97-106). */
int spef_destroy(spef_ctx* ctx);

/* Load a packed weight blob (built by build_mi355x.py from parameters.pt, model.py:261-266 layout).
 * _host: blob in host memory; _device: blob already in this device's memory -- copied device-to-device.
 * The blob is validated in full first (spef_validate_blob); on any failure the context keeps the model it had
 * (or stays empty), so a failed reload never leaves a half-loaded context. */
int spef_load_weights(spef_ctx* ctx, const void* host_blob, size_t bytes);
int spef_load_weights_device(spef_ctx* ctx, const void* dev_blob, size_t bytes);
/* Query the loaded model: head (0 URSONet, 1 keypoints), output widths, storage dtype (1 fp16, 2 bf16, 3 int8,
 * 4 fp32 = the reference's own arithmetic: exact-fp32 MFMA, one kernel per conv; 5 fp16x2 = fp32 activations with
 * hi + lo fp16 MFMA operands, the fp32-accurate fused schedule; 6 fp16mx = the fp16x2 weights and kernels with the
 * stem map, the block outputs of blocks 1-3 and the hidden tensors of blocks 2-4 stored fp16: the headline schedule,
 * within 1e-3 of float32 at trained head scales). */
int spef_model_info(const spef_ctx* ctx, int* head, int* n_out0, int* n_out1, int* dtype, int* n_ops);

/* Allocate activation workspace for batches up to B of H x W frames. Must precede spef_forward for that
 * size (keeps hipMalloc out of the forward so the forward can be stream-captured). */
int spef_reserve(spef_ctx* ctx, int B, int H, int W);

/* ModelWrapper.forward (pytorch_layers.py:29-32): frames -> raw head outputs (fp32).
 * URSONet head: out0 = orientation logits/raw [B x n_out0], out1 = position [B x n_out1].
 * Keypoint head: out0 = keypoint regression [B x 24] (pre-sigmoid), out1 unused (may be NULL). */
int spef_forward(spef_ctx* ctx, const void* input, int layout, int B, int H, int W, float* out0, float* out1,
                 void* stream);

/* Backbone only (MobileNetV2.forward, mobilenet_v2.py:269-271): 1280-channel feature map as fp32 NHWC
 * [B x H/32 x W/32 x 1280] (the C2 feature-MSE check). */
int spef_backbone(spef_ctx* ctx, const void* input, int layout, int B, int H, int W, float* features,
                  void* stream);

/* Debug probe: run the backbone through op `stop_op` (0 = stem, i = inverted-residual block i) and write that
 * activation as fp32 NHWC; *c, *h, *w receive its shape. */
int spef_probe(spef_ctx* ctx, const void* input, int layout, int B, int H, int W, int stop_op, float* out,
               int* c, int* h, int* w, void* stream);

/* Decode constants (host, float64, as built by OrientationSoftClassification.build_histogram,
 * classification_utils.py:39-83, and PositionSoftClassification.build_histogram, :201-215). At most 8192
 * orientation bins (SPEF_ERR_ARG above; the default 12^3 grid has 1728, 1232 with unused bins deleted). */
int spef_set_decode_tables(spef_ctx* ctx, const double* ori_bins, int n_ori_bins, const double* pos_grid,
                           int n_pos_bins);

/* SPEUtils.last_activ + SPEUtils.decode (spe_utils.py:56-101) for the URSONet head.
 * ori_mode: SPEF_CLASSIFICATION (softmax -> ori_soft [B x n_ori], Markley average -> quat [B x 4]) or
 *           SPEF_REGRESSION (L2 normalise ori_raw [B x 4] -> quat, spe_utils.py:72).
 * pos_mode: SPEF_CLASSIFICATION (softmax -> pos_soft [B x n_pos], soft-argmax -> pos [B x 3]) or
 *           SPEF_REGRESSION (pos = pos_raw copied).
 * n_ori / n_pos: the row widths of ori_raw / pos_raw (the shapes NumPy carries in the reference). They must equal
 *           the decode tables' bin counts in classification mode (spef_set_decode_tables) and 4 / 3 in regression
 *           mode, else SPEF_ERR_ARG -- the kernels never read rows of a width the tables do not describe.
 * status: device int[B], zeroed by this call; bit 1 NaN orientation, 2 position zero sum, 4 NaN position.
 * ori_soft / pos_soft may be NULL. */
int spef_decode(spef_ctx* ctx, int ori_mode, int pos_mode, const float* ori_raw, int n_ori, const float* pos_raw,
                int n_pos, int B, float* ori_soft, float* quat, float* pos_soft, float* pos, int* status, void* stream);

/* Pose covariance of the soft-classification decode (opt-in; nothing calls it unless asked): what the PDFs that
 * spef_decode averaged say about the uncertainty of the pose it returned, as the measurement covariance
 * spef_track_step takes (spef_amd/spe/decode_cov.py is the NumPy twin and the specification; DESIGN.md section 3,
 * Covariance path). Works on any PDF + pose pair: spef_decode's ori_soft / pos_soft with its quat / pos, or
 * spef_video_step's ori_filt / pos_filt with its quat / pos. All arithmetic is fp64, every sum in a fixed order: a
 * row's result does not depend on the batch it is in.
 *
 * cov [B x 36]: row-major 6 x 6, order (theta_x, theta_y, theta_z, t_x, t_y, t_z), theta a left perturbation in the
 *   camera frame (R = exp([theta]x) R^: the convention of spef_refine_keypoints and spef_track_step); the cross blocks
 *   are zero.
 *   theta block = sum_i p_i theta_i theta_i^T / sum_i p_i + floor_var[0] I, with theta_i the rotation vector of
 *     q_i (x) conj(q^) on the hemisphere of scalar part >= 0 (the Log of the tracker's innovation), q_i the bins, q^ =
 *     quat renormalised in fp64; every bin enters with its own p, redundant ones included, as in the Markley average.
 *   t block = sum_i p_i (g_i - t^)(g_i - t^)^T / sum_i p_i + floor_var[1] I over the position grid g, t^ = pos (the
 *     centred form).
 *   A head in regression mode has no PDF: its block is fixed_var[k] I (the caller passes the tracker's r), and its
 *     PDF, width and pose arguments are not read.
 * ori_hinv (or NULL) [B x 16]: inv(a) of a = sum_i p_i q_i q_i^T, not normalised -- the second value of the
 *   reference's OrientationSoftClassification.decode (classification_utils.py:142), rounded to float32. Orientation
 *   classification only (SPEF_ERR_ARG otherwise).
 * cov_status [B]: a word of its own, never ORed into the decode status (the scorer flags any row with a nonzero
 *   decode status):
 *     1  the orientation PDF or quat is not finite, quat is zero, or sum p <= 0: the theta block is NaN;
 *     2  a is not positive definite to fp64 -- a Cholesky pivot that is not finite or not above 2^-48 of its diagonal
 *        entry, which is what the rounding of the sums leaves of an exact zero (a one-hot PDF: the case where the
 *        reference's np.linalg.inv raises LinAlgError): ori_hinv is NaN; the theta block stands;
 *     4  the position PDF or pos is not finite, or sum p <= 0: the t block is NaN.
 *   A row with a NaN block is a non-finite covariance to spef_track_step, which then uses its fixed r.
 * Widths as in spef_decode: n_ori / n_pos must equal the tables' bin counts in classification mode (SPEF_ERR_ARG);
 * SPEF_ERR_STATE when a table that is needed is not set. SPEF_ERR_ARG, with nothing enqueued, also for a NULL PDF or
 * pose pointer of a head in classification mode, a NULL cov / cov_status / params, a negative or non-finite variance
 * and B < 1. One launch, one workgroup per (row, head); no atomics, no allocation and no host synchronisation: it can
 * follow spef_decode on a stream and be stream-captured. */
typedef struct { double fixed_var[2], floor_var[2]; } spef_cov_params;
int spef_decode_cov(spef_ctx* ctx, int ori_mode, int pos_mode, const float* ori_pdf, int n_ori, const float* pos_pdf,
                    int n_pos, const float* quat, const float* pos, int B, const spef_cov_params* params, float* cov,
                    float* ori_hinv, int* cov_status, void* stream);

/* Multi-hypothesis orientation decode (opt-in; nothing calls it unless asked): up to k_max orientations that the
 * soft-classification PDF holds at once, where spef_decode returns their one Markley average (an ambiguous view puts
 * two or more peaks into the PDF; their average is none of them). spef_amd/spe/modes.py is the NumPy twin and states
 * every step; DESIGN.md section 3, Modes path. Works on spef_decode's ori_soft or spef_video_step's ori_filt. All
 * arithmetic is fp64, every sum in a fixed order: a row's result does not depend on the batch it is in.
 *
 * Per row, with c = cos(sep_deg / 2) and |a . b| the absolute 4-D dot product: seeds by greedy suppression (the alive bin
 * of largest p, float32 values compared exactly, ties to the lowest index; a bin is alive while |q_j . q_s| < c for every
 * seed so far; stop at p <= 0 or, after the first, at p < seed_rel * p_seed0), `rounds` Lloyd rounds (a bin goes to the
 * mode of largest |q_i . m_k|, ties to the lowest k; m_k = the Markley average of its cluster), a prune by descending
 * mass (drop a mode of mass < min_mass, or within sep_deg of one already kept), and a final assignment over the
 * survivors.
 * spef_modes_params: k_max in 1..SPEF_MODES_MAX, rounds in 0..8, 0 < sep_deg <= 180, seed_rel in [0, 1], min_mass in
 *   [0, 1 / k_max], floor_var >= 0 (added to the diagonal of every theta block), all finite (SPEF_ERR_ARG otherwise).
 * mode_quat [B x k_max x 4]  unit quaternions, scalar part >= 0, by descending mass; mode_mass [B x k_max] the
 *   clusters' shares of sum p; mode_cov [B x k_max x 9] the theta block of spef_decode_cov restricted to the
 *   cluster's bins, about its mode, row-major 3 x 3. Entries at or past n_modes[b] are NaN. With one mode the result is
 *   the plain Markley decode of the whole PDF, mass 1, and spef_decode_cov's theta block.
 * n_modes [B]: 1..k_max, 0 for an invalid row. modes_status [B] (a word of its own, never ORed into the decode status):
 *   1 = the PDF is not finite or sum p is not positive and finite; every output of the row is NaN.
 * n_ori must equal the table's bin count (SPEF_ERR_ARG); SPEF_ERR_STATE without an orientation table; SPEF_ERR_ARG, with
 * nothing enqueued, also for a NULL pointer and B < 1. One launch, one workgroup per row; no atomics, no allocation and
 * no host synchronisation: it can follow spef_decode on a stream and be stream-captured. */
#define SPEF_MODES_MAX 4
typedef struct { int k_max, rounds; double sep_deg, seed_rel, min_mass, floor_var; } spef_modes_params;
int spef_decode_modes(spef_ctx* ctx, const float* ori_pdf, int n_ori, int B, const spef_modes_params* params,
                      float* mode_quat, float* mode_mass, float* mode_cov, int* n_modes, int* modes_status,
                      void* stream);

/* Adaptive video filter on the device: the reference's TemporalPDF.update_pdf (src/temporal/pdf_compare.py:94-134)
 * and the quaternion pole continuity of Inference.predict (src/temporal/inference.py:136-144, :173-180) for batches
 * of video frames. Frames are TIME-MAJOR: a batch of T * S rows holds T consecutive time steps of S independent
 * streams, row t * S + s = step t of stream s (T = 64, S = 1: 64 frames of one video; T = 1, S = 64: one new frame
 * from each of 64 cameras). The state (previous filtered PDFs, poles) lives on the device; results do not depend on
 * how a sequence is cut into calls.
 *
 * spef_video_create: a filter for n_streams streams with distance `metric` and TemporalPDF's (n, alpha) per head
 *   (the reference's Inference engine: ori 0.8 / 16.49, pos 0.5 / 48.64, L2). The bin counts are those of the
 *   context's decode tables, which must both be set (SPEF_ERR_STATE otherwise; spef_video_step returns
 *   SPEF_ERR_STATE as well when the tables were replaced by ones of other sizes since). An unknown metric or
 *   n_streams < 1: SPEF_ERR_ARG. Every stream starts reset. The filter keeps a stream's PDF in registers, at most
 *   8192 bins per table: with more in either table (a 21^3 = 9261-bin position grid, which spef_set_decode_tables
 *   and the still-frame spef_decode accept) spef_video_create returns SPEF_ERR_ARG and leaves *out as it was. */
enum spef_video_metric {   /* spef_amd.temporal.METRICS order */
  SPEF_METRIC_L2 = 0,
  SPEF_METRIC_KL = 1,
  SPEF_METRIC_JS = 2,
  SPEF_METRIC_HELLINGER = 3,
  SPEF_METRIC_TV = 4,
  SPEF_METRIC_WASSERSTEIN = 5
};
typedef struct spef_video spef_video;
int spef_video_create(spef_ctx* ctx, int n_streams, int metric, float n_ori, float alpha_ori, float n_pos,
                      float alpha_pos, spef_video** out);
/* Forget the previous PDFs and poles of stream `stream` (or of all streams: -1): its next frame passes through with
 * distance 0 and sets the poles. Enqueued on `stream_hip`; no host synchronisation. */
int spef_video_reset(spef_video* video, int stream, void* stream_hip);
/* Load the state of one stream from device memory (how spef_amd's Inference engine shares one filter between its
 * per-frame host path and this one): ori_pdf [n_ori bins] / pos_pdf [n_pos bins] = the previous filtered PDFs,
 * still_pole / video_pole [4] = the poles; a NULL pointer resets that part. Enqueued; no host synchronisation. */
int spef_video_set_state(spef_video* video, int stream, const float* ori_pdf, const float* pos_pdf,
                         const float* still_pole, const float* video_pole, void* stream_hip);
/* One filter step over T time steps of all S streams (S must equal n_streams, T >= 1; SPEF_ERR_ARG otherwise, with
 * nothing enqueued). ori_soft [T*S x n_ori bins] / pos_soft [T*S x n_pos bins] are spef_decode's soft outputs.
 * Outputs: ori_filt / pos_filt = the filtered PDFs (same shapes; either may be NULL), ori_dist / pos_dist [T*S]
 * = the distance of each frame to the stream's previous filtered PDF (0 on the first frame after a reset),
 * quat [T*S x 4] / pos [T*S x 3] = the decode of the filtered PDFs (Markley average / soft-argmax, the kernels of
 * spef_decode without their softmax), quat with the pole rule applied per stream in time order: negated when its dot
 * product with the stream's pole is negative; the pole moves only when |dot| > 0.5; the first frame sets it.
 * still_quat_inout (NULL, or spef_decode's quat [T*S x 4]) gets the same rule in place against the stream's
 * still-frame pole. status [T*S]: written by this call, the bits of spef_decode (1 NaN orientation, 2 position zero
 * sum, 4 NaN position).
 * Bad frames: a frame whose input PDF does not sum to a positive finite number (all zero, a NaN in it) is passed to
 * the decode unfiltered, so its status bits are set (all-zero orientation row: 1; all-zero position row: 2 and 4;
 * NaN row: 1 / 4), its distance is NaN, and the stream's state is left as it was: the next good frame is filtered
 * against the last good one. A blend that does not sum to a positive finite number (a NaN distance) is written
 * out and flagged the same way and does not replace the state either.
 * No allocation and no host synchronisation: it can follow spef_decode on a stream and be stream-captured. */
int spef_video_step(spef_ctx* ctx, spef_video* video, const float* ori_soft, const float* pos_soft, int T, int S,
                    float* still_quat_inout, float* ori_filt, float* ori_dist, float* pos_filt, float* pos_dist,
                    float* quat, float* pos, int* status, void* stream_hip);
int spef_video_destroy(spef_video* video);

/* Pose scoring on the device: SPEUtils.get_score (src/spe/spe_utils.py:103-159), the per-image error lists of
 * evaluation() with their std and median absolute deviation (src/tools/evaluation.py:59-99) and the per-video min /
 * max / median / mean / std of the temporal tool (temporal.py:27-48), for poses that stay on the device. Rows are
 * TIME-MAJOR as on the video path: row t * S + s belongs to group s (a video, a camera, or the one group of a plain
 * evaluation). A scorer keeps one log of `capacity` rows per (group, track); a track is one kind of pose (track 0 the
 * still poses, track 1 the filtered ones). Arithmetic (spef_amd/score.py states it in NumPy): float32 elementwise,
 * every sum fp64 in a fixed order, acos / sqrt in fp64 rounded to float32; results do not depend on how the rows are
 * cut into steps.
 *
 * One log row holds five float32: pos_err = |t_true - t|, pos_norm = pos_err / |t_true|, ori_rad = 2 acos(min(|q .
 * q_true|, 1)), ori_deg = ori_rad * 180 / pi, ori_stable = 2 atan2(|q - s q_true|, |q + s q_true|) in fp64 with s =
 * sign(q . q_true) (radians: the angle between the two unit quaternions, half the rotation angle, the form the parity
 * checks use; it resolves small angles, where the acos form stops at about 0.04 degrees). Row flags:
 * 1 = |q . q_true| > 1.01 (get_score raises ValueError there, spe_utils.py:137), 2 = a non-finite input, 4 =
 * |t_true| == 0, 8 = the row's decode status is nonzero. A flagged row is logged as NaN, counts in n_bad and enters no
 * statistic.
 *
 * spef_score_create: allocates the logs (n_groups, n_tracks, capacity >= 1, capacity <= 2^20; SPEF_ERR_ARG otherwise).
 *   The context is used for its device and its profiler and must outlive the scorer. Every log starts empty. */
#define SPEF_SCORE_FIELDS 19
enum spef_score_field {   /* spef_score_finalize's doubles per (group, track), in this order */
  SPEF_SCORE_N = 0,         /* good rows                                                                   */
  SPEF_SCORE_N_BAD,         /* flagged rows in the log                                                     */
  SPEF_SCORE_N_DROPPED,     /* rows that arrived after the log was full                                    */
  SPEF_SCORE_ORI_SCORE,     /* mean ori_rad            (get_score 'ori_score')                             */
  SPEF_SCORE_POS_SCORE,     /* mean pos_norm           ('pos_score')                                       */
  SPEF_SCORE_ESA_SCORE,     /* their sum               ('esa_score')                                       */
  SPEF_SCORE_ORI_ERROR,     /* ori_score * 180 / pi    ('ori_error', degrees)                              */
  SPEF_SCORE_POS_ERROR,     /* mean pos_err            ('pos_error', metres)                               */
  SPEF_SCORE_ORI_STD,       /* population std of ori_deg / pos_err, two passes in fp64                     */
  SPEF_SCORE_POS_STD,
  SPEF_SCORE_ORI_MEDIAN,    /* np.median of the float32 ori_deg / pos_err: the middle one or (a + b) * 0.5 */
  SPEF_SCORE_POS_MEDIAN,
  SPEF_SCORE_ORI_MAD,       /* median of float32 |x - median| (mad(), evaluation.py:16-32)                 */
  SPEF_SCORE_POS_MAD,
  SPEF_SCORE_ORI_MIN,
  SPEF_SCORE_ORI_MAX,
  SPEF_SCORE_POS_MIN,
  SPEF_SCORE_POS_MAX,
  SPEF_SCORE_FLAGS          /* OR of the flags of every row in the log                                     */
};
typedef struct spef_score spef_score;
int spef_score_create(spef_ctx* ctx, int n_groups, int n_tracks, int capacity, spef_score** out);
/* Empty the logs of group `group` (all groups: -1) in every track. Enqueued; no host synchronisation. */
int spef_score_reset(spef_score* score, int group, void* stream);
/* Score T time steps of all S groups (S must equal n_groups, T >= 1, 0 <= track < n_tracks; SPEF_ERR_ARG otherwise,
 * with nothing enqueued) and append them to the logs of `track`: row t * S + s goes to slot count[s] + t of group s,
 * the counts are read and advanced on the device. quat [T*S x 4] / pos [T*S x 3] = the predicted poses (spef_decode's
 * or spef_video_step's outputs), status (or NULL) [T*S] their decode status, quat_true / pos_true the targets.
 * rows_out (or NULL) [T*S x 5] receives the rows as well. A row that arrives when its log is full is not stored and is
 * counted in n_dropped. No allocation and no host synchronisation: it can follow spef_decode / spef_video_step on a
 * stream and be stream-captured. */
int spef_score_step(spef_score* score, int track, const float* quat, const float* pos, const int* status,
                    const float* quat_true, const float* pos_true, int T, int S, float* rows_out, void* stream);
/* The statistics of every (group, track) over its good rows: stats (device) receives n_groups * n_tracks *
 * SPEF_SCORE_FIELDS doubles, (group, track) major. With no good row every statistic is NaN. The logs are only read:
 * scoring can go on afterwards. The order statistics are exact (a sort of a scratch copy, in LDS up to 8192 rows).
 * No allocation and no host synchronisation. */
int spef_score_finalize(spef_score* score, double* stats, void* stream);
/* Copy n log slots starting at `first` of (track, group) to device buffers rows [n x 5] / flags [n] (first + n <=
 * capacity; slots at or past the group's count hold stale data). Enqueued; no host synchronisation. */
int spef_score_log(spef_score* score, int track, int group, int first, int n, float* rows, int* flags, void* stream);
int spef_score_destroy(spef_score* score);

/* Pose tracking for video (opt-in; nothing calls it unless asked): an error-state Kalman filter per video stream over the
 * per-frame pose of any head (spef_decode's, spef_decode_keypoints' or spef_refine_keypoints' outputs), on the device
 * (Tracking path; spef_amd/spe/track.py is the NumPy twin and states every step).
 *
 * State per stream: unit quaternion q (scalar first), position t, angular rate w [rad / frame] (a left perturbation in
 * the camera frame, R_{k+1} = exp([w]x) R_k: the convention of spef_refine_keypoints, whose cov is a measurement
 * covariance as it stands), velocity v [m / frame] and the 12 x 12 covariance P of the error state (theta, t, w, v).
 * One step is one frame: constant velocity, P- = F P F^T + Q with F = [[I6, I6], [0, I6]] (small rotations between
 * frames). All arithmetic is fp64; the state stays on the device as fp64, so results do not depend on how a sequence
 * is cut into calls, nor on the number of streams.
 *
 * spef_track_params: q[4] process variances added per frame to the (theta, t, w, v) blocks; p0[4] the initial
 *   variances of the blocks; r[2] the measurement variances (theta, t) of a row without a usable covariance; cov_scale
 *   multiplies a supplied covariance; gate_chi2 gates on the Mahalanobis distance d2 = y^T S^-1 y (0 = no gate);
 *   max_coast: a gated row that would be coasted frame number max_coast + 1 in a row starts the track again instead.
 * spef_track_create: n_streams in 1..65536, every parameter finite and >= 0 (SPEF_ERR_ARG otherwise); all streams start
 *   without a track. The context is used for its device and its profiler only.
 * spef_track_step: T time steps of all S streams, time-major (row t * S + s; S must equal n_streams, T >= 1;
 *   SPEF_ERR_ARG otherwise or for a null required pointer, with nothing enqueued).
 *   quat [T*S x 4] / pos [T*S x 3]  the measured poses; cov (or NULL) [T*S x 36] their row-major 6 x 6 covariances, order
 *     (w_x, w_y, w_z, t_x, t_y, t_z), symmetrised; a row with a non-finite entry uses r. status (or NULL) [T*S] the
 *     decode status: a row with any of bits 1 | 2 | 4 | 8 is an invalid measurement (16 and 32 are informational), as is
 *     one with a non-finite or zero quaternion, a non-finite position or an S = P-[0:6, 0:6] + R that is not positive
 *     definite.
 *   quat_out / pos_out  the tracked pose (they may alias quat / pos); the quaternion is unit and keeps the hemisphere of
 *     the stream's previous one. d2 (or NULL) [T*S] the Mahalanobis distance (0 on the row that starts a track, NaN
 *     when none was computed). cov_out (or NULL) [T*S x 36] the pose block P[0:6, 0:6]; rates_out (or NULL)
 *     [T*S x 6] (w, v).
 *   track_status [T*S] (a word of its own, not the decode status): 1 = measurement invalid, the row is the prediction;
 *     2 = gated, likewise; 4 = the track was started again from this row (with 2); 8 = no track and no valid measurement
 *     to start one: the row passes through unchanged (with 1; d2, cov_out and rates_out are NaN).
 *   One wave per stream; no atomics, no allocation and no host synchronisation: it can follow the decode on a stream and
 *   be stream-captured.
 * spef_track_reset: forget the track of one stream (all streams: -1). spef_track_get_state / spef_track_set_state:
 *   copy the state of streams [first_stream, first_stream + n) to / from a device buffer of n *
 *   SPEF_TRACK_STATE_DOUBLES doubles: have (0 / 1), consecutive coasted frames, 0, q[4], t[3], w[3], v[3], P[144]
 *   row-major. SPEF_ERR_ARG for a stream index out of range. All three are enqueued; no host synchronisation. */
typedef struct spef_track spef_track;
typedef struct { double q[4], p0[4], r[2], cov_scale, gate_chi2; int max_coast; } spef_track_params;
#define SPEF_TRACK_STATE_DOUBLES 160   /* have, coast, 0, q[4], t[3], w[3], v[3], P[144] row-major */
int spef_track_create(spef_ctx* ctx, int n_streams, const spef_track_params* params, spef_track** out);
int spef_track_reset(spef_track* track, int stream, void* stream_hip);
int spef_track_get_state(spef_track* track, int first_stream, int n, double* out_device, void* stream_hip);
int spef_track_set_state(spef_track* track, int first_stream, int n, const double* in_device, void* stream_hip);
int spef_track_step(spef_track* track, const float* quat, const float* pos, const float* cov, const int* status,
                    int T, int S, float* quat_out, float* pos_out, float* d2, float* cov_out, float* rates_out,
                    int* track_status, void* stream_hip);
/* spef_track_step with up to K (1..SPEF_MODES_MAX) orientation candidates per row, the outputs of spef_decode_modes
 * (K = its k_max): the tracker resolves the ambiguity by temporal association. mode_quat [T*S x K x 4], mode_mass
 * [T*S x K], mode_cov [T*S x K x 9], n_modes [T*S]; pos [T*S x 3] and cov [T*S x 36] (required: spef_decode_cov's
 * output, which supplies the t block) are shared by a row's candidates. Candidate k < n_modes is valid when its
 * quaternion is finite and non-zero and its mass is finite and > 0; its covariance C_k is cov with the block
 * [0:3, 0:3] replaced by mode_cov[k], then treated as spef_track_step treats cov. With a track the candidate of
 * smallest cost_k = d2_k + 2 sum_j ln L_k[j][j] - 2 ln mass_k (twice the negative log-likelihood of the innovation
 * under S_k = P-[0:6, 0:6] + R_k = L_k L_k^T, weighted by the mass; a failed pivot makes the candidate invalid; ties to
 * the lowest k) is the measurement; without a track the lowest valid k (the heaviest mode) is. With no valid candidate
 * the measurement is invalid. Everything else -- gating on the chosen d2, coasting, the update, the outputs -- is
 * spef_track_step's; with K = 1 the two agree bit for bit. chosen [T*S]: the index of the candidate taken, -1 when
 * none. A row that passes through (track_status 1 | 8) returns candidate 0 as it came. Both steps may be mixed on one
 * tracker. SPEF_ERR_ARG, with nothing enqueued, for a NULL required pointer, K out of range, S or T as above. */
int spef_track_step_modes(spef_track* track, const float* mode_quat, const float* mode_mass, const float* mode_cov,
                          const int* n_modes, int K, const float* pos, const float* cov, const int* status, int T,
                          int S, float* quat_out, float* pos_out, float* d2, float* cov_out, float* rates_out,
                          int* track_status, int* chosen, void* stream_hip);
int spef_track_destroy(spef_track* track);

/* Fixed-interval smoothing of a recorded video (opt-in): a Rauch-Tung-Striebel backward pass over the tracker's
 * posteriors, so that frame k is estimated from every frame of the window and not only from frames 0..k (DESIGN.md
 * section 3, Smoothing path; spef_amd/spe/smooth.py is the NumPy twin and states every step and the order of every
 * sum). It is the RTS recursion under the filter's own model, F = [[I6, I6], [0, I6]] (small rotations between
 * frames), on the error state (theta, t, w, v); it reads no measurement. All arithmetic is fp64.
 *
 * spef_track_history: a device buffer of capacity frames x n_streams rows x SPEF_TRACK_STATE_DOUBLES doubles, time-major
 *   (frame f, stream s at row f * n_streams + s), and the backward pass's workspace. A row is the tracker's state after
 *   that frame as spef_track_get_state lays it out, with the frame's track_status in slot 2. The number of frames
 *   recorded is kept by the host in the handle: every call below is checked and sized by it, so a stream capture
 *   records the frame positions of the calls it holds.
 * spef_track_history_create: capacity >= 1 and capacity * n_streams * 36 <= 2^31 - 1 (the rows one spef_track_smooth
 *   call may cover; SPEF_ERR_ARG otherwise); it copies the tracker's parameters, and belongs to that tracker. The only
 *   call here that allocates or synchronises. spef_track_history_reset: forget every frame (nothing is enqueued).
 *   spef_track_history_count: write the number of frames recorded to a device int (enqueued).
 * spef_track_step_hist: spef_track_step, bit for bit in its outputs and in the tracker's state, that also appends the T
 *   frames to the history. SPEF_ERR_ARG, with nothing enqueued, for what spef_track_step refuses, a history of another
 *   tracker, or more frames than the capacity has left.
 * spef_track_history_push: append the tracker's current state as one more frame, with track_status [n_streams] (device)
 *   as its status words -- how a caller records after spef_track_step_modes or after live T = 1 steps. SPEF_ERR_ARG for
 *   a NULL pointer, a history of another tracker or a full history.
 * spef_track_smooth: smooth the frames first .. first + T - 1 (first >= 0, T >= 1, first + T <= the frames recorded;
 *   SPEF_ERR_ARG otherwise or for a NULL required pointer, with nothing enqueued), every stream on its own.
 *   quat_io [T*S x 4] / pos_io [T*S x 3]  the filter's outputs for these rows, overwritten by the smoothed pose; the
 *     quaternion is unit and keeps the hemisphere of the filter's output for the row. cov_out (or NULL) [T*S x 36] the
 *     pose block of P^s, symmetric bit for bit; rates_out (or NULL) [T*S x 6] the smoothed (w, v). Without cov_out no
 *     covariance is smoothed at all; the pose does not depend on it, bit for bit.
 *   smooth_status [T*S]: 0 = smoothed; 1 = the row has no track: quat_io / pos_io are left untouched, cov_out and
 *     rates_out are NaN; 2 = a chain ends at this row, which is the filter's (x^s = x, P^s = P): the window's last
 *     frame, a row whose successor has no track or carries track_status & 4 (nothing is smoothed across a
 *     re-initialisation), and, with 4 as well, a row whose P- of the next frame has a Cholesky pivot that is not
 *     positive and finite.
 *   With G = P F^T (P-)^-1 (through the Cholesky factor of P-; (P-, q-, t-) are the filter's prediction from row k):
 *     delta = G [Log(q^s_{k+1} (x) conj(q-)), t^s_{k+1} - t-, w^s_{k+1} - w_k, v^s_{k+1} - v_k], q^s_k =
 *     normalise(exp(delta_theta) (x) q_k), (t, w, v)^s_k = (t, w, v)_k + delta, P^s_k = P_k + G (P^s_{k+1} - P-) G^T.
 *   Two kernels: one wave per (frame, stream) for the gains, one wave per stream for the chain. No atomics, no
 *   allocation, no host synchronisation: it can follow the tracker on a stream and be stream-captured. */
typedef struct spef_track_history spef_track_history;
int spef_track_history_create(spef_track* track, int capacity, spef_track_history** out);
int spef_track_history_reset(spef_track_history* hist);
int spef_track_history_count(spef_track_history* hist, int* count_device, void* stream_hip);
int spef_track_history_push(spef_track_history* hist, spef_track* track, const int* track_status, void* stream_hip);
/* Copy the rows of frames first .. first + T - 1 to a device buffer of T * n_streams * SPEF_TRACK_STATE_DOUBLES doubles
 * (first >= 0, T >= 1, first + T <= the frames recorded; SPEF_ERR_ARG otherwise). Enqueued. */
int spef_track_history_get(spef_track_history* hist, int first, int T, double* out_device, void* stream_hip);
int spef_track_step_hist(spef_track* track, spef_track_history* hist, const float* quat, const float* pos,
                         const float* cov, const int* status, int T, int S, float* quat_out, float* pos_out, float* d2,
                         float* cov_out, float* rates_out, int* track_status, void* stream_hip);
int spef_track_smooth(spef_track_history* hist, int first, int T, float* quat_io, float* pos_io, float* cov_out,
                      float* rates_out, int* smooth_status, void* stream_hip);
int spef_track_history_destroy(spef_track_history* hist);

/* Histogram observers for the INT8 calibration: the statistic of every activation-quantizer input of the float model,
 * accumulated on the device over as many frames as the caller streams (Calibration path;
 * spef_amd.quant.observe_host is the NumPy twin and scales_from_stats turns the counts into scales).
 *
 * Statistic of a float32 value x with b = bits(|x|) as uint32: b >= 0x7f800000 (non-finite) counts in n_nonfinite and
 * nowhere else; b < 103 << 23 (|x| < 2^-24: zeros, -0, denormals) in n_under; b >= 135 << 23 (|x| >= 2^8) in n_over;
 * otherwise in bin k = (b - (103 << 23)) >> 15 of 8192 (32 binades x 256 sub-bins; the upper edge of bin k is the float
 * with bits ((k + 1) << 15) + (103 << 23)). max_bits = max of b over the finite values. Every count is an exact
 * uint64 and depends neither on launch geometry nor on how the frames are cut into calls.
 *
 * Taps (one per quantizer, in spef_amd.quant's QParams order; n_blocks inverted residuals in the loaded model):
 *   0 image, 1 stem, 2 + 3 (i - 1) + {0, 1, 2} = quant / expand / dw of block i (1-based), 2 + 3 n_blocks final,
 *   3 + 3 n_blocks last. quant of block i >= 2 sees the block input and, for a residual block, the project output
 *   before the add; expand is absent when t == 1; taps that do not exist stay empty.
 *
 * spef_observer_create: taps from the model loaded in ctx; allocates all state (zeroed).
 * spef_observe: the fp32 schedule (one kernel per conv) with the observer enqueued after every launch; features (or
 *   NULL) receives what spef_backbone writes, bit-identical. SPEF_ERR_STATE unless the loaded blob is fp32 and
 *   spef_reserve covers the size; SPEF_ERR_ARG for an observer created on a model with another op list. No allocation
 *   and no host synchronisation: it can be stream-captured.
 * spef_observer_update: feeds n float32 values of any device tensor (4-byte aligned) into a tap. SPEF_ERR_ARG for a
 *   bad tap or n < 0; n == 0 is a no-op.
 * spef_observer_read: copies the records of taps [first_tap, first_tap + n) to out_device, per tap 8 + n_bins uint64:
 *   n_total, n_under, n_over, n_nonfinite, max_bits, 0, 0, 0, then the bins. Enqueued; no host synchronisation. */
typedef struct spef_observer spef_observer;
int spef_observer_create(spef_ctx* ctx, spef_observer** out);
int spef_observer_info(const spef_observer* obs, int* n_taps, int* n_bins);
int spef_observer_reset(spef_observer* obs, void* stream);
int spef_observe(spef_ctx* ctx, spef_observer* obs, const void* input, int layout, int B, int H, int W,
                 float* features, void* stream);
int spef_observer_update(spef_observer* obs, int tap, const float* x, int64_t n, void* stream);
int spef_observer_read(spef_observer* obs, int first_tap, int n, uint64_t* out_device, void* stream);
int spef_observer_destroy(spef_observer* obs);

/* Keypoint mode (ORI == POS == 'keypoints', config.py:53-58): the 3-D model points (host float32 n x 3,
 * e.g. tangoPoints.mat's 11 Tango keypoints, keypoints_utils.py:31-45), the camera matrix (host float64
 * 3x3 row-major) and the image size the keypoints are normalised by (Camera nu, nv; speed.py:18-32).
 * All or nothing: on any failure (SPEF_ERR_ARG: a null pointer, n outside 4..16, a degenerate -- coplanar -- model;
 * SPEF_ERR_HIP: an allocation or a copy) the previous configuration stays exactly as it was, and a context that had
 * none stays unconfigured (spef_decode_keypoints / spef_refine_keypoints return SPEF_ERR_STATE). */
int spef_set_keypoints(spef_ctx* ctx, const float* kp3d, int n, const double* K, float nu, float nv);

/* Lens distortion of the keypoint camera, OpenCV order (k1, k2, p1, p2[, k3]); n = 0 removes it. The keypoint
 * decode then undistorts the 2-D points as cv2.solvePnP does before EPnP (undistortPoints, 5 iterations) -- the
 * reference passes camera.distCoeffs (keypoints_utils.py:136-142; SPEED+ camera, speed_plus.py:18-40). */
int spef_set_keypoint_distortion(spef_ctx* ctx, const double* dist, int n);

/* SPEUtils.last_activ (sigmoid, spe_utils.py:68) + KeyPoints.decode_batch (keypoints_utils.py:152-174):
 * raw [B x 2(n+1)] (origin + n keypoints) -> optional kp_out (sigmoid values, same shape), quat [B x 4],
 * pos [B x 3] by batched EPnP (cv2.SOLVEPNP_EPNP semantics) + dcm2quat. status bit 8 = EPnP failure. */
int spef_decode_keypoints(spef_ctx* ctx, const float* raw, int B, int apply_sigmoid, float* kp_out, float* quat,
                          float* pos, int* status, void* stream);

/* Robust pose refinement behind EPnP (opt-in; nothing calls it unless asked): Levenberg-Marquardt on the reprojection
 * error over the pose itself, R <- exp([w]x) R, t <- t + dt, in fp64, on the observations spef_decode_keypoints solves
 * on (float32 pixels, origin dropped, undistorted when distortion is configured; pinhole K).
 *   kp        [B x 2(n+1)] normalised keypoints after the sigmoid (spef_decode_keypoints' kp_out).
 *   weights   NULL or [B x n] per-point confidences c_i >= 0 (NULL: all 1).
 *   huber_px  Huber threshold in pixels on the point's residual norm e_i; 0 = plain least squares. Loss: c_i e_i^2 up
 *             to the threshold, c_i (2 d e_i - d^2) beyond (IRLS weight c_i d / e_i).
 *   quat_inout / pos_inout  the start pose (EPnP's, the classification head's or the previous frame's), replaced by the
 *             refined one; the quaternion keeps the start's hemisphere. A problem in which no trial was accepted keeps
 *             its input bit for bit.
 *   Damping starts at 1e-3, x 1/10 (floor 1e-9) on an accepted trial, x 10 otherwise; a trial is accepted only when the
 *   cost falls strictly and every point stays in front of the camera. Stops on a step below 1e-10 (rad, and relative to
 *   |t|), damping above 1e12, or after max_iters trials (1..100).
 *   fit   [B x 4] (may be NULL): unweighted reprojection RMS in px before / after, minimised cost before / after.
 *   cov   [B x 36] (may be NULL): row-major 6 x 6 pose covariance s^2 (J^T W J)^-1 at the final pose, order
 *         (w_x, w_y, w_z, t_x, t_y, t_z), s^2 = cost_after / max(2 m - 6, 1), m = points with c_i > 0; NaN when the
 *         normal matrix is singular.
 *   iters [B] (may be NULL): trials run.
 *   status [B] is ORed into, not cleared: bit 16 = not refined, the pose is untouched and fit / cov are NaN (the row
 *         carries bit 8; a non-finite keypoint, weight or pose; a negative weight; a point at Z <= 0; fewer than 3
 *         points with c_i > 0), bit 32 = stopped at max_iters (the pose is the best accepted one).
 * Uses the model, camera and distortion of spef_set_keypoints / spef_set_keypoint_distortion (SPEF_ERR_STATE when not
 * set). SPEF_ERR_ARG: a null required pointer, B <= 0, max_iters outside 1..100, huber_px negative or not finite.
 * No allocation, no host synchronisation: it can follow spef_decode_keypoints on the same stream. */
int spef_refine_keypoints(spef_ctx* ctx, const float* kp, const float* weights, int B, int max_iters, float huber_px,
                          float* quat_inout, float* pos_inout, float* fit, float* cov, int* iters, int* status,
                          void* stream);

/* Outlier-robust keypoint decode (opt-in; nothing calls it unless asked): exhaustive 3-point consensus between
 * spef_decode_keypoints and spef_refine_keypoints, on the observations both solve on. A model has n <= 16 points, so
 * all C(n, 3) <= 560 minimal samples are solved and scored: no sampling, no seed, and a problem's result does not depend
 * on its batch. Candidates are the points with c_i > 0 (all of them when weights is NULL). Every triple i < j < k of
 * candidates (index = its rank among all C(n, 3) triples in lexicographic order; a triple whose model triangle is
 * degenerate is skipped) is solved by P3P in fp64 (Grunert's quartic, closed-form roots + two Newton steps; up to four
 * poses). A hypothesis is valid when every model point has Z > 0; its cost is the sum over the candidates of
 * min(e_i^2, inlier_px^2), e_i = reprojection error in pixels. The lowest cost wins (ties: lowest triple, then lowest
 * root in ascending order); its inliers are the candidates with e_i^2 < inlier_px^2.
 *   kp        [B x 2(n+1)] normalised keypoints after the sigmoid (spef_decode_keypoints' kp_out).
 *   weights   NULL or [B x n] confidences c_i >= 0.
 *   quat_inout / pos_inout  the start pose (EPnP's). On consensus: replaced by the winning hypothesis, the quaternion
 *             unit and on the start's hemisphere (when the start is finite and nonzero).
 *   weights_out [B x n]: c_i (or 1) for inliers, 0 otherwise: the weights to hand to spef_refine_keypoints.
 *   info  [B x 4] (may be NULL): inliers, winning triple index, winning root, hypotheses scored.
 *   cost  [B] (may be NULL): the winning cost.
 *   status [B] is ORed into, not cleared: bit 64 = no consensus (a non-finite keypoint or weight, a negative weight,
 *         fewer than 3 candidates, no valid hypothesis, fewer inliers than min_inliers). The pose is then untouched bit
 *         for bit, weights_out is the input confidences (or 1), cost is NaN and info is 0, -1, -1, scored. The bit is
 *         informational, as 16 and 32 are. Bit 8 is not read.
 * SPEF_ERR_STATE without spef_set_keypoints. SPEF_ERR_ARG, with nothing enqueued: a null required pointer, B < 1,
 * inlier_px not finite or <= 0, min_inliers outside 4..n. No allocation, no atomics, no host synchronisation. */
int spef_consensus_keypoints(spef_ctx* ctx, const float* kp, const float* weights, int B, float inlier_px,
                             int min_inliers, float* quat_inout, float* pos_inout, float* weights_out, int* info,
                             float* cost, int* status, void* stream);
/* The same call with one more output: pose64 [B x 12] (may be NULL), the winning hypothesis as it was scored, before the
 * float32 rounding of quat / pos: R row-major (9), then t (3); NaN on a row with bit 64. A float32 pose reprojects
 * to about 1e-3 px at best; this one lets a caller verify the minimal solve itself. */
int spef_consensus_keypoints_f64(spef_ctx* ctx, const float* kp, const float* weights, int B, float inlier_px,
                                 int min_inliers, float* quat_inout, float* pos_inout, float* weights_out, int* info,
                                 float* cost, double* pose64, int* status, void* stream);

/* Input preprocessing on the device (SPEDataset.__getitem__ + transforms.Resize(img_size), utils.py:212-249,
 * speed.py:66-69): decoded frames uint8 [B x Hin x Win x 3] (RGB, HWC) -> uint8 [B x H x W x 3], bit-identical to
 * Pillow's Image.resize((W, H), BILINEAR). The result feeds spef_forward with SPEF_IN_U8_NHWC (ToTensor's /255
 * is fused into the stem). Temporary storage is owned by the context. */
int spef_preprocess(spef_ctx* ctx, const uint8_t* frames, int B, int Hin, int Win, uint8_t* out, int H, int W,
                    void* stream);

/* Track-guided region of interest for keypoint mode (opt-in; nothing calls it unless asked): where the tracker expects
 * the target, the network sees only that part of the frame, cropped and resized to its input, and the keypoints it
 * gives are mapped back to the full frame exactly (an affine map), so that spef_decode_keypoints(apply_sigmoid = 0),
 * spef_consensus_keypoints and spef_refine_keypoints take them unchanged (ROI path;
 * spef_amd/spe/roi.py is the NumPy twin of the prediction, the box rule and the un-mapping and states every step).
 * Keypoint mode only: a crop under a soft-classification head changes the apparent attitude.
 *
 * spef_track_predict: the one-frame-ahead pose of streams [first_stream, first_stream + n) from the tracker's state,
 *   which it does not change: quat_out [n x 4] = normalise(exp([w]x) q) in the hemisphere of q, pos_out [n x 3] =
 *   t + v (fp64, rounded to float32; the conventions of spef_track_step), have_out [n] = 1 where the stream has a
 *   track, else 0 with a zero pose. SPEF_ERR_ARG for a null pointer or a stream index out of range.
 * spef_roi_boxes: the box of B poses in frames Hin x Win for a network input H x W, in fp64 without fused
 *   multiply-adds: project the origin and the n model points of spef_set_keypoints with K (quat2dcm of the quaternion
 *   as given, spe/utils.py:10-53) and, when spef_set_keypoint_distortion is on, the forward distortion of
 *   KeyPoints.project (keypoints_utils.py:77-82); take min and max over the n + 1 points
 *   (create_bbox_from_keypoints, :176-198); grow each side by margin (a fraction of the side) on both ends; raise
 *   each side to min_side; widen or heighten about the centre to the aspect W / H; round: w = floor(w + 0.5),
 *   x0 = floor(cx - w / 2 + 0.5), x1 = x0 + w, likewise in y; shift the box into the frame without changing its size.
 *   have (or NULL) [B]: spef_track_predict's flag.
 *   box_out [B x 4] int32 (x0, y0, x1, y1), x1 / y1 exclusive; status [B]: bit 1 = the row got the full frame
 *   (0, 0, Win, Hin): have is 0, the pose is not finite, a point has Z <= 0, a pixel is not finite, or the grown box
 *   is wider than Win or taller than Hin. SPEF_ERR_ARG: a null required pointer, a size below 1, margin negative or
 *   not finite, min_side below 1 or not finite; SPEF_ERR_STATE without spef_set_keypoints.
 * spef_preprocess_roi: spef_preprocess with one box per frame: frames uint8 [B x Hin x Win x 3], box [B x 4] (device,
 *   as spef_roi_boxes writes it) -> out uint8 [B x H x W x 3], bit-identical to Pillow's
 *   Image.crop(box).resize((W, H), BILINEAR) -- crop, then resize: no pixel outside the box is read, unlike
 *   resize(..., box=box). The coefficient tables are computed on the device per frame and axis (Pillow's
 *   precompute_coeffs, fp64) into tables the context owns; one fused kernel then runs both passes on tiles of the
 *   output through an 8-bit LDS tile, with Pillow's rounding between them and no temporary in device memory.
 *   status (or NULL) [B]: 0, or bit 2 for a box that is not inside the frame or has a side below 1 (a caller's own:
 *   spef_roi_boxes makes none); such a frame is written as zeros and nothing outside the frames is read. B <= 65535.
 *   The tables grow with B as spef_preprocess' temporary does; a call at a shape seen before allocates nothing.
 * spef_roi_unmap_keypoints: raw [B x 2(n+1)] head output of the crops -> kp_out (same shape), the normalised
 *   full-frame keypoints: the sigmoid exactly as spef_decode_keypoints applies it (float32; skipped when apply_sigmoid
 *   is 0), then u = (x0 + s_u (x1 - x0)) / nu, v = (y0 + s_v (y1 - y0)) / nv in fp64, rounded once to float32.
 *   SPEF_ERR_STATE without spef_set_keypoints.
 * All four only enqueue on `stream`: no host synchronisation, and they can be stream-captured once the tables exist. */
#define SPEF_ROI_FULL_FRAME 1   /* spef_roi_boxes' status: the row fell back to the full frame */
#define SPEF_ROI_BAD_BOX 2      /* spef_preprocess_roi's status: box not inside the frame, frame written as zeros */
int spef_track_predict(spef_track* track, int first_stream, int n, float* quat_out, float* pos_out, int* have_out,
                       void* stream_hip);
int spef_roi_boxes(spef_ctx* ctx, const float* quat, const float* pos, const int* have, int B, int Hin, int Win, int H,
                   int W, double margin, double min_side, int* box_out, int* status, void* stream);
int spef_preprocess_roi(spef_ctx* ctx, const uint8_t* frames, const int* box, int B, int Hin, int Win, uint8_t* out,
                        int H, int W, int* status, void* stream);
int spef_roi_unmap_keypoints(spef_ctx* ctx, const float* raw, const int* box, int B, int apply_sigmoid, float* kp_out,
                             void* stream);

/* Head fit (opt-in; nothing calls it unless asked): fit the URSONet head's two Linear layers (ursonet.py:17-25) on the
 * device over cached backbone features, the backbone frozen (Head-fit path;
 * spef_amd/solver/head_fit.py is the NumPy twin and states every step, the hash and the order of every float32
 * operation). It stands where the reference's train.py + SPELoss (src/solver/loss.py) + import_optimizer
 * (src/solver/optimizer.py) stand when only the head is trained.
 *
 * spef_features: the backbone through the global mean; pooled_out receives fp32 [B x feat_c] (1280), the values
 *   spef_forward hands to its FC at the same schedule, bit for bit. Needs spef_reserve as spef_forward does. URSONet-head
 *   blobs only (SPEF_ERR_STATE for a keypoint blob, and for an int8 blob, whose pooled buffer holds codes).
 *
 * spef_encode_targets: OrientationSoftClassification.encode (classification_utils.py:85-111) and
 *   PositionSoftClassification.encode (:217-240) of B poses on the context's decode tables: quat [B x 4] / pos [B x 3]
 *   (device, fp64: a float32 quaternion moves a target by more than the reference's own encode is pinned to) ->
 *   ori_soft [B x n_ori bins] / pos_soft [B x n_pos bins] float32; either pair may be NULL. params: the two variances,
 *   (smooth / n_bins_per_dim)^2 / 12 per head, computed by the caller (both > 0 and finite). mask (NULL, or device uint8
 *   [n_ori bins]): the reference's redundant_flags; a masked bin gets kernel 0, the delete_unused_bins = False case.
 *   fp64 without fused multiply-adds, the normalising sum in a fixed order, rounded once to float32. enc_status
 *   [B x 2] (orientation, position; a word of its own): 1 = a non-finite input or a kernel sum that is zero or not finite
 *   (the reference raises there); that row of that head is NaN, its neighbours are untouched. SPEF_ERR_STATE when a table
 *   that is needed is not set. One launch, one workgroup per (row, head); no atomics, no allocation, no host
 *   synchronisation.
 *
 * spef_headfit_create: a trainer for K features (K % 16 == 0) and n_ori + n_pos outputs, independent of the loaded
 *   model's sizes; the context is used for its device and must outlive the trainer. It owns W [Np x K] (Np = n_ori + n_pos
 *   rounded up to 16, rows = ori then pos: the layout of the blob's FC op), bias [Np], two optimizer state tensors of
 *   each shape (SGD: the momentum buffer; Adam: exp_avg, exp_avg_sq), G [Bmax x Np], the dropout copy of X, the logits
 *   and a step counter, all on the device, all zero at first. The only call here that allocates or synchronises.
 *   spef_headfit_params:
 *     ori_mode  SPEF_CLASSIFICATION (SPEF_REGRESSION: SPEF_ERR_ARG, out of scope). pos_mode SPEF_CLASSIFICATION, or
 *               SPEF_REGRESSION with n_pos == 3.
 *     optimizer SPEF_HEADFIT_SGD (torch.optim.SGD with momentum, dampening 0) or SPEF_HEADFIT_ADAM (torch.optim.Adam),
 *               both with L2 weight decay added to the gradient: what import_optimizer builds.
 *     beta, norm_distance  SPELoss' (loss.py:125). momentum; beta1, beta2, eps (Adam); weight_decay >= 0.
 *     dropout_p in [0, 1): nn.Dropout on the orientation branch's input (the reference's 0.2; 0 = off); seed.
 *     Bmax >= 1: the largest batch of a step.
 * spef_headfit_step: one optimisation step on X [B x K] (1 <= B <= Bmax), ori_target [B x n_ori] soft labels,
 *   pos_target [B x n_pos] soft labels or [B x 3] positions. With train = 0 it is an evaluation: loss only, no dropout,
 *   neither the weights nor the state nor the counter change (grad_out must be NULL).
 *   Loss: orientation and position classification -mean_b sum_i t log softmax(z) (SoftClassLoss, loss.py:109, on
 *   SPEUtils.last_activ's softmax), log p computed as z - max - log(sum) so that a zero probability under a zero target
 *   adds 0; position regression PosRegLoss as written (loss.py:35-37): the Frobenius norm of pred - target over the whole
 *   batch, divided by the target's with norm_distance; total = beta * ori + pos (loss.py:157).
 *   loss_out (or NULL): device float[3] = total, orientation, position. logits_out (or NULL) [B x (n_ori + n_pos)].
 *   grad_out (or NULL) [Np x K] then [Np]: dLoss/dW and dLoss/dbias before weight decay (validation and inspection; the
 *   step itself never writes dW to memory).
 *   lr is a DEVICE pointer to one float, read by the update kernel when it runs, and the step counter (the dropout
 *   hash's step, Adam's bias corrections) is read and advanced on the device: a captured step replays correctly, each
 *   replay one step further, at whatever the caller has written to *lr meanwhile.
 *   No allocation, no host synchronisation and no atomics; every sum has a fixed order, so a step is deterministic.
 * spef_headfit_set_weights / _get_weights: copy W [(n_ori + n_pos) x K] and bias [n_ori + n_pos] (no padding) from / to
 *   device buffers. spef_headfit_get_state: the two state tensors of W and of bias, same shapes (any may be NULL).
 *   spef_headfit_get_g: G = dLoss/dlogits [B x (n_ori + n_pos)] of the last step or evaluation of B rows (1 <= B <= Bmax;
 *   validation and inspection). spef_headfit_get_raw: one of the trainer's tensors as it lies in memory, padding rows
 *   included: `which` = SPEF_HEADFIT_RAW_W / _S1 / _S2 [Np x K], _BIAS / _BIAS_S1 / _BIAS_S2 [Np], _XD [Bmax x K] (the
 *   dropout copy of X the last training step wrote); SPEF_ERR_ARG for a tensor the trainer does not have (S2 under SGD,
 *   XD with dropout off). spef_headfit_reset_state zeroes the state and the step counter. All enqueued on `stream`.
 * spef_headfit_load_model / spef_headfit_commit: copy the head from / to the context's FC op, device to device,
 *   enqueued. SPEF_ERR_STATE without a loaded fp32-head URSONet blob (int8 blobs hold an int8 head), SPEF_ERR_ARG unless
 *   K, n_ori and n_pos equal the blob's. After a commit spef_forward uses the new head. */
enum spef_headfit_optimizer { SPEF_HEADFIT_SGD = 0, SPEF_HEADFIT_ADAM = 1 };
enum spef_headfit_raw {
  SPEF_HEADFIT_RAW_W = 0, SPEF_HEADFIT_RAW_BIAS, SPEF_HEADFIT_RAW_S1, SPEF_HEADFIT_RAW_BIAS_S1, SPEF_HEADFIT_RAW_S2,
  SPEF_HEADFIT_RAW_BIAS_S2, SPEF_HEADFIT_RAW_XD
};
typedef struct {
  int ori_mode, pos_mode, optimizer, norm_distance, Bmax;
  uint32_t seed;
  double beta, momentum, beta1, beta2, eps, weight_decay, dropout_p;
} spef_headfit_params;
typedef struct spef_headfit spef_headfit;
typedef struct { double ori_var, pos_var; } spef_encode_params;
int spef_features(spef_ctx* ctx, const void* input, int layout, int B, int H, int W, float* pooled_out, void* stream);
/* The width of a spef_features row (the blob's feat_c, 1280 for MobileNetV2); SPEF_ERR_STATE without weights. */
int spef_feature_width(const spef_ctx* ctx, int* feat_c);
int spef_encode_targets(spef_ctx* ctx, const double* quat, const double* pos, int B, const spef_encode_params* params,
                        const uint8_t* mask, float* ori_soft, float* pos_soft, int* enc_status, void* stream);
int spef_headfit_create(spef_ctx* ctx, int K, int n_ori, int n_pos, const spef_headfit_params* params,
                        spef_headfit** out);
int spef_headfit_step(spef_headfit* trainer, const float* X, const float* ori_target, const float* pos_target, int B,
                      const float* lr, int train, float* loss_out, float* logits_out, float* grad_out, void* stream);
int spef_headfit_set_weights(spef_headfit* trainer, const float* W, const float* bias, void* stream);
int spef_headfit_get_weights(spef_headfit* trainer, float* W, float* bias, void* stream);
int spef_headfit_get_state(spef_headfit* trainer, float* W_s1, float* bias_s1, float* W_s2, float* bias_s2,
                           void* stream);
int spef_headfit_get_g(spef_headfit* trainer, int B, float* G, void* stream);
int spef_headfit_get_raw(spef_headfit* trainer, int which, float* out, void* stream);
int spef_headfit_reset_state(spef_headfit* trainer, void* stream);
int spef_headfit_load_model(spef_headfit* trainer, spef_ctx* ctx, void* stream);
int spef_headfit_commit(spef_headfit* trainer, spef_ctx* ctx, void* stream);
int spef_headfit_destroy(spef_headfit* trainer);

/* Schedule options (both choices of each are bit-identical; the parity tests switch them):
 * SPEF_OPT_FUSE_BLOCKS (default 1): each inverted-residual block as one fused kernel (expand + depthwise + project
 *   on-chip); 0 = one kernel per conv (the reference's module-by-module schedule).
 * SPEF_OPT_WAVESPEC (default 2): role-split fused kernels for the low-resolution blocks. 2 = three-stage pipeline
 *   (MFMA waves expand + project, VALU waves depthwise); 1 = two-stage (expand waves, depthwise + project waves);
 *   0 = LDS-slab fused kernels everywhere.
 * SPEF_OPT_Q8_ROLESPLIT (default 0): int8 blobs run blocks 8-17 as role-split kernels (expand waves vs depthwise +
 *   project waves) instead of the LDS-slab kernels: faster with one batch in flight, slower when several batches
 *   share the GPU (the role-split workgroups hold a CU's LDS; DESIGN.md section 3, INT8 path).
 * (Kernel-tuning knobs used by the sweep tools are internal: csrc/spef_tuning.hpp.) */
enum spef_option {
  SPEF_OPT_FUSE_BLOCKS = 1,
  SPEF_OPT_WAVESPEC = 6,
  SPEF_OPT_Q8_ROLESPLIT = 7
};
int spef_set_option(spef_ctx* ctx, int option, int value);

/* Host-only validation of a weight blob (no device needed: build tools and CPU tests use it). Checks the header,
 * the op table, every tensor's extent against the data section (from the op geometry) and the head widths;
 * returns SPEF_ERR_BLOB with a message on the first problem. Outputs may be NULL. */
int spef_validate_blob(const void* host_blob, size_t bytes, int* dtype, int* head, int* n_out0, int* n_out1);

/* Weight broadcast over RCCL (xGMI) -- SURVEY.md §8b/§8e: rank `root` sends the blob its context holds, every
 * other rank's context receives and loads it (header, op table and data section, device to device; no host
 * round trip). Collective: every rank of `comm` calls it with the same root. Replaces each rank reading
 * parameters.pt itself (modeling/model.py:261-266).
 * Failure handling (the reference's analogue is the socket timeouts of spe_nvidia.py:82-103):
 *  - the ranks agree (all-reduce MAX of a status word) after the header broadcast and again after the receivers
 *    have staged the blob; no rank enters a data collective unless all are ready, no receiver commits the new
 *    model unless all staged it, and every rank returns the same status, naming the failing rank;
 *  - every wait is bounded by the communicator's timeout; an RCCL error or a timeout aborts the communicator
 *    (ncclCommAbort) and returns SPEF_ERR_COMM -- the handle is then dead (spef_comm_destroy only forgets it).
 * On any failure a receiving context keeps the model it had.
 * `comm` is an RCCL communicator (ncclComm_t): one made with spef_comm_init (nonblocking, ncclConfig_t.blocking
 * = 0, bounded by `timeout_ms`; <= 0 = 120 s) from an id that rank 0 drew with spef_comm_unique_id and the host
 * shipped to the other ranks (any side channel: torch.distributed, MPI, a file), or the host's own (120 s).
 * spef_comm_abort aborts a communicator from the host (e.g. when the launcher learns a peer died). */
int spef_comm_unique_id(void* id_out, size_t cap);
int spef_comm_init(int device, int nranks, int rank, const void* id, int timeout_ms, void** comm_out);
int spef_comm_abort(void* comm);
int spef_comm_destroy(void* comm);
int spef_bcast_weights(spef_ctx* ctx, void* comm, int root);

/* Per-launch HIP-event profiling of every kernel the context enqueues between begin and end (bench.py's
 * roofline leg). spef_profile_end synchronises, then writes a JSON object
 *   {"<kernel key>": [launches, total_ms, algorithmic_bytes, algorithmic_flops], ...}
 * into buf (host, cap bytes); *needed receives the size required including the terminating NUL. */
int spef_profile_begin(spef_ctx* ctx);
int spef_profile_end(spef_ctx* ctx, char* buf, size_t cap, size_t* needed);

/* On-box measurement (bench.py; SURVEY.md §8d "peaks re-measured by the build's own microbenchmark"), no model
 * involved. spef_measure_peaks runs, on `device`, `reps` timed launches (after one warm-up) of each of: a dense
 * v_mfma_f32_16x16x32_f16 loop, a v_mfma_i32_16x16x64_i8 loop (random operands, 8 independent chains per wave,
 * 4 waves per SIMD), a 4 GiB HBM copy and a 4 GiB HBM read, and writes the best rates: out[0] fp16 TFLOP/s,
 * out[1] int8 TOP/s, out[2] copy GB/s (read + write bytes), out[3] read GB/s, out[4] / out[5] the shader clock in
 * MHz held inside the fp16 / int8 loop (median over workgroups of delta s_memtime / delta s_memrealtime x 100),
 * out[6] / out[7] the stream configuration behind out[2] / out[3] (workgroups per CU x 100 + 16-B loads in flight
 * per thread x 10 + 1 if nontemporal): `out` holds 8 doubles. The calling thread's current device is restored.
 * spef_clock_stamp enqueues n_wg one-wave workgroups on `stream`, each writing (location, s_memtime,
 * s_memrealtime) as three uint64 into the device buffer `out` -- location = XCD id << 8 | HW_ID[15:8] (CU, SH,
 * SE): two stamps around a timed region give the clock held during it (deltas within one CU). */
int spef_measure_peaks(int device, int reps, double* out);
int spef_clock_stamp(void* out, int n_wg, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPEF_H_ */
