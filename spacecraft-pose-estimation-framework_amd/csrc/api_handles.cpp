// Handles that live beside a context (include/spef.h): the video filter, the histogram observers, the pose scorer and
// the pose tracker.
#include <math.h>

#include <algorithm>

#include "spef_ctx.hpp"

std::vector<std::array<uint32_t, 7>> op_geometry(const spef_ctx* c) {
  std::vector<std::array<uint32_t, 7>> g;
  for (const OpDesc& op : c->ops) g.push_back({op.kind, op.cin, op.cout, op.hidden, op.stride, op.expand, op.flags});
  return g;
}

extern "C" {

// ------------------------------------------------------------------------------------------ video filter
struct spef_video {
  int device = 0;
  int S = 0, metric = 0;
  int n_ori = 0, n_pos = 0;              // bin counts of the decode tables at creation
  float nmix[2] = {0.f, 0.f}, alpha[2] = {0.f, 0.f};
  float* state[2] = {nullptr, nullptr};  // [S][n] previous filtered PDFs (ori, pos)
  float* state_sum = nullptr;            // [2][S]
  int* flags = nullptr;                  // [4][S]: ori have, pos have, still pole have, video pole have
  float* poles = nullptr;                // [2][S][4]: still, video
  float* scratch[2] = {nullptr, nullptr};  // filtered PDFs of one chunk when the caller does not want them
  int scratch_T = 0;
};

static VideoHead video_head(const spef_video* v, int k, const float* in, float* filt, float* dist) {
  VideoHead h;
  h.in = in;
  h.filt = filt;
  h.dist = dist;
  h.state = v->state[k];
  h.state_sum = v->state_sum + (size_t)k * v->S;
  h.have = v->flags + (size_t)k * v->S;
  h.n = k ? v->n_pos : v->n_ori;
  h.nmix = v->nmix[k];
  h.alpha = v->alpha[k];
  return h;
}

int spef_video_destroy(spef_video* v) {
  if (!v) return SPEF_OK;
  Dev d(v->device);
  for (int k = 0; k < 2; ++k) {
    if (v->state[k]) hipFree(v->state[k]);
    if (v->scratch[k]) hipFree(v->scratch[k]);
  }
  if (v->state_sum) hipFree(v->state_sum);
  if (v->flags) hipFree(v->flags);
  if (v->poles) hipFree(v->poles);
  delete v;
  return SPEF_OK;
}

int spef_video_create(spef_ctx* c, int n_streams, int metric, float n_ori, float alpha_ori, float n_pos,
                      float alpha_pos, spef_video** out) {
  if (!c || !out) return fail(SPEF_ERR_ARG, "null argument");
  if (n_streams < 1) return fail(SPEF_ERR_ARG, "n_streams must be at least 1");
  if (metric < VM_L2 || metric > VM_WASSERSTEIN) return fail(SPEF_ERR_ARG, "unknown distance metric");
  if (!c->d_ori_bins || !c->d_pos_grid)
    return fail(SPEF_ERR_STATE, "the video filter needs both decode tables (spef_set_decode_tables)");
  // video_scan_kernel keeps a stream's PDF in registers, at most 32 bins per thread (launch_video_scan has the same
  // guard): refuse a larger table here, not at every step. The still-frame position decode has no such limit.
  if (c->n_ori_bins > 8192 || c->n_pos_bins > 8192)
    return fail(SPEF_ERR_ARG, "the video filter takes at most 8192 bins per table, the " +
                                  std::string(c->n_ori_bins > 8192 ? "orientation" : "position") + " table has " +
                                  std::to_string(c->n_ori_bins > 8192 ? c->n_ori_bins : c->n_pos_bins));
  Dev d(c->device);
  spef_video* v = new spef_video;
  v->device = c->device;
  v->S = n_streams;
  v->metric = metric;
  v->n_ori = c->n_ori_bins;
  v->n_pos = c->n_pos_bins;
  v->nmix[0] = n_ori; v->alpha[0] = alpha_ori;
  v->nmix[1] = n_pos; v->alpha[1] = alpha_pos;
  // scratch: at least 64 rows, whole time steps
  v->scratch_T = n_streams >= 64 ? 1 : 64 / n_streams;
  const size_t S = (size_t)n_streams, rows = S * v->scratch_T;
  hipError_t e = hipMalloc(&v->state[0], S * v->n_ori * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&v->state[1], S * v->n_pos * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&v->scratch[0], rows * v->n_ori * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&v->scratch[1], rows * v->n_pos * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&v->state_sum, 2 * S * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&v->flags, 4 * S * sizeof(int));
  if (e == hipSuccess) e = hipMalloc(&v->poles, 8 * S * sizeof(float));
  if (e == hipSuccess) e = hipMemset(v->flags, 0, 4 * S * sizeof(int));
  if (e == hipSuccess) e = hipMemset(v->state_sum, 0, 2 * S * sizeof(float));
  if (e == hipSuccess) e = hipMemset(v->poles, 0, 8 * S * sizeof(float));
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    spef_video_destroy(v);
    return fail(SPEF_ERR_HIP, std::string("spef_video_create: ") + hipGetErrorString(e));
  }
  *out = v;
  return SPEF_OK;
}

int spef_video_reset(spef_video* v, int stream, void* stream_hip) {
  if (!v) return fail(SPEF_ERR_ARG, "null video filter");
  if (stream < -1 || stream >= v->S) return fail(SPEF_ERR_ARG, "stream index out of range");
  Dev d(v->device);
  HIP_TRY(launch_video_reset(v->flags, v->S, stream, (hipStream_t)stream_hip));
  return SPEF_OK;
}

int spef_video_set_state(spef_video* v, int stream, const float* ori_pdf, const float* pos_pdf,
                         const float* still_pole, const float* video_pole, void* stream_hip) {
  if (!v) return fail(SPEF_ERR_ARG, "null video filter");
  if (stream < 0 || stream >= v->S) return fail(SPEF_ERR_ARG, "stream index out of range");
  Dev d(v->device);
  HIP_TRY(launch_video_set_state(video_head(v, 0, nullptr, nullptr, nullptr), video_head(v, 1, nullptr, nullptr, nullptr),
                                 v->poles, v->flags + 2 * (size_t)v->S, v->S, stream, ori_pdf, pos_pdf, still_pole,
                                 video_pole, (hipStream_t)stream_hip));
  return SPEF_OK;
}

int spef_video_step(spef_ctx* c, spef_video* v, const float* ori_soft, const float* pos_soft, int T, int S,
                    float* still_quat, float* ori_filt, float* ori_dist, float* pos_filt, float* pos_dist, float* quat,
                    float* pos, int* status, void* stream_hip) {
  if (!c || !v) return fail(SPEF_ERR_ARG, "null context or video filter");
  if (!ori_soft || !pos_soft || !ori_dist || !pos_dist || !quat || !pos || !status)
    return fail(SPEF_ERR_ARG, "null argument");
  if (S != v->S)
    return fail(SPEF_ERR_ARG, "S = " + std::to_string(S) + ", the filter has " + std::to_string(v->S) + " streams");
  if (T < 1) return fail(SPEF_ERR_ARG, "T must be at least 1");
  if ((int64_t)T * S > 0x7fffffff) return fail(SPEF_ERR_ARG, "too many frames");
  if (c->device != v->device) return fail(SPEF_ERR_ARG, "the filter belongs to another device");
  if (!c->d_ori_bins || !c->d_pos_grid || c->n_ori_bins != v->n_ori || c->n_pos_bins != v->n_pos)
    return fail(SPEF_ERR_STATE, "the decode tables changed since spef_video_create");
  Dev d(c->device);
  hipStream_t s = (hipStream_t)stream_hip;
  // with both filtered-PDF outputs given: one scan, one decode over all T * S frames; otherwise chunks of
  // scratch_T time steps through the filter's own buffers
  const int Tc = (ori_filt && pos_filt) ? T : v->scratch_T;
  for (int t0 = 0; t0 < T; t0 += Tc) {
    const int tc = std::min(Tc, T - t0);
    const size_t r0 = (size_t)t0 * S;
    float* fo = ori_filt ? ori_filt + r0 * v->n_ori : v->scratch[0];
    float* fp = pos_filt ? pos_filt + r0 * v->n_pos : v->scratch[1];
    const VideoHead ho = video_head(v, 0, ori_soft + r0 * v->n_ori, fo, ori_dist + r0);
    const VideoHead hp = video_head(v, 1, pos_soft + r0 * v->n_pos, fp, pos_dist + r0);
    const double px = (double)tc * S * (v->n_ori + v->n_pos);
    HIP_TRY(prof_launch(c, s, "video_scan_kernel", px * 12, px * 20,
                        [&] { return launch_video_scan(ho, hp, tc, S, v->metric, s); }));
    HIP_TRY(prof_launch(c, s, "decode_pdf_kernels", px * 4 + 32.0 * v->n_ori + 24.0 * v->n_pos, px * 30, [&] {
      return launch_decode_pdf(fo, fp, tc * S, v->n_ori, c->d_ori_bins, v->n_pos, c->d_pos_grid, quat + r0 * 4,
                               pos + r0 * 3, status + r0, s);
    }));
  }
  HIP_TRY(prof_launch(c, s, "video_pole_kernel", (double)T * S * 64, 0.0, [&] {
    return launch_video_pole(quat, still_quat, v->poles, v->flags + 2 * (size_t)v->S, T, S, s);
  }));
  return SPEF_OK;
}

// ------------------------------------------------------------------------------------------ histogram observers
int spef_observer_destroy(spef_observer* o) {
  if (!o) return SPEF_OK;
  Dev d(o->device);
  if (o->state) hipFree(o->state);
  delete o;
  return SPEF_OK;
}

int spef_observer_create(spef_ctx* c, spef_observer** out) {
  if (!c || !out) return fail(SPEF_ERR_ARG, "null argument");
  if (!c->loaded) return fail(SPEF_ERR_STATE, "weights not loaded (spef_load_weights)");
  Dev d(c->device);
  spef_observer* o = new spef_observer;
  o->device = c->device;
  o->geom = op_geometry(c);
  for (const OpDesc& op : c->ops) o->n_blocks += (op.kind == OP_IRB || op.kind == OP_QIRB) ? 1 : 0;
  o->n_taps = 4 + 3 * o->n_blocks;
  const size_t bytes = (size_t)o->n_taps * (OBS_COUNTERS + OBS_BINS) * sizeof(uint64_t);
  hipError_t e = hipMalloc(&o->state, bytes);
  if (e == hipSuccess) e = hipMemset(o->state, 0, bytes);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    spef_observer_destroy(o);
    return fail(SPEF_ERR_HIP, std::string("spef_observer_create: ") + hipGetErrorString(e));
  }
  *out = o;
  return SPEF_OK;
}

int spef_observer_info(const spef_observer* o, int* n_taps, int* n_bins) {
  if (!o) return fail(SPEF_ERR_ARG, "null observer");
  if (n_taps) *n_taps = o->n_taps;
  if (n_bins) *n_bins = OBS_BINS;
  return SPEF_OK;
}

int spef_observer_reset(spef_observer* o, void* stream) {
  if (!o) return fail(SPEF_ERR_ARG, "null observer");
  Dev d(o->device);
  HIP_TRY(launch_observe_reset(o->state, (int64_t)o->n_taps * (OBS_COUNTERS + OBS_BINS), (hipStream_t)stream));
  return SPEF_OK;
}

int spef_observer_update(spef_observer* o, int tap, const float* x, int64_t n, void* stream) {
  if (!o) return fail(SPEF_ERR_ARG, "null observer");
  if (tap < 0 || tap >= o->n_taps) return fail(SPEF_ERR_ARG, "tap index out of range");
  if (n < 0) return fail(SPEF_ERR_ARG, "negative element count");
  if (n == 0) return SPEF_OK;
  if (!x || ((uintptr_t)x & 3)) return fail(SPEF_ERR_ARG, "null or misaligned tensor");
  Dev d(o->device);
  HIP_TRY(launch_observe(o->tap(tap), x, n, false, num_cus() * 5, (hipStream_t)stream));
  return SPEF_OK;
}

int spef_observer_read(spef_observer* o, int first_tap, int n, uint64_t* out_device, void* stream) {
  if (!o || !out_device) return fail(SPEF_ERR_ARG, "null argument");
  if (first_tap < 0 || n < 0 || (int64_t)first_tap + n > o->n_taps) return fail(SPEF_ERR_ARG, "taps out of range");
  if (n == 0) return SPEF_OK;
  Dev d(o->device);
  HIP_TRY(hipMemcpyAsync(out_device, o->tap(first_tap), (size_t)n * (OBS_COUNTERS + OBS_BINS) * sizeof(uint64_t),
                         hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return SPEF_OK;
}

// ------------------------------------------------------------------------------------------ pose scoring
static_assert(SPEF_SCORE_FIELDS == SCORE_FIELDS && (int)SPEF_SCORE_FLAGS == (int)SF_FLAGS &&
                  (int)SPEF_SCORE_POS_MAX == (int)SF_POS_MAX,
              "spef_score_field and spef::ScoreField must agree");

struct spef_score {
  spef_ctx* ctx = nullptr;   // profiler of the step / finalize launches
  int device = 0;
  int n_tracks = 0;
  ScoreLog log{};
  float* scratch = nullptr;  // the sort's copies when the capacity exceeds one LDS tile
  unsigned scratch_stride = 0;
};

int spef_score_destroy(spef_score* sc) {
  if (!sc) return SPEF_OK;
  Dev d(sc->device);   // not through ctx: the context may be gone already
  if (sc->log.rows) hipFree(sc->log.rows);
  if (sc->log.flags) hipFree(sc->log.flags);
  if (sc->log.count) hipFree(sc->log.count);
  if (sc->log.dropped) hipFree(sc->log.dropped);
  if (sc->scratch) hipFree(sc->scratch);
  delete sc;
  return SPEF_OK;
}

int spef_score_create(spef_ctx* c, int n_groups, int n_tracks, int capacity, spef_score** out) {
  if (!c || !out) return fail(SPEF_ERR_ARG, "null argument");
  if (n_groups < 1 || n_tracks < 1 || capacity < 1)
    return fail(SPEF_ERR_ARG, "n_groups, n_tracks and capacity must be at least 1");
  if (capacity > (1 << 20)) return fail(SPEF_ERR_ARG, "capacity above 2^20 rows per group");
  if ((int64_t)n_groups * n_tracks > (1 << 16)) return fail(SPEF_ERR_ARG, "more than 65536 (group, track) logs");
  Dev d(c->device);
  spef_score* sc = new spef_score;
  sc->ctx = c;
  sc->device = c->device;
  sc->n_tracks = n_tracks;
  sc->log.n_groups = n_groups;
  sc->log.capacity = capacity;
  const size_t logs = (size_t)n_groups * n_tracks, slots = logs * capacity;
  hipError_t e = hipMalloc(&sc->log.rows, slots * 5 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&sc->log.flags, slots * sizeof(int));
  if (e == hipSuccess) e = hipMalloc(&sc->log.count, logs * sizeof(int));
  if (e == hipSuccess) e = hipMalloc(&sc->log.dropped, logs * sizeof(long long));
  if (e == hipSuccess && (unsigned)capacity > SCORE_TILE) {
    unsigned p = SCORE_TILE;
    while (p < (unsigned)capacity) p <<= 1;
    sc->scratch_stride = p;
    e = hipMalloc(&sc->scratch, logs * 2 * p * sizeof(float));
  }
  if (e == hipSuccess) e = hipMemset(sc->log.count, 0, logs * sizeof(int));
  if (e == hipSuccess) e = hipMemset(sc->log.dropped, 0, logs * sizeof(long long));
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    spef_score_destroy(sc);
    return fail(SPEF_ERR_HIP, std::string("spef_score_create: ") + hipGetErrorString(e));
  }
  *out = sc;
  return SPEF_OK;
}

int spef_score_reset(spef_score* sc, int group, void* stream) {
  if (!sc) return fail(SPEF_ERR_ARG, "null scorer");
  if (group < -1 || group >= sc->log.n_groups) return fail(SPEF_ERR_ARG, "group index out of range");
  Dev d(sc->device);
  HIP_TRY(launch_score_reset(sc->log, sc->n_tracks, group, (hipStream_t)stream));
  return SPEF_OK;
}

int spef_score_step(spef_score* sc, int track, const float* quat, const float* pos, const int* status,
                    const float* quat_true, const float* pos_true, int T, int S, float* rows_out, void* stream) {
  if (!sc) return fail(SPEF_ERR_ARG, "null scorer");
  if (!quat || !pos || !quat_true || !pos_true) return fail(SPEF_ERR_ARG, "null argument");
  if (track < 0 || track >= sc->n_tracks) return fail(SPEF_ERR_ARG, "track index out of range");
  if (S != sc->log.n_groups)
    return fail(SPEF_ERR_ARG, "S = " + std::to_string(S) + ", the scorer has " + std::to_string(sc->log.n_groups) +
                                  " groups");
  if (T < 1) return fail(SPEF_ERR_ARG, "T must be at least 1");
  if ((int64_t)T * S > 0x7fffffff) return fail(SPEF_ERR_ARG, "too many rows");
  spef_ctx* c = sc->ctx;
  Dev d(c->device);
  hipStream_t s = (hipStream_t)stream;
  const double rows = (double)T * S;
  HIP_TRY(prof_launch(c, s, "score_step_kernel", rows * (14 * 4 + 4 + 24 + (rows_out ? 20 : 0)), rows * 60, [&] {
    return launch_score_step(sc->log, track, quat, pos, status, quat_true, pos_true, T, S, rows_out, s);
  }));
  return SPEF_OK;
}

int spef_score_finalize(spef_score* sc, double* stats, void* stream) {
  if (!sc || !stats) return fail(SPEF_ERR_ARG, "null argument");
  spef_ctx* c = sc->ctx;
  Dev d(c->device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(prof_launch(c, s, "score_finalize_kernel", 0.0, 0.0, [&] {
    return launch_score_finalize(sc->log, sc->n_tracks, sc->scratch, sc->scratch_stride, stats, s);
  }));
  return SPEF_OK;
}

int spef_score_log(spef_score* sc, int track, int group, int first, int n, float* rows, int* flags, void* stream) {
  if (!sc || !rows || !flags) return fail(SPEF_ERR_ARG, "null argument");
  if (track < 0 || track >= sc->n_tracks) return fail(SPEF_ERR_ARG, "track index out of range");
  if (group < 0 || group >= sc->log.n_groups) return fail(SPEF_ERR_ARG, "group index out of range");
  if (first < 0 || n < 0 || (int64_t)first + n > sc->log.capacity) return fail(SPEF_ERR_ARG, "slots out of range");
  Dev d(sc->device);
  HIP_TRY(launch_score_read(sc->log, track, group, first, n, rows, flags, (hipStream_t)stream));
  return SPEF_OK;
}

// ------------------------------------------------------------------------------------------ pose tracking
static_assert(SPEF_TRACK_STATE_DOUBLES == TRACK_STATE, "SPEF_TRACK_STATE_DOUBLES and spef::TRACK_STATE must agree");

int spef_track_destroy(spef_track* tr) {
  if (!tr) return SPEF_OK;
  Dev d(tr->device);   // not through ctx: the context may be gone already
  if (tr->state) hipFree(tr->state);
  delete tr;
  return SPEF_OK;
}

int spef_track_create(spef_ctx* c, int n_streams, const spef_track_params* p, spef_track** out) {
  if (!c || !p || !out) return fail(SPEF_ERR_ARG, "null argument");
  if (n_streams < 1 || n_streams > 65536) return fail(SPEF_ERR_ARG, "n_streams must be in 1..65536");
  bool good = std::isfinite(p->cov_scale) && p->cov_scale >= 0 && std::isfinite(p->gate_chi2) && p->gate_chi2 >= 0 &&
              p->max_coast >= 0;
  for (int k = 0; k < 4; ++k)
    good = good && std::isfinite(p->q[k]) && p->q[k] >= 0 && std::isfinite(p->p0[k]) && p->p0[k] >= 0;
  for (int k = 0; k < 2; ++k) good = good && std::isfinite(p->r[k]) && p->r[k] >= 0;
  if (!good) return fail(SPEF_ERR_ARG, "tracker parameters must be finite and not negative");
  Dev d(c->device);
  spef_track* tr = new spef_track;
  tr->ctx = c;
  tr->device = c->device;
  tr->S = n_streams;
  for (int k = 0; k < 4; ++k) {
    tr->prm.q[k] = p->q[k];
    tr->prm.p0[k] = p->p0[k];
  }
  tr->prm.r[0] = p->r[0];
  tr->prm.r[1] = p->r[1];
  tr->prm.cov_scale = p->cov_scale;
  tr->prm.gate_chi2 = p->gate_chi2;
  tr->prm.max_coast = (double)p->max_coast;
  const size_t bytes = (size_t)n_streams * TRACK_STATE * sizeof(double);
  hipError_t e = hipMalloc(&tr->state, bytes);
  if (e == hipSuccess) e = hipMemset(tr->state, 0, bytes);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    spef_track_destroy(tr);
    return fail(SPEF_ERR_HIP, std::string("spef_track_create: ") + hipGetErrorString(e));
  }
  *out = tr;
  return SPEF_OK;
}

int spef_track_reset(spef_track* tr, int stream, void* stream_hip) {
  if (!tr) return fail(SPEF_ERR_ARG, "null tracker");
  if (stream < -1 || stream >= tr->S) return fail(SPEF_ERR_ARG, "stream index out of range");
  Dev d(tr->device);
  double* at = tr->state + (stream < 0 ? 0 : (size_t)stream * TRACK_STATE);
  HIP_TRY(launch_track_reset(at, (int64_t)(stream < 0 ? tr->S : 1) * TRACK_STATE, (hipStream_t)stream_hip));
  return SPEF_OK;
}

int spef_track_get_state(spef_track* tr, int first_stream, int n, double* out_device, void* stream_hip) {
  if (!tr || !out_device) return fail(SPEF_ERR_ARG, "null argument");
  if (first_stream < 0 || n < 1 || (int64_t)first_stream + n > tr->S)
    return fail(SPEF_ERR_ARG, "stream index out of range");
  Dev d(tr->device);
  HIP_TRY(launch_track_copy(out_device, tr->state + (size_t)first_stream * TRACK_STATE, (int64_t)n * TRACK_STATE,
                            (hipStream_t)stream_hip));
  return SPEF_OK;
}

int spef_track_set_state(spef_track* tr, int first_stream, int n, const double* in_device, void* stream_hip) {
  if (!tr || !in_device) return fail(SPEF_ERR_ARG, "null argument");
  if (first_stream < 0 || n < 1 || (int64_t)first_stream + n > tr->S)
    return fail(SPEF_ERR_ARG, "stream index out of range");
  Dev d(tr->device);
  HIP_TRY(launch_track_copy(tr->state + (size_t)first_stream * TRACK_STATE, in_device, (int64_t)n * TRACK_STATE,
                            (hipStream_t)stream_hip));
  return SPEF_OK;
}

int spef_track_step(spef_track* tr, const float* quat, const float* pos, const float* cov, const int* status, int T,
                    int S, float* quat_out, float* pos_out, float* d2, float* cov_out, float* rates_out,
                    int* track_status, void* stream_hip) {
  if (!tr) return fail(SPEF_ERR_ARG, "null tracker");
  if (!quat || !pos || !quat_out || !pos_out || !track_status) return fail(SPEF_ERR_ARG, "null argument");
  if (S != tr->S)
    return fail(SPEF_ERR_ARG, "S = " + std::to_string(S) + ", the tracker has " + std::to_string(tr->S) + " streams");
  if (T < 1) return fail(SPEF_ERR_ARG, "T must be at least 1");
  if ((int64_t)T * S * 36 > 0x7fffffff) return fail(SPEF_ERR_ARG, "too many rows");
  spef_ctx* c = tr->ctx;
  Dev d(tr->device);
  hipStream_t s = (hipStream_t)stream_hip;
  const double rows = (double)T * S;
  HIP_TRY(prof_launch(c, s, "track_step_kernel",
                      rows * (2 * 28 + 8 + (cov ? 144 : 0) + (status ? 4 : 0) + (cov_out ? 144 : 0) + (rates_out ? 24 : 0)) +
                          2.0 * S * TRACK_STATE * 8,
                      rows * 2.0 * 3000.0, [&] {
    return launch_track_step(tr->prm, tr->state, quat, pos, cov, status, T, S, quat_out, pos_out, d2, cov_out,
                             rates_out, track_status, s);
  }));
  return SPEF_OK;
}

int spef_track_step_modes(spef_track* tr, const float* mode_quat, const float* mode_mass, const float* mode_cov,
                          const int* n_modes, int K, const float* pos, const float* cov, const int* status, int T,
                          int S, float* quat_out, float* pos_out, float* d2, float* cov_out, float* rates_out,
                          int* track_status, int* chosen, void* stream_hip) {
  if (!tr) return fail(SPEF_ERR_ARG, "null tracker");
  if (!mode_quat || !mode_mass || !mode_cov || !n_modes || !pos || !cov || !quat_out || !pos_out || !track_status ||
      !chosen)
    return fail(SPEF_ERR_ARG, "null argument");
  if (K < 1 || K > SPEF_MODES_MAX) return fail(SPEF_ERR_ARG, "K must be in 1.." + std::to_string(SPEF_MODES_MAX));
  if (S != tr->S)
    return fail(SPEF_ERR_ARG, "S = " + std::to_string(S) + ", the tracker has " + std::to_string(tr->S) + " streams");
  if (T < 1) return fail(SPEF_ERR_ARG, "T must be at least 1");
  if ((int64_t)T * S * 36 > 0x7fffffff) return fail(SPEF_ERR_ARG, "too many rows");
  spef_ctx* c = tr->ctx;
  Dev d(tr->device);
  hipStream_t s = (hipStream_t)stream_hip;
  const double rows = (double)T * S;
  HIP_TRY(prof_launch(c, s, "track_step_modes_kernel",
                      rows * (K * 56 + 4 + 12 + 28 + 12 + 144 + (status ? 4 : 0) + (cov_out ? 144 : 0) + (rates_out ? 24 : 0)) +
                          2.0 * S * TRACK_STATE * 8,
                      rows * (1.0 + K) * 3000.0, [&] {
    return launch_track_step_modes(tr->prm, tr->state, mode_quat, mode_mass, mode_cov, n_modes, K, pos, cov, status, T,
                                   S, quat_out, pos_out, d2, cov_out, rates_out, track_status, chosen, s);
  }));
  return SPEF_OK;
}

// ------------------------------------------------------------------------------------------ pose smoothing
struct spef_track_history {
  spef_track* track = nullptr;   // identity only: the tracker may be gone when the history is smoothed
  spef_ctx* ctx = nullptr;
  int device = 0;
  int S = 0, capacity = 0;
  int count = 0;                 // frames recorded: known to the host, every launch is sized by it
  TrackParams prm{};
  double* rows = nullptr;        // [capacity][S][TRACK_STATE]
  double* ws = nullptr;          // [capacity][S][SMOOTH_WS]: the backward pass's gains
};

int spef_track_history_destroy(spef_track_history* h) {
  if (!h) return SPEF_OK;
  Dev d(h->device);
  if (h->rows) hipFree(h->rows);
  if (h->ws) hipFree(h->ws);
  delete h;
  return SPEF_OK;
}

int spef_track_history_create(spef_track* tr, int capacity, spef_track_history** out) {
  if (!tr || !out) return fail(SPEF_ERR_ARG, "null argument");
  if (capacity < 1) return fail(SPEF_ERR_ARG, "capacity must be at least 1");
  if ((int64_t)capacity * tr->S * 36 > 0x7fffffff)   // the rows of one spef_track_smooth call, as spef_track_step
    return fail(SPEF_ERR_ARG, "too many rows: capacity * n_streams * 36 must stay below 2^31");
  Dev d(tr->device);
  spef_track_history* h = new spef_track_history;
  h->track = tr;
  h->ctx = tr->ctx;
  h->device = tr->device;
  h->S = tr->S;
  h->capacity = capacity;
  h->prm = tr->prm;
  const size_t rows = (size_t)capacity * tr->S;
  hipError_t e = hipMalloc(&h->rows, rows * TRACK_STATE * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&h->ws, rows * SMOOTH_WS * sizeof(double));
  if (e == hipSuccess) e = hipMemset(h->rows, 0, rows * TRACK_STATE * sizeof(double));
  if (e == hipSuccess) e = hipMemset(h->ws, 0, rows * SMOOTH_WS * sizeof(double));
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    spef_track_history_destroy(h);
    return fail(SPEF_ERR_HIP, std::string("spef_track_history_create: ") + hipGetErrorString(e));
  }
  *out = h;
  return SPEF_OK;
}

int spef_track_history_reset(spef_track_history* h) {
  if (!h) return fail(SPEF_ERR_ARG, "null history");
  h->count = 0;
  return SPEF_OK;
}

int spef_track_history_count(spef_track_history* h, int* count_device, void* stream_hip) {
  if (!h || !count_device) return fail(SPEF_ERR_ARG, "null argument");
  Dev d(h->device);
  HIP_TRY(launch_track_history_count(count_device, h->count, (hipStream_t)stream_hip));
  return SPEF_OK;
}

int spef_track_history_push(spef_track_history* h, spef_track* tr, const int* track_status, void* stream_hip) {
  if (!h || !tr || !track_status) return fail(SPEF_ERR_ARG, "null argument");
  if (h->track != tr || h->S != tr->S) return fail(SPEF_ERR_ARG, "the history belongs to another tracker");
  if (h->count + 1 > h->capacity) return fail(SPEF_ERR_ARG, "the history is full");
  Dev d(h->device);
  HIP_TRY(launch_track_history_push(h->rows + (int64_t)h->count * h->S * TRACK_STATE, tr->state, track_status, h->S,
                                    (hipStream_t)stream_hip));
  h->count += 1;
  return SPEF_OK;
}

int spef_track_history_get(spef_track_history* h, int first, int T, double* out_device, void* stream_hip) {
  if (!h || !out_device) return fail(SPEF_ERR_ARG, "null argument");
  if (first < 0 || T < 1 || (int64_t)first + T > h->count) return fail(SPEF_ERR_ARG, "frames out of range");
  Dev d(h->device);
  HIP_TRY(launch_track_copy(out_device, h->rows + (int64_t)first * h->S * TRACK_STATE, (int64_t)T * h->S * TRACK_STATE,
                            (hipStream_t)stream_hip));
  return SPEF_OK;
}

int spef_track_step_hist(spef_track* tr, spef_track_history* h, const float* quat, const float* pos, const float* cov,
                         const int* status, int T, int S, float* quat_out, float* pos_out, float* d2, float* cov_out,
                         float* rates_out, int* track_status, void* stream_hip) {
  if (!tr || !h) return fail(SPEF_ERR_ARG, "null tracker or history");
  if (!quat || !pos || !quat_out || !pos_out || !track_status) return fail(SPEF_ERR_ARG, "null argument");
  if (h->track != tr || h->S != tr->S) return fail(SPEF_ERR_ARG, "the history belongs to another tracker");
  if (S != tr->S)
    return fail(SPEF_ERR_ARG, "S = " + std::to_string(S) + ", the tracker has " + std::to_string(tr->S) + " streams");
  if (T < 1) return fail(SPEF_ERR_ARG, "T must be at least 1");
  if ((int64_t)T * S * 36 > 0x7fffffff) return fail(SPEF_ERR_ARG, "too many rows");
  if ((int64_t)h->count + T > h->capacity)
    return fail(SPEF_ERR_ARG, std::to_string(h->count) + " + " + std::to_string(T) + " frames exceed the history's capacity " +
                                  std::to_string(h->capacity));
  spef_ctx* c = tr->ctx;
  Dev d(tr->device);
  hipStream_t s = (hipStream_t)stream_hip;
  const double rows = (double)T * S;
  HIP_TRY(prof_launch(c, s, "track_step_hist_kernel",
                      rows * (2 * 28 + 8 + (cov ? 144 : 0) + (status ? 4 : 0) + (cov_out ? 144 : 0) + (rates_out ? 24 : 0) +
                              TRACK_STATE * 8) +
                          2.0 * S * TRACK_STATE * 8,
                      rows * 2.0 * 3000.0, [&] {
    return launch_track_step_hist(tr->prm, tr->state, h->rows + (int64_t)h->count * S * TRACK_STATE, quat, pos, cov,
                                  status, T, S, quat_out, pos_out, d2, cov_out, rates_out, track_status, s);
  }));
  h->count += T;
  return SPEF_OK;
}

int spef_track_smooth(spef_track_history* h, int first, int T, float* quat_io, float* pos_io, float* cov_out,
                      float* rates_out, int* smooth_status, void* stream_hip) {
  if (!h) return fail(SPEF_ERR_ARG, "null history");
  if (!quat_io || !pos_io || !smooth_status) return fail(SPEF_ERR_ARG, "null argument");
  if (first < 0 || T < 1 || (int64_t)first + T > h->count)
    return fail(SPEF_ERR_ARG, "frames " + std::to_string(first) + " .. " + std::to_string((int64_t)first + T - 1) +
                                  " are not all recorded (" + std::to_string(h->count) + " frames)");
  spef_ctx* c = h->ctx;
  Dev d(h->device);
  hipStream_t s = (hipStream_t)stream_hip;
  const int S = h->S;
  const double rows = (double)T * S;
  const double* x = h->rows + (int64_t)first * S * TRACK_STATE;
  double* ws = h->ws + (int64_t)first * S * SMOOTH_WS;
  const bool want_cov = cov_out != nullptr;
  HIP_TRY(prof_launch(c, s, "smooth_gain_kernel", rows * 8.0 * (TRACK_STATE + 152 + (want_cov ? 144 : 0)),
                      rows * 2.0 * 1500.0, [&] { return launch_track_smooth_gain(h->prm, x, ws, T, S, want_cov, s); }));
  HIP_TRY(prof_launch(c, s, "smooth_chain_kernel",
                      rows * (8.0 * (16 + 152 + (want_cov ? 288 : 0)) + 28 + 4 + (want_cov ? 144 : 0) + (rates_out ? 24 : 0)),
                      rows * 2.0 * (want_cov ? 3700.0 : 250.0), [&] {
    return launch_track_smooth_chain(x, ws, T, S, quat_io, pos_io, cov_out, rates_out, smooth_status, s);
  }));
  return SPEF_OK;
}

}  // extern "C"
