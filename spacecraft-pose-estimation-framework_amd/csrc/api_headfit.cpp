// The head-fit handle (include/spef.h, spef_headfit_*): the URSONet head's two Linear layers trained on the device over
// cached backbone features. The kernels are in k_headfit.hip; the forward is k_head.hip's launch_fc.
#include <cmath>

#include "spef_ctx.hpp"

struct spef_headfit {
  int device = 0;
  HeadFitShape d{};
  HeadFitOpt opt{};
  int pos_reg = 0, norm_distance = 0;
  double beta = 1.0, dropout_p = 0.0;
  uint32_t seed = 0, drop_thr = 0;
  float inv_keep = 1.0f;
  float *W = nullptr, *bias = nullptr;          // [Np][K], [Np]
  float *S1 = nullptr, *S2 = nullptr;           // optimizer state of W
  float *bS1 = nullptr, *bS2 = nullptr;         // optimizer state of bias
  float* G = nullptr;                           // [Bmax][Np]
  float* Xd = nullptr;                          // [Bmax][K] dropout copy of X
  float *Zo = nullptr, *Zp = nullptr;           // logits [Bmax][n_ori], [Bmax][n_pos]
  float* spill = nullptr;                       // [Bmax][15]: the orientation rows the position launch recomputes
  double *rowloss = nullptr, *rowaux = nullptr; // [2][Bmax], [Bmax]
  uint32_t* counter = nullptr;                  // [2]: steps completed, index of the step in flight
  float* sc = nullptr;                          // [2]: Adam's bias corrections of the step in flight
  size_t n() const { return (size_t)d.n_ori + d.n_pos; }
};

namespace {

template <typename T>
hipError_t zalloc(T** p, size_t count) {
  hipError_t e = hipMalloc(p, count * sizeof(T));
  if (e == hipSuccess) e = hipMemset(*p, 0, count * sizeof(T));
  return e;
}

const OpDesc* fc_op(const spef_ctx* c) {
  for (const OpDesc& op : c->ops)
    if (op.kind == OP_FC) return &op;
  return nullptr;
}

// the context's FC op when the trainer's sizes are the blob's
int model_head(spef_headfit* t, spef_ctx* c, const OpDesc** op) {
  if (!t || !c) return fail(SPEF_ERR_ARG, "null trainer or context");
  if (c->device != t->device) return fail(SPEF_ERR_ARG, "the trainer belongs to another device");
  if (!c->loaded) return fail(SPEF_ERR_STATE, "weights not loaded (spef_load_weights)");
  *op = fc_op(c);
  if (c->hdr.head != HEAD_URSONET || c->hdr.dtype == DT_I8 || !*op)
    return fail(SPEF_ERR_STATE, "the head fit needs a URSONet blob with a float head");
  if ((int)c->hdr.feat_c != t->d.K || (int)c->hdr.n_out0 != t->d.n_ori || (int)c->hdr.n_out1 != t->d.n_pos)
    return fail(SPEF_ERR_ARG, "trainer sizes (K " + std::to_string(t->d.K) + ", " + std::to_string(t->d.n_ori) + " + " +
                                  std::to_string(t->d.n_pos) + ") differ from the model's (" +
                                  std::to_string(c->hdr.feat_c) + ", " + std::to_string(c->hdr.n_out0) + " + " +
                                  std::to_string(c->hdr.n_out1) + ")");
  return SPEF_OK;
}

}  // namespace

extern "C" {

int spef_encode_targets(spef_ctx* c, const double* quat, const double* pos, int B, const spef_encode_params* p,
                        const uint8_t* mask, float* ori_soft, float* pos_soft, int* enc_status, void* stream) {
  if (!c || !p || !enc_status) return fail(SPEF_ERR_ARG, "null argument");
  if (B < 1) return fail(SPEF_ERR_ARG, "B must be at least 1");
  if (!ori_soft && !pos_soft) return fail(SPEF_ERR_ARG, "no output requested");
  if ((ori_soft && !quat) || (pos_soft && !pos)) return fail(SPEF_ERR_ARG, "null pose of a requested head");
  if ((ori_soft && !(std::isfinite(p->ori_var) && p->ori_var > 0.0)) ||
      (pos_soft && !(std::isfinite(p->pos_var) && p->pos_var > 0.0)))
    return fail(SPEF_ERR_ARG, "a variance is not positive and finite");
  if ((ori_soft && !c->d_ori_bins) || (pos_soft && !c->d_pos_grid))
    return fail(SPEF_ERR_STATE, "decode table not set (spef_set_decode_tables)");
  Dev dv(c->device);
  hipStream_t s = (hipStream_t)stream;
  const double px = (double)B * ((ori_soft ? c->n_ori_bins : 0) + (pos_soft ? c->n_pos_bins : 0));
  HIP_TRY(prof_launch(c, s, "encode_targets_kernel", px * 4 + 32.0 * c->n_ori_bins + 24.0 * c->n_pos_bins, px * 40, [&] {
    return launch_encode_targets(quat, pos, B, c->d_ori_bins, c->n_ori_bins, c->d_pos_grid, c->n_pos_bins, p->ori_var,
                                 p->pos_var, mask, ori_soft, pos_soft, enc_status, s);
  }));
  return SPEF_OK;
}

int spef_headfit_destroy(spef_headfit* t) {
  if (!t) return SPEF_OK;
  Dev d(t->device);
  void* all[] = {t->W, t->bias, t->S1, t->S2, t->bS1, t->bS2, t->G, t->Xd, t->Zo, t->Zp, t->spill,
                 t->rowloss, t->rowaux, t->counter, t->sc};
  for (void* p : all)
    if (p) (void)hipFree(p);
  delete t;
  return SPEF_OK;
}

int spef_headfit_create(spef_ctx* c, int K, int n_ori, int n_pos, const spef_headfit_params* p, spef_headfit** out) {
  if (!c || !p || !out) return fail(SPEF_ERR_ARG, "null argument");
  if (K < 16 || K % 16) return fail(SPEF_ERR_ARG, "K must be a positive multiple of 16");
  if (n_ori < 1 || n_pos < 1 || (int64_t)n_ori + n_pos > (1 << 24)) return fail(SPEF_ERR_ARG, "bad head widths");
  if (p->ori_mode != SPEF_CLASSIFICATION)
    return fail(SPEF_ERR_ARG, "the head fit trains the orientation branch in classification mode only");
  if (p->pos_mode != SPEF_CLASSIFICATION && p->pos_mode != SPEF_REGRESSION) return fail(SPEF_ERR_ARG, "bad pos_mode");
  if (p->pos_mode == SPEF_REGRESSION && n_pos != 3) return fail(SPEF_ERR_ARG, "position regression has 3 outputs");
  if (p->optimizer != SPEF_HEADFIT_SGD && p->optimizer != SPEF_HEADFIT_ADAM) return fail(SPEF_ERR_ARG, "bad optimizer");
  if (p->Bmax < 1 || (int64_t)p->Bmax * K > 0x7fffffff) return fail(SPEF_ERR_ARG, "bad Bmax");
  const double v[] = {p->beta, p->momentum, p->beta1, p->beta2, p->eps, p->weight_decay, p->dropout_p};
  for (double x : v)
    if (!std::isfinite(x) || x < 0.0) return fail(SPEF_ERR_ARG, "a parameter is negative or not finite");
  if (p->dropout_p >= 1.0) return fail(SPEF_ERR_ARG, "dropout_p must be below 1");
  if (p->optimizer == SPEF_HEADFIT_ADAM && (p->beta1 >= 1.0 || p->beta2 >= 1.0))
    return fail(SPEF_ERR_ARG, "Adam's betas must be below 1");
  Dev dv(c->device);
  spef_headfit* t = new spef_headfit;
  t->device = c->device;
  t->d = HeadFitShape{K, n_ori, n_pos, (n_ori + n_pos + 15) & ~15, p->Bmax};
  t->opt = HeadFitOpt{p->optimizer == SPEF_HEADFIT_ADAM ? HF_ADAM : HF_SGD, p->momentum, p->beta1, p->beta2, p->eps,
                      p->weight_decay};
  t->pos_reg = p->pos_mode == SPEF_REGRESSION;
  t->norm_distance = p->norm_distance != 0;
  t->beta = p->beta;
  t->dropout_p = p->dropout_p;
  t->seed = p->seed;
  // an element is dropped when its hash is below floor(p * 2^32); the kept ones are scaled by float32(1 / (1 - p))
  t->drop_thr = (uint32_t)floor(p->dropout_p * 4294967296.0);
  t->inv_keep = (float)(1.0 / (1.0 - p->dropout_p));
  const size_t Np = (size_t)t->d.Np, Bm = (size_t)p->Bmax;
  hipError_t e = zalloc(&t->W, Np * K);
  if (e == hipSuccess) e = zalloc(&t->bias, Np);
  if (e == hipSuccess) e = zalloc(&t->S1, Np * K);
  if (e == hipSuccess) e = zalloc(&t->bS1, Np);
  if (e == hipSuccess && t->opt.kind == HF_ADAM) e = zalloc(&t->S2, Np * K);
  if (e == hipSuccess && t->opt.kind == HF_ADAM) e = zalloc(&t->bS2, Np);
  if (e == hipSuccess) e = zalloc(&t->G, Bm * Np);
  if (e == hipSuccess && t->drop_thr) e = zalloc(&t->Xd, Bm * K);
  if (e == hipSuccess) e = zalloc(&t->Zo, Bm * n_ori);
  if (e == hipSuccess) e = zalloc(&t->Zp, Bm * n_pos);
  if (e == hipSuccess) e = zalloc(&t->spill, Bm * 15);
  if (e == hipSuccess) e = zalloc(&t->rowloss, 2 * Bm);
  if (e == hipSuccess) e = zalloc(&t->rowaux, Bm);
  if (e == hipSuccess) e = zalloc(&t->counter, 2);
  if (e == hipSuccess) e = zalloc(&t->sc, 2);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    spef_headfit_destroy(t);
    return fail(SPEF_ERR_HIP, std::string("spef_headfit_create: ") + hipGetErrorString(e));
  }
  *out = t;
  return SPEF_OK;
}

int spef_headfit_step(spef_headfit* t, const float* X, const float* To, const float* Tp, int B, const float* lr,
                      int train, float* loss_out, float* logits_out, float* grad_out, void* stream) {
  if (!t) return fail(SPEF_ERR_ARG, "null trainer");
  if (!X || !To || !Tp) return fail(SPEF_ERR_ARG, "null argument");
  if (B < 1 || B > t->d.Bmax)
    return fail(SPEF_ERR_ARG, "B = " + std::to_string(B) + ", the trainer takes 1.." + std::to_string(t->d.Bmax));
  if (train && !lr) return fail(SPEF_ERR_ARG, "a training step needs lr (a device pointer)");
  if (!train && grad_out) return fail(SPEF_ERR_ARG, "an evaluation (train = 0) writes no gradient");
  Dev dv(t->device);
  hipStream_t s = (hipStream_t)stream;
  const HeadFitShape& d = t->d;
  const bool drop = train && t->drop_thr;
  const float* Xo = X;
  if (drop) {
    HIP_TRY(launch_headfit_dropout(X, t->Xd, B, d.K, t->seed, t->drop_thr, t->inv_keep, t->counter, s));
    Xo = t->Xd;
    // the orientation rows read Xd, the position rows X: two launches of the same 16-row tiles. The tile that holds the
    // boundary runs in both; the second writes its orientation rows to a spill buffer.
    const int r0 = d.n_ori & ~15;
    HIP_TRY(launch_fc(Xo, t->W, t->bias, t->Zo, d.n_ori, nullptr, 0, B, d.K, s));
    HIP_TRY(launch_fc(X, t->W + (size_t)r0 * d.K, t->bias + r0, t->spill, d.n_ori - r0, t->Zp, d.n_pos, B, d.K, s));
  } else {
    HIP_TRY(launch_fc(X, t->W, t->bias, t->Zo, d.n_ori, t->Zp, d.n_pos, B, d.K, s));
  }
  const float so = (float)t->beta / (float)B, sp = 1.0f / (float)B;
  HIP_TRY(launch_headfit_loss(d, t->Zo, To, t->Zp, Tp, B, t->pos_reg, so, sp, t->G, t->rowloss, t->rowaux, logits_out, s));
  HIP_TRY(launch_headfit_finish(d, t->rowloss, t->rowaux, B, t->pos_reg, t->norm_distance, t->beta, t->Zp, Tp, t->G,
                                train, t->opt.beta1, t->opt.beta2, t->counter, t->sc, loss_out, s));
  if (train)
    HIP_TRY(launch_headfit_update(d, t->opt, t->G, Xo, X, B, t->W, t->S1, t->S2, t->bias, t->bS1, t->bS2, grad_out, lr,
                                  t->sc, s));
  return SPEF_OK;
}

int spef_headfit_set_weights(spef_headfit* t, const float* W, const float* bias, void* stream) {
  if (!t || !W || !bias) return fail(SPEF_ERR_ARG, "null argument");
  Dev dv(t->device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemcpyAsync(t->W, W, t->n() * t->d.K * sizeof(float), hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(t->bias, bias, t->n() * sizeof(float), hipMemcpyDeviceToDevice, s));
  return SPEF_OK;
}

int spef_headfit_get_weights(spef_headfit* t, float* W, float* bias, void* stream) {
  if (!t || !W || !bias) return fail(SPEF_ERR_ARG, "null argument");
  Dev dv(t->device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemcpyAsync(W, t->W, t->n() * t->d.K * sizeof(float), hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(bias, t->bias, t->n() * sizeof(float), hipMemcpyDeviceToDevice, s));
  return SPEF_OK;
}

int spef_headfit_get_state(spef_headfit* t, float* W_s1, float* bias_s1, float* W_s2, float* bias_s2, void* stream) {
  if (!t) return fail(SPEF_ERR_ARG, "null trainer");
  if ((W_s2 || bias_s2) && t->opt.kind != HF_ADAM) return fail(SPEF_ERR_ARG, "SGD keeps one state tensor");
  Dev dv(t->device);
  hipStream_t s = (hipStream_t)stream;
  const size_t nw = t->n() * t->d.K * sizeof(float), nb = t->n() * sizeof(float);
  if (W_s1) HIP_TRY(hipMemcpyAsync(W_s1, t->S1, nw, hipMemcpyDeviceToDevice, s));
  if (bias_s1) HIP_TRY(hipMemcpyAsync(bias_s1, t->bS1, nb, hipMemcpyDeviceToDevice, s));
  if (W_s2) HIP_TRY(hipMemcpyAsync(W_s2, t->S2, nw, hipMemcpyDeviceToDevice, s));
  if (bias_s2) HIP_TRY(hipMemcpyAsync(bias_s2, t->bS2, nb, hipMemcpyDeviceToDevice, s));
  return SPEF_OK;
}

int spef_headfit_get_g(spef_headfit* t, int B, float* G, void* stream) {
  if (!t || !G) return fail(SPEF_ERR_ARG, "null argument");
  if (B < 1 || B > t->d.Bmax) return fail(SPEF_ERR_ARG, "B out of range");
  Dev dv(t->device);
  const size_t w = t->n() * sizeof(float);
  HIP_TRY(hipMemcpy2DAsync(G, w, t->G, (size_t)t->d.Np * sizeof(float), w, (size_t)B, hipMemcpyDeviceToDevice,
                           (hipStream_t)stream));
  return SPEF_OK;
}

int spef_headfit_get_raw(spef_headfit* t, int which, float* out, void* stream) {
  if (!t || !out) return fail(SPEF_ERR_ARG, "null argument");
  const size_t Np = (size_t)t->d.Np, K = (size_t)t->d.K;
  const float* src[] = {t->W, t->bias, t->S1, t->bS1, t->S2, t->bS2, t->Xd};
  const size_t count[] = {Np * K, Np, Np * K, Np, Np * K, Np, (size_t)t->d.Bmax * K};
  if (which < 0 || which > SPEF_HEADFIT_RAW_XD) return fail(SPEF_ERR_ARG, "unknown tensor");
  if (!src[which]) return fail(SPEF_ERR_ARG, "the trainer has no such tensor (SGD keeps one state, dropout is off)");
  Dev dv(t->device);
  HIP_TRY(hipMemcpyAsync(out, src[which], count[which] * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return SPEF_OK;
}

int spef_headfit_reset_state(spef_headfit* t, void* stream) {
  if (!t) return fail(SPEF_ERR_ARG, "null trainer");
  Dev dv(t->device);
  hipStream_t s = (hipStream_t)stream;
  const size_t nw = (size_t)t->d.Np * t->d.K * sizeof(float), nb = (size_t)t->d.Np * sizeof(float);
  HIP_TRY(hipMemsetAsync(t->S1, 0, nw, s));
  HIP_TRY(hipMemsetAsync(t->bS1, 0, nb, s));
  if (t->S2) HIP_TRY(hipMemsetAsync(t->S2, 0, nw, s));
  if (t->bS2) HIP_TRY(hipMemsetAsync(t->bS2, 0, nb, s));
  HIP_TRY(hipMemsetAsync(t->counter, 0, 2 * sizeof(uint32_t), s));
  return SPEF_OK;
}

int spef_headfit_load_model(spef_headfit* t, spef_ctx* c, void* stream) {
  const OpDesc* op = nullptr;
  int rc = model_head(t, c, &op);
  if (rc) return rc;
  Dev dv(t->device);
  hipStream_t s = (hipStream_t)stream;
  const size_t Np = (size_t)t->d.Np;
  HIP_TRY(hipMemcpyAsync(t->W, ptr<float>(c, op->w0), Np * t->d.K * sizeof(float), hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(t->bias, ptr<float>(c, op->b0), Np * sizeof(float), hipMemcpyDeviceToDevice, s));
  return SPEF_OK;
}

int spef_headfit_commit(spef_headfit* t, spef_ctx* c, void* stream) {
  const OpDesc* op = nullptr;
  int rc = model_head(t, c, &op);
  if (rc) return rc;
  Dev dv(t->device);
  hipStream_t s = (hipStream_t)stream;
  const size_t Np = (size_t)t->d.Np;
  HIP_TRY(hipMemcpyAsync(c->d_data + op->w0, t->W, Np * t->d.K * sizeof(float), hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->d_data + op->b0, t->bias, Np * sizeof(float), hipMemcpyDeviceToDevice, s));
  return SPEF_OK;
}

}  // extern "C"
