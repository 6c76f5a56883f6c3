// Decode side of the C ABI (include/spef.h): decode tables, the classification / regression decode and the pose
// covariance of its PDFs, the keypoint model set-up for EPnP, the consensus and the refinement behind it, and the
// Pillow-exact resize.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "spef_ctx.hpp"

// Pillow precompute_coeffs + normalize_coeffs_8bpc (libImaging/Resample.c), BILINEAR filter (support 1):
// bounds [out][2] = (xmin, count), coefficients [out][ksize] in fixed point with 22 fractional bits.
static int pil_coeffs(int in_size, int out_size, std::vector<int>& bounds, std::vector<int>& kk) {
  const double scale = (double)(float)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  const int ksize = (int)ceil(support) * 2 + 1;
  bounds.assign(2 * out_size, 0);
  kk.assign((size_t)out_size * ksize, 0);
  std::vector<double> k(ksize);
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
      double t = (x + xmin - center + 0.5) * ss;
      if (t < 0.0) t = -t;
      const double w = t < 1.0 ? 1.0 - t : 0.0;
      k[x] = w;
      ww += w;
    }
    for (int x = 0; x < xmax; ++x)
      if (ww != 0.0) k[x] /= ww;
    for (int x = 0; x < xmax; ++x)
      kk[(size_t)xx * ksize + x] = k[x] < 0 ? (int)(-0.5 + k[x] * (1 << 22)) : (int)(0.5 + k[x] * (1 << 22));
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
  }
  return ksize;
}

extern "C" {

int spef_set_decode_tables(spef_ctx* c, const double* ori_bins, int n_ori_bins, const double* pos_grid,
                           int n_pos_bins) {
  if (!c) return fail(SPEF_ERR_ARG, "null context");
  if (n_ori_bins > 8192) return fail(SPEF_ERR_ARG, "at most 8192 orientation bins");
  Dev d(c->device);
  if (c->d_ori_bins) hipFree(c->d_ori_bins);
  if (c->d_pos_grid) hipFree(c->d_pos_grid);
  c->d_ori_bins = nullptr;
  c->d_pos_grid = nullptr;
  c->n_ori_bins = c->n_pos_bins = 0;
  if (ori_bins && n_ori_bins > 0) {
    HIP_TRY(hipMalloc(&c->d_ori_bins, sizeof(double) * 4 * n_ori_bins));
    HIP_TRY(hipMemcpy(c->d_ori_bins, ori_bins, sizeof(double) * 4 * n_ori_bins, hipMemcpyHostToDevice));
    c->n_ori_bins = n_ori_bins;
  }
  if (pos_grid && n_pos_bins > 0) {
    HIP_TRY(hipMalloc(&c->d_pos_grid, sizeof(double) * 3 * n_pos_bins));
    HIP_TRY(hipMemcpy(c->d_pos_grid, pos_grid, sizeof(double) * 3 * n_pos_bins, hipMemcpyHostToDevice));
    c->n_pos_bins = n_pos_bins;
  }
  return SPEF_OK;
}

int spef_decode(spef_ctx* c, int ori_mode, int pos_mode, const float* ori_raw, int n_ori, const float* pos_raw,
                int n_pos, int B, float* ori_soft, float* quat, float* pos_soft, float* pos, int* status, void* stream) {
  if (!c) return fail(SPEF_ERR_ARG, "null context");
  if (B <= 0 || !ori_raw || !quat || !pos_raw || !pos || !status) return fail(SPEF_ERR_ARG, "null argument");
  // row widths must be the ones the decode describes (the kernels stride rows by the table sizes)
  if (ori_mode == SPEF_CLASSIFICATION && c->d_ori_bins && n_ori != c->n_ori_bins)
    return fail(SPEF_ERR_ARG, "orientation logits are " + std::to_string(n_ori) + " wide, the histogram has " +
                                  std::to_string(c->n_ori_bins) + " bins");
  if (ori_mode == SPEF_REGRESSION && n_ori != 4) return fail(SPEF_ERR_ARG, "orientation regression needs 4 outputs");
  if (pos_mode == SPEF_CLASSIFICATION && c->d_pos_grid && n_pos != c->n_pos_bins)
    return fail(SPEF_ERR_ARG, "position logits are " + std::to_string(n_pos) + " wide, the grid has " +
                                  std::to_string(c->n_pos_bins) + " bins");
  if (pos_mode == SPEF_REGRESSION && n_pos != 3) return fail(SPEF_ERR_ARG, "position regression needs 3 outputs");
  if (ori_mode != SPEF_CLASSIFICATION && ori_mode != SPEF_REGRESSION)
    return fail(SPEF_ERR_ARG, "ori_mode must be regression or classification");
  if (pos_mode != SPEF_CLASSIFICATION && pos_mode != SPEF_REGRESSION)
    return fail(SPEF_ERR_ARG, "pos_mode must be regression or classification");
  if (ori_mode == SPEF_CLASSIFICATION && !c->d_ori_bins)
    return fail(SPEF_ERR_STATE, "orientation bins not set (spef_set_decode_tables)");
  if (pos_mode == SPEF_CLASSIFICATION && !c->d_pos_grid)
    return fail(SPEF_ERR_STATE, "position grid not set (spef_set_decode_tables)");
  Dev d(c->device);
  hipStream_t s = (hipStream_t)stream;
  // the orientation kernel runs first: it writes every status word and, in position regression mode, copies the
  // raw position (no memset / copy launches); the position decode then ORs its bits in, in stream order
  const float* pos_src = (pos_mode == SPEF_REGRESSION && pos != pos_raw) ? pos_raw : nullptr;
  if (ori_mode == SPEF_CLASSIFICATION) {
    HIP_TRY(prof_launch(c, s, "decode_ori_kernel", (double)B * c->n_ori_bins * (ori_soft ? 8 : 4) + 32.0 * c->n_ori_bins,
                        (double)B * c->n_ori_bins * 30, [&] {
      return launch_decode_ori(ori_raw, B, c->n_ori_bins, c->d_ori_bins, ori_soft, quat, status, pos_src, pos, s);
    }));
  } else {
    HIP_TRY(launch_normalize_ori(ori_raw, B, quat, status, pos_src, pos, s));
  }
  if (pos_mode == SPEF_CLASSIFICATION)
    HIP_TRY(launch_decode_pos(pos_raw, B, c->n_pos_bins, c->d_pos_grid, pos_soft, pos, status, s));
  return SPEF_OK;
}

int spef_decode_cov(spef_ctx* c, int ori_mode, int pos_mode, const float* ori_pdf, int n_ori, const float* pos_pdf,
                    int n_pos, const float* quat, const float* pos, int B, const spef_cov_params* prm, float* cov,
                    float* ori_hinv, int* cov_status, void* stream) {
  if (!c) return fail(SPEF_ERR_ARG, "null context");
  if (B < 1 || !prm || !cov || !cov_status) return fail(SPEF_ERR_ARG, "null argument");
  if (ori_mode != SPEF_CLASSIFICATION && ori_mode != SPEF_REGRESSION)
    return fail(SPEF_ERR_ARG, "ori_mode must be regression or classification");
  if (pos_mode != SPEF_CLASSIFICATION && pos_mode != SPEF_REGRESSION)
    return fail(SPEF_ERR_ARG, "pos_mode must be regression or classification");
  for (int k = 0; k < 2; ++k)
    if (!(prm->fixed_var[k] >= 0.0) || !std::isfinite(prm->fixed_var[k]) || !(prm->floor_var[k] >= 0.0) ||
        !std::isfinite(prm->floor_var[k]))
      return fail(SPEF_ERR_ARG, "fixed_var and floor_var must be finite and >= 0");
  const bool oc = ori_mode == SPEF_CLASSIFICATION, pc = pos_mode == SPEF_CLASSIFICATION;
  if (oc && (!ori_pdf || !quat)) return fail(SPEF_ERR_ARG, "orientation classification needs ori_pdf and quat");
  if (pc && (!pos_pdf || !pos)) return fail(SPEF_ERR_ARG, "position classification needs pos_pdf and pos");
  if (ori_hinv && !oc) return fail(SPEF_ERR_ARG, "ori_hinv needs the orientation head in classification mode");
  if (oc && !c->d_ori_bins) return fail(SPEF_ERR_STATE, "orientation bins not set (spef_set_decode_tables)");
  if (pc && !c->d_pos_grid) return fail(SPEF_ERR_STATE, "position grid not set (spef_set_decode_tables)");
  if (oc && n_ori != c->n_ori_bins)
    return fail(SPEF_ERR_ARG, "the orientation PDF is " + std::to_string(n_ori) + " wide, the histogram has " +
                                  std::to_string(c->n_ori_bins) + " bins");
  if (pc && n_pos != c->n_pos_bins)
    return fail(SPEF_ERR_ARG, "the position PDF is " + std::to_string(n_pos) + " wide, the grid has " +
                                  std::to_string(c->n_pos_bins) + " bins");
  Dev d(c->device);
  hipStream_t s = (hipStream_t)stream;
  CovParams p;
  for (int k = 0; k < 2; ++k) {
    p.fixed_var[k] = prm->fixed_var[k];
    p.floor_var[k] = prm->floor_var[k];
  }
  const double no = oc ? c->n_ori_bins : 0, np = pc ? c->n_pos_bins : 0;
  HIP_TRY(prof_launch(c, s, "decode_cov_kernel", (double)B * (4.0 * no + 8.0 * np + 224.0) + 32.0 * no + 24.0 * np,
                      (double)B * (no * 120.0 + np * 24.0), [&] {
    return launch_decode_cov(oc, pc, ori_pdf, n_ori, c->d_ori_bins, pos_pdf, n_pos, c->d_pos_grid, quat, pos, B, p, cov,
                             ori_hinv, cov_status, s);
  }));
  return SPEF_OK;
}

int spef_decode_modes(spef_ctx* c, const float* ori_pdf, int n_ori, int B, const spef_modes_params* prm,
                      float* mode_quat, float* mode_mass, float* mode_cov, int* n_modes, int* modes_status,
                      void* stream) {
  if (!c) return fail(SPEF_ERR_ARG, "null context");
  if (B < 1 || !ori_pdf || !prm || !mode_quat || !mode_mass || !mode_cov || !n_modes || !modes_status)
    return fail(SPEF_ERR_ARG, "null argument");
  if (prm->k_max < 1 || prm->k_max > SPEF_MODES_MAX)
    return fail(SPEF_ERR_ARG, "k_max must be in 1.." + std::to_string(SPEF_MODES_MAX));
  if (prm->rounds < 0 || prm->rounds > 8) return fail(SPEF_ERR_ARG, "rounds must be in 0..8");
  if (!std::isfinite(prm->sep_deg) || !std::isfinite(prm->seed_rel) || !std::isfinite(prm->min_mass) ||
      !std::isfinite(prm->floor_var))
    return fail(SPEF_ERR_ARG, "the modes parameters must be finite");
  if (!(prm->sep_deg > 0.0 && prm->sep_deg <= 180.0)) return fail(SPEF_ERR_ARG, "sep_deg must be in (0, 180]");
  if (!(prm->seed_rel >= 0.0 && prm->seed_rel <= 1.0)) return fail(SPEF_ERR_ARG, "seed_rel must be in [0, 1]");
  if (!(prm->min_mass >= 0.0 && prm->min_mass <= 1.0 / prm->k_max))
    return fail(SPEF_ERR_ARG, "min_mass must be in [0, 1 / k_max]");
  if (!(prm->floor_var >= 0.0)) return fail(SPEF_ERR_ARG, "floor_var must be >= 0");
  if (!c->d_ori_bins) return fail(SPEF_ERR_STATE, "orientation bins not set (spef_set_decode_tables)");
  if (n_ori != c->n_ori_bins)
    return fail(SPEF_ERR_ARG, "the orientation PDF is " + std::to_string(n_ori) + " wide, the histogram has " +
                                  std::to_string(c->n_ori_bins) + " bins");
  Dev d(c->device);
  hipStream_t s = (hipStream_t)stream;
  ModesParams p;
  p.k_max = prm->k_max;
  p.rounds = prm->rounds;
  p.cos_half_sep = cos(prm->sep_deg * (M_PI / 180.0) * 0.5);
  p.seed_rel = prm->seed_rel;
  p.min_mass = prm->min_mass;
  p.floor_var = prm->floor_var;
  // passes over the row: sum p, <= k_max seedings, `rounds` + 1 moment passes, the prune's masses, the theta blocks
  const double passes = 3.0 + p.k_max + p.rounds;
  HIP_TRY(prof_launch(c, s, "decode_modes_kernel", (double)B * (4.0 * n_ori + 14.0 * 4 * p.k_max + 8.0) + 32.0 * n_ori,
                      (double)B * n_ori * (passes * 30.0 * p.k_max + 120.0), [&] {
    return launch_decode_modes(ori_pdf, n_ori, c->d_ori_bins, B, p, mode_quat, mode_mass, mode_cov, n_modes,
                               modes_status, s);
  }));
  return SPEF_OK;
}

int spef_set_keypoints(spef_ctx* c, const float* kp3d, int n, const double* K, float nu, float nv) {
  if (!c || !kp3d || !K || n < 4 || n > 16) return fail(SPEF_ERR_ARG, "bad keypoint configuration");
  // All or nothing: the model is computed and checked on the host and both device buffers are allocated and filled
  // before anything in the context changes, so a failure (a degenerate model, a failed allocation or copy) leaves the
  // previous configuration -- or none -- exactly as it was.
  // epnp.cpp choose_control_points + compute_barycentric_coordinates depend only on the 3-D model: do them
  // once here (fp64). PCA axis signs are canonical (largest-|component| positive; oracle/epnp_ref.py too).
  std::vector<double> model(12 + 4 * (size_t)n);
  {
    double pw[16][3], c0[3] = {0, 0, 0};
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < 3; ++j) {
        pw[i][j] = (double)kp3d[3 * i + j];
        c0[j] += pw[i][j] / n;
      }
    double a[3][3] = {}, v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < 3; ++j)
        for (int k = 0; k < 3; ++k) a[j][k] += (pw[i][j] - c0[j]) * (pw[i][k] - c0[k]);
    for (int sweep = 0; sweep < 50; ++sweep) {
      double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
      if (off < 1e-40) break;
      for (int p = 0; p < 2; ++p)
        for (int q = p + 1; q < 3; ++q) {
          if (fabs(a[p][q]) < 1e-300) continue;
          const double th = (a[q][q] - a[p][p]) / (2 * a[p][q]);
          const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1));
          const double cs = 1 / sqrt(t * t + 1), sn = t * cs;
          for (int k = 0; k < 3; ++k) {
            const double x = a[k][p], y = a[k][q];
            a[k][p] = cs * x - sn * y;
            a[k][q] = sn * x + cs * y;
          }
          for (int k = 0; k < 3; ++k) {
            const double x = a[p][k], y = a[q][k];
            a[p][k] = cs * x - sn * y;
            a[q][k] = sn * x + cs * y;
          }
          for (int k = 0; k < 3; ++k) {
            const double x = v[k][p], y = v[k][q];
            v[k][p] = cs * x - sn * y;
            v[k][q] = sn * x + cs * y;
          }
        }
    }
    int ord[3] = {0, 1, 2};
    for (int i = 0; i < 3; ++i)
      for (int j = i + 1; j < 3; ++j)
        if (a[ord[j]][ord[j]] > a[ord[i]][ord[i]]) std::swap(ord[i], ord[j]);
    double cws[4][3];
    for (int j = 0; j < 3; ++j) cws[0][j] = c0[j];
    for (int i = 1; i < 4; ++i) {
      const int e = ord[i - 1];
      int big = 0;
      for (int j = 1; j < 3; ++j)
        if (fabs(v[j][e]) > fabs(v[big][e])) big = j;
      const double sgn = v[big][e] >= 0 ? 1.0 : -1.0;
      const double k = sqrt(std::max(a[e][e], 0.0) / n);
      for (int j = 0; j < 3; ++j) cws[i][j] = c0[j] + k * sgn * v[j][e];
    }
    double cc[3][3];
    for (int i = 0; i < 3; ++i)
      for (int j = 1; j < 4; ++j) cc[i][j - 1] = cws[j][i] - cws[0][i];
    const double det = cc[0][0] * (cc[1][1] * cc[2][2] - cc[1][2] * cc[2][1]) -
                       cc[0][1] * (cc[1][0] * cc[2][2] - cc[1][2] * cc[2][0]) +
                       cc[0][2] * (cc[1][0] * cc[2][1] - cc[1][1] * cc[2][0]);
    if (fabs(det) < 1e-300) return fail(SPEF_ERR_ARG, "degenerate 3-D keypoint model");
    double ci[3][3];
    ci[0][0] = (cc[1][1] * cc[2][2] - cc[1][2] * cc[2][1]) / det;
    ci[0][1] = (cc[0][2] * cc[2][1] - cc[0][1] * cc[2][2]) / det;
    ci[0][2] = (cc[0][1] * cc[1][2] - cc[0][2] * cc[1][1]) / det;
    ci[1][0] = (cc[1][2] * cc[2][0] - cc[1][0] * cc[2][2]) / det;
    ci[1][1] = (cc[0][0] * cc[2][2] - cc[0][2] * cc[2][0]) / det;
    ci[1][2] = (cc[0][2] * cc[1][0] - cc[0][0] * cc[1][2]) / det;
    ci[2][0] = (cc[1][0] * cc[2][1] - cc[1][1] * cc[2][0]) / det;
    ci[2][1] = (cc[0][1] * cc[2][0] - cc[0][0] * cc[2][1]) / det;
    ci[2][2] = (cc[0][0] * cc[1][1] - cc[0][1] * cc[1][0]) / det;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 3; ++j) model[3 * i + j] = cws[i][j];
    for (int i = 0; i < n; ++i) {
      double al[3];
      for (int j = 0; j < 3; ++j)
        al[j] = ci[j][0] * (pw[i][0] - cws[0][0]) + ci[j][1] * (pw[i][1] - cws[0][1]) + ci[j][2] * (pw[i][2] - cws[0][2]);
      model[12 + 4 * i + 0] = 1.0 - al[0] - al[1] - al[2];
      model[12 + 4 * i + 1] = al[0];
      model[12 + 4 * i + 2] = al[1];
      model[12 + 4 * i + 3] = al[2];
    }
  }
  Dev d(c->device);
  float* new_kp3d = nullptr;
  double* new_model = nullptr;
  hipError_t e = hipMalloc(&new_kp3d, sizeof(float) * 3 * n);
  if (e == hipSuccess) e = hipMalloc(&new_model, sizeof(double) * model.size());
  if (e == hipSuccess) e = hipMemcpy(new_kp3d, kp3d, sizeof(float) * 3 * n, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(new_model, model.data(), sizeof(double) * model.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (new_kp3d) hipFree(new_kp3d);
    if (new_model) hipFree(new_model);
    return fail(SPEF_ERR_HIP, std::string("spef_set_keypoints: ") + hipGetErrorString(e));
  }
  if (c->kp3d) hipFree(c->kp3d);
  if (c->kp_model) hipFree(c->kp_model);
  c->kp3d = new_kp3d;
  c->kp_model = new_model;
  c->kp_n = n;
  memcpy(c->camK, K, sizeof(c->camK));
  c->cam_nu = nu;
  c->cam_nv = nv;
  return SPEF_OK;
}

int spef_set_keypoint_distortion(spef_ctx* c, const double* dist, int n) {
  if (!c) return fail(SPEF_ERR_ARG, "null context");
  if (n != 0 && n != 4 && n != 5) return fail(SPEF_ERR_ARG, "distortion: 0, 4 (k1 k2 p1 p2) or 5 (+ k3) coefficients");
  if (n && !dist) return fail(SPEF_ERR_ARG, "null distortion coefficients");
  EpnpDist d = {0, 0, 0, 0, 0, 0};
  if (n) {
    d.k1 = dist[0];
    d.k2 = dist[1];
    d.p1 = dist[2];
    d.p2 = dist[3];
    d.k3 = n == 5 ? dist[4] : 0.0;
    d.on = (d.k1 != 0 || d.k2 != 0 || d.p1 != 0 || d.p2 != 0 || d.k3 != 0) ? 1 : 0;
  }
  c->kp_dist = d;
  return SPEF_OK;
}

int spef_decode_keypoints(spef_ctx* c, const float* raw, int B, int apply_sigmoid, float* kp_out, float* quat,
                          float* pos, int* status, void* stream) {
  if (!c || !raw || !quat || !pos || !status || B <= 0) return fail(SPEF_ERR_ARG, "null argument");
  if (!c->kp3d || !c->kp_model) return fail(SPEF_ERR_STATE, "keypoints not configured (spef_set_keypoints)");
  Dev d(c->device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(status, 0, sizeof(int) * B, s));
  HIP_TRY(prof_launch(c, s, "epnp_kernel", (double)B * (2 * (c->kp_n + 1) * 8 + 28), (double)B * 1.0e5, [&] {
    return launch_epnp(raw, B, c->kp_n, c->kp3d, c->kp_model, c->camK, c->cam_nu, c->cam_nv, c->kp_dist, apply_sigmoid, kp_out,
                       quat, pos, status, s);
  }));
  return SPEF_OK;
}

int spef_refine_keypoints(spef_ctx* c, const float* kp, const float* weights, int B, int max_iters, float huber_px,
                          float* quat_inout, float* pos_inout, float* fit, float* cov, int* iters, int* status,
                          void* stream) {
  if (!c || !kp || !quat_inout || !pos_inout || !status || B <= 0) return fail(SPEF_ERR_ARG, "null argument");
  if (max_iters < 1 || max_iters > 100) return fail(SPEF_ERR_ARG, "max_iters must be in 1..100");
  if (!(huber_px >= 0.0f) || !std::isfinite(huber_px)) return fail(SPEF_ERR_ARG, "huber_px must be finite and >= 0");
  if (!c->kp3d || !c->kp_model) return fail(SPEF_ERR_STATE, "keypoints not configured (spef_set_keypoints)");
  Dev d(c->device);
  hipStream_t s = (hipStream_t)stream;
  const int n = c->kp_n;
  HIP_TRY(prof_launch(c, s, "refine_kernel", (double)B * ((2 * (n + 1) + (weights ? n : 0)) * 4 + 2 * 28 + 8 +
                                                          (fit ? 16 : 0) + (cov ? 144 : 0) + (iters ? 4 : 0)),
                      (double)B * 8.0 * n * 180.0, [&] {
    return launch_refine(kp, weights, B, n, c->kp3d, c->camK, c->cam_nu, c->cam_nv, c->kp_dist, max_iters, huber_px,
                         quat_inout, pos_inout, fit, cov, iters, status, s);
  }));
  return SPEF_OK;
}

int spef_consensus_keypoints_f64(spef_ctx* c, const float* kp, const float* weights, int B, float inlier_px,
                                 int min_inliers, float* quat_inout, float* pos_inout, float* weights_out, int* info,
                                 float* cost, double* pose64, int* status, void* stream) {
  if (!c || !kp || !quat_inout || !pos_inout || !weights_out || !status || B < 1)
    return fail(SPEF_ERR_ARG, "null argument");
  if (!(inlier_px > 0.0f) || !std::isfinite(inlier_px)) return fail(SPEF_ERR_ARG, "inlier_px must be finite and > 0");
  if (!c->kp3d || !c->kp_model) return fail(SPEF_ERR_STATE, "keypoints not configured (spef_set_keypoints)");
  const int n = c->kp_n;
  if (min_inliers < 4 || min_inliers > n)
    return fail(SPEF_ERR_ARG, "min_inliers must be in 4.." + std::to_string(n));
  Dev d(c->device);
  hipStream_t s = (hipStream_t)stream;
  const double triples = n * (n - 1) * (n - 2) / 6.0;
  HIP_TRY(prof_launch(c, s, "consensus_kernel", (double)B * ((2 * (n + 1) + (weights ? n : 0) + n) * 4 + 2 * 28 + 8 +
                                                             (info ? 16 : 0) + (cost ? 4 : 0) + (pose64 ? 96 : 0)),
                      (double)B * triples * (600.0 + 2.0 * (120.0 + 40.0 * n)), [&] {
    return launch_consensus(kp, weights, B, n, c->kp3d, c->camK, c->cam_nu, c->cam_nv, c->kp_dist, inlier_px,
                            min_inliers, quat_inout, pos_inout, weights_out, info, cost, pose64, status, s);
  }));
  return SPEF_OK;
}

int spef_consensus_keypoints(spef_ctx* c, const float* kp, const float* weights, int B, float inlier_px,
                             int min_inliers, float* quat_inout, float* pos_inout, float* weights_out, int* info,
                             float* cost, int* status, void* stream) {
  return spef_consensus_keypoints_f64(c, kp, weights, B, inlier_px, min_inliers, quat_inout, pos_inout, weights_out,
                                      info, cost, nullptr, status, stream);
}

int spef_preprocess(spef_ctx* c, const uint8_t* frames, int B, int Hin, int Win, uint8_t* out, int H, int W,
                    void* stream) {
  if (!c || !frames || !out) return fail(SPEF_ERR_ARG, "null argument");
  if (B <= 0 || Hin <= 0 || Win <= 0 || H <= 0 || W <= 0) return fail(SPEF_ERR_ARG, "bad preprocess shape");
  Dev d(c->device);
  hipStream_t s = (hipStream_t)stream;
  const int key[4] = {Hin, Win, H, W};
  if (memcmp(key, c->pre_key, sizeof(key)) != 0) {
    std::vector<int> bh, kh, bv, kv;
    c->pre_ksh = pil_coeffs(Win, W, bh, kh);
    c->pre_ksv = pil_coeffs(Hin, H, bv, kv);
    c->pre_y0 = bv[0];
    c->pre_ht = bv[2 * H - 2] + bv[2 * H - 1] - c->pre_y0;
    for (int i = 0; i < H; ++i) bv[2 * i] -= c->pre_y0;   // vertical bounds relative to the temp image
    std::vector<int> th(bh), tv(bv);
    th.insert(th.end(), kh.begin(), kh.end());
    tv.insert(tv.end(), kv.begin(), kv.end());
    if (c->pre_bh) hipFree(c->pre_bh);
    if (c->pre_bv) hipFree(c->pre_bv);
    c->pre_bh = c->pre_bv = nullptr;
    memset(c->pre_key, 0, sizeof(c->pre_key));
    HIP_TRY(hipMalloc(&c->pre_bh, th.size() * sizeof(int)));
    HIP_TRY(hipMalloc(&c->pre_bv, tv.size() * sizeof(int)));
    HIP_TRY(hipMemcpy(c->pre_bh, th.data(), th.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->pre_bv, tv.data(), tv.size() * sizeof(int), hipMemcpyHostToDevice));
    memcpy(c->pre_key, key, sizeof(key));
  }
  const size_t tmp = (size_t)B * c->pre_ht * W * 3;
  if (tmp > c->pre_tmp_bytes) {
    if (c->pre_tmp) hipFree(c->pre_tmp);
    c->pre_tmp = nullptr;
    c->pre_tmp_bytes = 0;
    HIP_TRY(hipMalloc(&c->pre_tmp, tmp));
    c->pre_tmp_bytes = tmp;
  }
  HIP_TRY(prof_launch(c, s, "resize_h_kernel", (double)B * c->pre_ht * Win * 3 + (double)tmp, 0.0, [&] {
    return launch_resize_h(frames, c->pre_tmp, c->pre_bh, c->pre_bh + 2 * W, c->pre_ksh, B, Hin, Win, c->pre_y0,
                           c->pre_ht, W, s);
  }));
  HIP_TRY(prof_launch(c, s, "resize_v_kernel", (double)tmp + (double)B * H * W * 3, 0.0, [&] {
    return launch_resize_v(c->pre_tmp, out, c->pre_bv, c->pre_bv + 2 * H, c->pre_ksv, B, c->pre_ht, H, W, s);
  }));
  return SPEF_OK;
}

}  // extern "C"
