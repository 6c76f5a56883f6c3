// Region-of-interest side of the C ABI (include/spef.h): the tracker's one-frame-ahead prediction, the box of a pose,
// the crop-and-resize with one box per frame and the un-mapping of the keypoints a crop gave (k_roi.hip).
#include <math.h>
#include <string.h>

#include <algorithm>

#include "spef_ctx.hpp"

// Pillow's ksize for the BILINEAR filter (precompute_coeffs; pil_coeffs in api_decode.cpp): no box of a frame has more.
static int pil_ksize(int in_size, int out_size) {
  const double scale = (double)(float)in_size / out_size;
  return (int)ceil(scale < 1.0 ? 1.0 : scale) * 2 + 1;
}

// The most source rows a tile of th output rows can need, over every box of the frame: for rows ya <= yb of one tile,
// (ymin + count)(yb) - ymin(ya) <= (center(yb) + support + 0.5) - (center(ya) - support + 0.5 - 1)
// = (yb - ya) scale + 2 support + 1, and a box's scale is at most the frame's.
static int roi_rows_cap(int in_size, int out_size, int th) {
  const double scale = (double)(float)in_size / out_size;
  const double support = scale < 1.0 ? 1.0 : scale;
  return (int)ceil((th - 1) * scale + 2.0 * support) + 2;
}

extern "C" {

int spef_track_predict(spef_track* tr, int first_stream, int n, float* quat_out, float* pos_out, int* have_out,
                       void* stream_hip) {
  if (!tr) return fail(SPEF_ERR_ARG, "null tracker");
  if (!quat_out || !pos_out || !have_out) return fail(SPEF_ERR_ARG, "null argument");
  if (first_stream < 0 || n < 1 || (int64_t)first_stream + n > tr->S)
    return fail(SPEF_ERR_ARG, "stream index out of range");
  Dev d(tr->device);
  hipStream_t s = (hipStream_t)stream_hip;
  HIP_TRY(prof_launch(tr->ctx, s, "track_predict_kernel", (double)n * (17 * 8 + 32), (double)n * 100.0, [&] {
    return launch_track_predict(tr->state + (size_t)first_stream * TRACK_STATE, n, quat_out, pos_out, have_out, s);
  }));
  return SPEF_OK;
}

int spef_roi_boxes(spef_ctx* c, const float* quat, const float* pos, const int* have, int B, int Hin, int Win, int H,
                   int W, double margin, double min_side, int* box_out, int* status, void* stream) {
  if (!c || !quat || !pos || !box_out || !status) return fail(SPEF_ERR_ARG, "null argument");
  if (B <= 0 || Hin <= 0 || Win <= 0 || H <= 0 || W <= 0) return fail(SPEF_ERR_ARG, "bad ROI shape");
  if (!(margin >= 0.0) || !std::isfinite(margin)) return fail(SPEF_ERR_ARG, "margin must be finite and >= 0");
  if (!(min_side >= 1.0) || !std::isfinite(min_side)) return fail(SPEF_ERR_ARG, "min_side must be finite and >= 1");
  if (!c->kp3d || !c->kp_model) return fail(SPEF_ERR_STATE, "keypoints not configured (spef_set_keypoints)");
  Dev d(c->device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(prof_launch(c, s, "roi_box_kernel", (double)B * (28 + (have ? 4 : 0) + 20), (double)B * 40.0 * (c->kp_n + 1),
                      [&] {
    return launch_roi_boxes(quat, pos, have, B, c->kp_n, c->kp3d, c->camK, c->kp_dist, Hin, Win, H, W, margin, min_side,
                            box_out, status, s);
  }));
  return SPEF_OK;
}

int spef_preprocess_roi(spef_ctx* c, const uint8_t* frames, const int* box, int B, int Hin, int Win, uint8_t* out,
                        int H, int W, int* status, void* stream) {
  if (!c || !frames || !box || !out) return fail(SPEF_ERR_ARG, "null argument");
  if (B <= 0 || B > 65535 || Hin <= 0 || Win <= 0 || H <= 0 || W <= 0) return fail(SPEF_ERR_ARG, "bad preprocess shape");
  if ((int64_t)Hin * Win * 3 > 0x7fffffff) return fail(SPEF_ERR_ARG, "frame too large");
  Dev d(c->device);
  hipStream_t s = (hipStream_t)stream;
  const int key[4] = {Hin, Win, H, W};
  const bool new_key = memcmp(key, c->roi_key, sizeof(key)) != 0;
  if (new_key) {
    // tile shape: the largest of 16 x 64 output pixels and its halvings (rows first) whose LDS stays under a quarter
    // of the CU's 160 KiB -- the coefficient rows of the tile and the 8-bit rows between the passes
    const int ksh = (pil_ksize(Win, W) + 3) & ~3, ksv = (pil_ksize(Hin, H) + 3) & ~3;
    int th = 16, tw = 64;
    const size_t budget = 40 * 1024;
    while (roi_resample_lds_bytes(ksh, ksv, th, tw, roi_rows_cap(Hin, H, th)) > budget && (th > 1 || tw > 1)) {
      if (th > 1)
        th /= 2;
      else
        tw /= 2;
    }
    if (roi_resample_lds_bytes(ksh, ksv, th, tw, roi_rows_cap(Hin, H, th)) > budget || (H + th - 1) / th > 65535)
      return fail(SPEF_ERR_ARG, "the resize ratio is too large for spef_preprocess_roi");
    c->roi_kstr_h = ksh;
    c->roi_kstr_v = ksv;
    c->roi_th = th;
    c->roi_tw = tw;
    c->roi_rows_cap = roi_rows_cap(Hin, H, th);
  }
  if (new_key || B > c->roi_B) {   // grown like spef_preprocess' temporary
    if (c->roi_tab_h) hipFree(c->roi_tab_h);
    if (c->roi_tab_v) hipFree(c->roi_tab_v);
    if (c->roi_valid) hipFree(c->roi_valid);
    c->roi_tab_h = c->roi_tab_v = c->roi_valid = nullptr;
    c->roi_B = 0;
    memset(c->roi_key, 0, sizeof(c->roi_key));
    HIP_TRY(hipMalloc(&c->roi_tab_h, sizeof(int) * (size_t)B * W * (2 + c->roi_kstr_h)));
    HIP_TRY(hipMalloc(&c->roi_tab_v, sizeof(int) * (size_t)B * H * (2 + c->roi_kstr_v)));
    HIP_TRY(hipMalloc(&c->roi_valid, sizeof(int) * (size_t)B));
    c->roi_B = B;
    memcpy(c->roi_key, key, sizeof(key));
  }
  const double tab_bytes = 4.0 * B * ((double)W * (2 + c->roi_kstr_h) + (double)H * (2 + c->roi_kstr_v));
  HIP_TRY(prof_launch(c, s, "roi_coeffs_kernel", tab_bytes + 16.0 * B, (double)B * (W + H) * 40.0, [&] {
    return launch_roi_coeffs(box, B, Hin, Win, H, W, c->roi_kstr_h, c->roi_kstr_v, c->roi_tab_h, c->roi_tab_v,
                             c->roi_valid, status, s);
  }));
  // algorithmic bytes: the full frames (an upper bound: the boxes are on the device), the tables and the output
  HIP_TRY(prof_launch(c, s, "roi_resample_kernel", (double)B * Hin * Win * 3 + tab_bytes + (double)B * H * W * 3, 0.0,
                      [&] {
    return launch_roi_resample(frames, out, c->roi_tab_h, c->roi_tab_v, c->roi_valid, B, Hin, Win, H, W, c->roi_kstr_h,
                               c->roi_kstr_v, c->roi_th, c->roi_tw, c->roi_rows_cap, s);
  }));
  return SPEF_OK;
}

int spef_roi_unmap_keypoints(spef_ctx* c, const float* raw, const int* box, int B, int apply_sigmoid, float* kp_out,
                             void* stream) {
  if (!c || !raw || !box || !kp_out || B <= 0) return fail(SPEF_ERR_ARG, "null argument");
  if (!c->kp3d || !c->kp_model) return fail(SPEF_ERR_STATE, "keypoints not configured (spef_set_keypoints)");
  Dev d(c->device);
  hipStream_t s = (hipStream_t)stream;
  const int nk = 2 * (c->kp_n + 1);
  HIP_TRY(prof_launch(c, s, "roi_unmap_kernel", (double)B * (8.0 * nk + 16), (double)B * nk * 12.0, [&] {
    return launch_roi_unmap(raw, box, B, nk, c->cam_nu, c->cam_nv, apply_sigmoid, kp_out, s);
  }));
  return SPEF_OK;
}

}  // extern "C"
