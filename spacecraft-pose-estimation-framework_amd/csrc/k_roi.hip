// Track-guided region of interest for keypoint mode (ROI path; spef_amd/spe/roi.py is the NumPy
// twin of the prediction, the box rule and the un-mapping and states every step):
//   track_predict_kernel  the tracker's one-frame-ahead pose, q+ = exp([w]x) q, t+ = t + v, read from its state
//   roi_box_kernel        the box of a pose: project the origin and the model points, grow, raise to a minimum side,
//                         fit the aspect of the network input, round, shift into the frame -- or the full frame
//   roi_coeffs_kernel     Pillow's precompute_coeffs + normalize_coeffs_8bpc per frame and axis, for that frame's box
//   roi_resample_kernel   Image.crop(box).resize((W, H), BILINEAR), bit-exactly, both passes in one kernel
//   roi_unmap_kernel      sigmoid + the affine map from crop coordinates back to normalised full-frame keypoints
//
// The resample kernel: one workgroup per (frame, tile of TH x TW output pixels). The horizontal pass reads the source
// rows the tile's vertical pass needs straight from the frame and writes them, rounded to 8 bits exactly as Pillow's
// temporary image is, into an LDS tile [rows][TW][3]; the vertical pass reads that tile, four bytes (one dword) of a
// row at a time. There is no HBM temporary (its size would differ per frame). The tile's coefficient rows are staged in
// LDS first, padded to an odd dword stride (conflict-free on the 32 ds_write / ds_read_b32 banks of a half-wave).
// Source bytes are read as aligned dwords: four 3-byte pixels are 12 bytes, which four aligned dwords cover at any byte
// offset; v_alignbyte_b32 shifts them into three dwords whose twelve bytes are extracted at fixed positions.
// A dword that holds no byte of the frames is never read (the address is clamped to the last dword that does; the
// coefficients of such pixels are zero), so no load leaves the allocation: an aligned dword holding a valid byte lies
// in that byte's page.
#include <math.h>

#include "spef_common.hpp"
#include "spef_kernels.hpp"
#include "spef_track_math.hpp"

namespace spef {

// Everything below is exact arithmetic by contract with the twin and with Pillow: no fused multiply-adds.
#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------ prediction
// One thread per stream; reads the state row, changes nothing. Without a track (have = 0) the outputs are zeros.
__global__ __launch_bounds__(64) void track_predict_kernel(const double* __restrict__ state, int n,
                                                           float* __restrict__ quat_out, float* __restrict__ pos_out,
                                                           int* __restrict__ have_out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const double* st = state + (size_t)i * TRACK_STATE;
  const bool have = st[0] != 0.0;
  double q[4], w[3], qp[4] = {0, 0, 0, 0}, tp[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = st[3 + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) w[k] = st[10 + k];
  if (have) {
    track_rotate(w, q, q, qp);
#pragma unroll
    for (int k = 0; k < 3; ++k) tp[k] = st[7 + k] + st[13 + k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) quat_out[4 * (size_t)i + k] = (float)qp[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) pos_out[3 * (size_t)i + k] = (float)tp[k];
  have_out[i] = have ? 1 : 0;
}

hipError_t launch_track_predict(const double* state, int n, float* quat_out, float* pos_out, int* have_out,
                                hipStream_t s) {
  track_predict_kernel<<<(n + 63) / 64, 64, 0, s>>>(state, n, quat_out, pos_out, have_out);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ box of a pose
__device__ __forceinline__ bool roi_finite(double x) { return fabs(x) < INFINITY; }

// One thread per row: spe/roi.py box_of_pose, step by step.
__global__ __launch_bounds__(64) void roi_box_kernel(const float* __restrict__ quat, const float* __restrict__ pos,
                                                     const int* __restrict__ have, int B, int n,
                                                     const float* __restrict__ kp3d, double fu, double fv, double uc,
                                                     double vc, EpnpDist dist, int Hin, int Win, double aspect,
                                                     double margin, double min_side, int* __restrict__ box_out,
                                                     int* __restrict__ status) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const double q0 = (double)quat[4 * (size_t)b], q1 = (double)quat[4 * (size_t)b + 1];
  const double q2 = (double)quat[4 * (size_t)b + 2], q3 = (double)quat[4 * (size_t)b + 3];
  const double t0 = (double)pos[3 * (size_t)b], t1 = (double)pos[3 * (size_t)b + 1], t2 = (double)pos[3 * (size_t)b + 2];
  bool ok = (!have || have[b] != 0) && roi_finite(q0) && roi_finite(q1) && roi_finite(q2) && roi_finite(q3) &&
            roi_finite(t0) && roi_finite(t1) && roi_finite(t2);
  int x0 = 0, y0 = 0, x1 = Win, y1 = Hin;
  if (ok) {
    // quat2dcm (spe/utils.py:10-53), as spef_amd.quaternion.quat2dcm writes it
    const double R[3][3] = {
        {2 * (q0 * q0) - 1 + 2 * (q1 * q1), 2 * q1 * q2 - 2 * q0 * q3, 2 * q1 * q3 + 2 * q0 * q2},
        {2 * q1 * q2 + 2 * q0 * q3, 2 * (q0 * q0) - 1 + 2 * (q2 * q2), 2 * q2 * q3 - 2 * q0 * q1},
        {2 * q1 * q3 - 2 * q0 * q2, 2 * q2 * q3 + 2 * q0 * q1, 2 * (q0 * q0) - 1 + 2 * (q3 * q3)}};
    double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
    for (int i = 0; i <= n && ok; ++i) {   // the origin first, then the n model points
      double p0 = 0.0, p1 = 0.0, p2 = 0.0;
      if (i > 0) {
        p0 = (double)kp3d[3 * (i - 1)];
        p1 = (double)kp3d[3 * (i - 1) + 1];
        p2 = (double)kp3d[3 * (i - 1) + 2];
      }
      const double X = ((R[0][0] * p0 + R[0][1] * p1) + R[0][2] * p2) + t0;
      const double Y = ((R[1][0] * p0 + R[1][1] * p1) + R[1][2] * p2) + t1;
      const double Z = ((R[2][0] * p0 + R[2][1] * p1) + R[2][2] * p2) + t2;
      if (!(Z > 0.0)) {
        ok = false;
        break;
      }
      double x = X / Z, y = Y / Z;
      if (dist.on) {   // keypoints_utils.py:77-82, in its order of operations
        const double xu = x, yu = y;
        const double r2 = xu * xu + yu * yu;
        const double cdist = ((1 + dist.k1 * r2) + (dist.k2 * r2) * r2) + ((dist.k3 * r2) * r2) * r2;
        x = (xu * cdist + ((dist.p1 * 2) * xu) * yu) + dist.p2 * (r2 + (2 * xu) * xu);
        y = (yu * cdist + dist.p1 * (r2 + (2 * yu) * yu)) + ((dist.p2 * 2) * xu) * yu;
      }
      const double u = fu * x + uc, v = fv * y + vc;
      if (!roi_finite(u) || !roi_finite(v)) {
        ok = false;
        break;
      }
      xmin = fmin(xmin, u);
      xmax = fmax(xmax, u);
      ymin = fmin(ymin, v);
      ymax = fmax(ymax, v);
    }
    if (ok) {
      const double cx = (xmin + xmax) * 0.5, cy = (ymin + ymax) * 0.5;
      double w = xmax - xmin, h = ymax - ymin;
      w = w + (2 * margin) * w;
      h = h + (2 * margin) * h;
      w = fmax(w, min_side);
      h = fmax(h, min_side);
      if (w < h * aspect)
        w = h * aspect;
      else
        h = w / aspect;
      // wider than the frame (or not a number a 32-bit size holds): the full frame
      if (!(w + 0.5 < (double)Win + 1.0) || !(h + 0.5 < (double)Hin + 1.0)) {
        ok = false;
      } else {
        const int wi = (int)floor(w + 0.5), hi = (int)floor(h + 0.5);
        const double fx0 = floor((cx - w * 0.5) + 0.5), fy0 = floor((cy - h * 0.5) + 0.5);
        if (wi > Win || hi > Hin || wi < 1 || hi < 1) {
          ok = false;
        } else {
          // shift into the frame; the size stays (the comparisons are in double: the corner may be far outside)
          x0 = fx0 < 0.0 ? 0 : (fx0 + wi > (double)Win ? Win - wi : (int)fx0);
          y0 = fy0 < 0.0 ? 0 : (fy0 + hi > (double)Hin ? Hin - hi : (int)fy0);
          x1 = x0 + wi;
          y1 = y0 + hi;
        }
      }
    }
  }
  if (!ok) {
    x0 = 0;
    y0 = 0;
    x1 = Win;
    y1 = Hin;
  }
  box_out[4 * (size_t)b] = x0;
  box_out[4 * (size_t)b + 1] = y0;
  box_out[4 * (size_t)b + 2] = x1;
  box_out[4 * (size_t)b + 3] = y1;
  status[b] = ok ? 0 : ROI_FULL_FRAME;
}

hipError_t launch_roi_boxes(const float* quat, const float* pos, const int* have, int B, int n, const float* kp3d,
                            const double* K, const EpnpDist& dist, int Hin, int Win, int H, int W, double margin,
                            double min_side, int* box_out, int* status, hipStream_t s) {
  roi_box_kernel<<<(B + 63) / 64, 64, 0, s>>>(quat, pos, have, B, n, kp3d, K[0], K[4], K[2], K[5], dist, Hin, Win,
                                               (double)W / (double)H, margin, min_side, box_out, status);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ coefficients
// Table layout per frame and axis (ints): [out][2] (first source index in the frame, count), then [out][kstr]
// coefficients with 22 fractional bits, zero from `count` on. One thread per (frame, axis, output index): pil_coeffs
// (api_decode.cpp) on the box side, in its order of operations, with the box corner added to the first index.
// valid[b] = 0 for a box that is not inside the frame or has a side below 1: its tables are zeros.
__global__ __launch_bounds__(256) void roi_coeffs_kernel(const int* __restrict__ box, int B, int Hin, int Win, int H,
                                                         int W, int kstr_h, int kstr_v, int* __restrict__ tab_h,
                                                         int* __restrict__ tab_v, int* __restrict__ valid,
                                                         int* __restrict__ status) {
  const int per = W + H;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)B * per) return;
  const int b = (int)(t / per), r = (int)(t - (int64_t)b * per);
  const int x0 = box[4 * (size_t)b], y0 = box[4 * (size_t)b + 1], x1 = box[4 * (size_t)b + 2], y1 = box[4 * (size_t)b + 3];
  const bool good = x0 >= 0 && y0 >= 0 && x1 <= Win && y1 <= Hin && x1 > x0 && y1 > y0;
  if (r == 0) {
    valid[b] = good ? 1 : 0;
    if (status) status[b] = good ? 0 : ROI_BAD_BOX;
  }
  const bool horiz = r < W;
  const int xx = horiz ? r : r - W;
  const int out_size = horiz ? W : H, kstr = horiz ? kstr_h : kstr_v;
  int* tab = horiz ? tab_h + (size_t)b * W * (2 + kstr_h) : tab_v + (size_t)b * H * (2 + kstr_v);
  int* bounds = tab + 2 * xx;
  int* kk = tab + 2 * out_size + (size_t)xx * kstr;
  if (!good) {
    bounds[0] = 0;
    bounds[1] = 0;
    for (int x = 0; x < kstr; ++x) kk[x] = 0;
    return;
  }
  const int in_size = horiz ? x1 - x0 : y1 - y0, off = horiz ? x0 : y0;
  const double scale = (double)(float)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  const double center = (xx + 0.5) * scale;
  const double ss = 1.0 / filterscale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  if (xmax > kstr) xmax = kstr;   // never: count <= 2 ceil(support) + 1 <= the full frame's ksize <= kstr
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) {
    double tt = (x + xmin - center + 0.5) * ss;
    if (tt < 0.0) tt = -tt;
    ww += tt < 1.0 ? 1.0 - tt : 0.0;
  }
  for (int x = 0; x < kstr; ++x) {
    int c = 0;
    if (x < xmax) {
      double tt = (x + xmin - center + 0.5) * ss;
      if (tt < 0.0) tt = -tt;
      double k = tt < 1.0 ? 1.0 - tt : 0.0;
      if (ww != 0.0) k /= ww;
      c = k < 0 ? (int)(-0.5 + k * (1 << 22)) : (int)(0.5 + k * (1 << 22));
    }
    kk[x] = c;
  }
  bounds[0] = xmin + off;
  bounds[1] = xmax;
}

hipError_t launch_roi_coeffs(const int* box, int B, int Hin, int Win, int H, int W, int kstr_h, int kstr_v, int* tab_h,
                             int* tab_v, int* valid, int* status, hipStream_t s) {
  const int64_t n = (int64_t)B * (W + H), nb = (n + 255) / 256;
  if (nb > 0x7fffffff) return hipErrorInvalidValue;
  roi_coeffs_kernel<<<(unsigned)nb, 256, 0, s>>>(box, B, Hin, Win, H, W, kstr_h, kstr_v, tab_h, tab_v, valid, status);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ resample
__device__ __forceinline__ uint32_t roi_clip8(int v) {
  v >>= 22;
  return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// in [B][Hin][Win][3], out [B][H][W][3]; tab_h / tab_v / valid as roi_coeffs_kernel writes them. Grid: (tiles in x,
// tiles in y, B). Dynamic LDS (ints first): horizontal bounds [TW][2] and coefficients [TW][kstr_h + 1], vertical bounds
// [TH][2] and coefficients [TH][kstr_v + 1], then the 8-bit tile [rows_cap][tstride] (tstride = 3 TW rounded up to 4).
// kstr_h and kstr_v are multiples of 4 (so + 1 makes the dword stride odd).
__global__ __launch_bounds__(256) void roi_resample_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                           const int* __restrict__ tab_h, const int* __restrict__ tab_v,
                                                           const int* __restrict__ valid, int Hin, int Win, int H, int W,
                                                           int kstr_h, int kstr_v, int TH, int TW, int rows_cap,
                                                           int tstride, size_t in_bytes) {
  extern __shared__ int roi_lds[];
  const int b = blockIdx.z, tid = threadIdx.x;
  const int ox = blockIdx.x * TW, oy = blockIdx.y * TH;
  const int tw = min(TW, W - ox), th = min(TH, H - oy);
  uint8_t* dst = out + (size_t)b * H * W * 3;
  if (!valid[b]) {   // uniform per workgroup: a box that is not inside the frame gives a black frame
    for (int i = tid; i < th * tw * 3; i += 256) {
      const int y = i / (tw * 3), r = i - y * (tw * 3);
      dst[((size_t)(oy + y) * W + ox) * 3 + r] = 0;
    }
    return;
  }
  const int sh = kstr_h + 1, sv = kstr_v + 1;
  int* bh = roi_lds;               // [TW][2]
  int* ch = bh + 2 * TW;           // [TW][sh]
  int* bv = ch + TW * sh;          // [TH][2]
  int* cv = bv + 2 * TH;           // [TH][sv]
  uint8_t* tile = reinterpret_cast<uint8_t*>(cv + TH * sv);
  const int* gh = tab_h + (size_t)b * W * (2 + kstr_h);
  const int* gv = tab_v + (size_t)b * H * (2 + kstr_v);
  for (int i = tid; i < 2 * tw; i += 256) bh[i] = gh[2 * ox + i];
  for (int i = tid; i < tw * kstr_h; i += 256) {
    const int x = i / kstr_h, k = i - x * kstr_h;
    ch[x * sh + k] = gh[2 * W + (size_t)(ox + x) * kstr_h + k];
  }
  for (int i = tid; i < 2 * th; i += 256) bv[i] = gv[2 * oy + i];
  for (int i = tid; i < th * kstr_v; i += 256) {
    const int y = i / kstr_v, k = i - y * kstr_v;
    cv[y * sv + k] = gv[2 * H + (size_t)(oy + y) * kstr_v + k];
  }
  __syncthreads();
  // source rows of the tile: the first row of its first output row to the last row of its last one (both monotonic)
  const int row0 = bv[0];
  int rows = bv[2 * (th - 1)] + bv[2 * (th - 1) + 1] - row0;
  rows = min(rows, rows_cap);   // never more: rows_cap is the bound for the full frame (api_roi.cpp)

  // ---- horizontal pass: item = (row, x), x fastest
  const uint8_t* frame = in + (size_t)b * Hin * Win * 3;
  const uintptr_t last_word = ((uintptr_t)in + in_bytes - 1) & ~(uintptr_t)3;   // the last dword holding a frame byte
  for (int i = tid; i < rows * tw; i += 256) {
    const int r = i / tw, x = i - r * tw;
    const int xmin = bh[2 * x], n = bh[2 * x + 1];
    const int* k = ch + x * sh;
    const uintptr_t a = (uintptr_t)(frame + ((size_t)(row0 + r) * Win + xmin) * 3);
    uintptr_t wa = a & ~(uintptr_t)3;
    const uint32_t sft = (uint32_t)(a & 3);
    int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
    uint32_t w0 = *reinterpret_cast<const uint32_t*>(wa < last_word ? wa : last_word);
    for (int g = 0; g < n; g += 4) {   // four pixels = 12 bytes = the dwords w0..w3 shifted by sft bytes
      const uint32_t w1 = *reinterpret_cast<const uint32_t*>(wa + 4 < last_word ? wa + 4 : last_word);
      const uint32_t w2 = *reinterpret_cast<const uint32_t*>(wa + 8 < last_word ? wa + 8 : last_word);
      const uint32_t w3 = *reinterpret_cast<const uint32_t*>(wa + 12 < last_word ? wa + 12 : last_word);
      const uint32_t d0 = __builtin_amdgcn_alignbyte(w1, w0, sft);
      const uint32_t d1 = __builtin_amdgcn_alignbyte(w2, w1, sft);
      const uint32_t d2 = __builtin_amdgcn_alignbyte(w3, w2, sft);
      const int k0 = k[g], k1 = k[g + 1], k2 = k[g + 2], k3 = k[g + 3];   // zero past n (kstr is a multiple of 4)
      s0 += (int)(d0 & 255) * k0 + (int)(d0 >> 24) * k1 + (int)((d1 >> 16) & 255) * k2 + (int)((d2 >> 8) & 255) * k3;
      s1 += (int)((d0 >> 8) & 255) * k0 + (int)(d1 & 255) * k1 + (int)(d1 >> 24) * k2 + (int)((d2 >> 16) & 255) * k3;
      s2 += (int)((d0 >> 16) & 255) * k0 + (int)((d1 >> 8) & 255) * k1 + (int)(d2 & 255) * k2 + (int)(d2 >> 24) * k3;
      w0 = w3;
      wa += 12;
    }
    uint8_t* t = tile + (size_t)r * tstride + 3 * x;
    t[0] = (uint8_t)roi_clip8(s0);
    t[1] = (uint8_t)roi_clip8(s1);
    t[2] = (uint8_t)roi_clip8(s2);
  }
  __syncthreads();

  // ---- vertical pass: item = (y, dword of the row), four consecutive bytes of the tile row share every coefficient
  const int nbytes = tw * 3, nd = (nbytes + 3) >> 2;
  for (int i = tid; i < th * nd; i += 256) {
    const int y = i / nd, d = i - y * nd;
    const int r0 = bv[2 * y] - row0, n = bv[2 * y + 1];
    const int* k = cv + y * sv;
    int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21, a3 = 1 << 21;
    for (int j = 0; j < n; ++j) {
      const int rr = min(r0 + j, rows_cap - 1);   // never clamps (see rows above)
      const uint32_t v = *reinterpret_cast<const uint32_t*>(tile + (size_t)rr * tstride + 4 * d);
      const int c = k[j];
      a0 += (int)(v & 255) * c;
      a1 += (int)((v >> 8) & 255) * c;
      a2 += (int)((v >> 16) & 255) * c;
      a3 += (int)(v >> 24) * c;
    }
    const uint32_t o0 = roi_clip8(a0), o1 = roi_clip8(a1), o2 = roi_clip8(a2), o3 = roi_clip8(a3);
    uint8_t* o = dst + ((size_t)(oy + y) * W + ox) * 3 + 4 * d;
    const int left = nbytes - 4 * d;   // bytes of this dword inside the tile row
    if (left >= 4 && ((uintptr_t)o & 3) == 0) {
      *reinterpret_cast<uint32_t*>(o) = o0 | (o1 << 8) | (o2 << 16) | (o3 << 24);
    } else {
      o[0] = (uint8_t)o0;
      if (left > 1) o[1] = (uint8_t)o1;
      if (left > 2) o[2] = (uint8_t)o2;
      if (left > 3) o[3] = (uint8_t)o3;
    }
  }
}

size_t roi_resample_lds_bytes(int kstr_h, int kstr_v, int TH, int TW, int rows_cap) {
  const size_t tstride = ((size_t)TW * 3 + 3) & ~(size_t)3;
  return sizeof(int) * ((size_t)TW * (2 + kstr_h + 1) + (size_t)TH * (2 + kstr_v + 1)) + (size_t)rows_cap * tstride;
}

hipError_t launch_roi_resample(const uint8_t* in, uint8_t* out, const int* tab_h, const int* tab_v, const int* valid,
                               int B, int Hin, int Win, int H, int W, int kstr_h, int kstr_v, int TH, int TW,
                               int rows_cap, hipStream_t s) {
  const int tstride = (TW * 3 + 3) & ~3;
  const size_t lds = roi_resample_lds_bytes(kstr_h, kstr_v, TH, TW, rows_cap);
  const dim3 grid((W + TW - 1) / TW, (H + TH - 1) / TH, B);
  if (grid.y > 65535 || B > 65535 || lds > 64 * 1024) return hipErrorInvalidValue;
  roi_resample_kernel<<<grid, 256, lds, s>>>(in, out, tab_h, tab_v, valid, Hin, Win, H, W, kstr_h, kstr_v, TH, TW,
                                             rows_cap, tstride, (size_t)B * Hin * Win * 3);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ un-mapping
// One thread per coordinate: the sigmoid exactly as epnp_kernel applies it (float32), then the map from the crop back
// to the frame in fp64, rounded once to float32: u = (x0 + s (x1 - x0)) / nu, v = (y0 + s (y1 - y0)) / nv.
__global__ __launch_bounds__(256) void roi_unmap_kernel(const float* __restrict__ raw, const int* __restrict__ box, int B,
                                                        int nk, float nu, float nv, int apply_sigmoid,
                                                        float* __restrict__ kp_out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)B * nk) return;
  const int b = (int)(t / nk), j = (int)(t - (int64_t)b * nk);
  float x = raw[t];
  if (apply_sigmoid) x = 1.0f / (1.0f + expf(-x));   // spe_utils.py:68, float32
  const int axis = j & 1;
  const double lo = (double)box[4 * (size_t)b + axis], hi = (double)box[4 * (size_t)b + 2 + axis];
  const double size = axis ? (double)nv : (double)nu;
  kp_out[t] = (float)((lo + (double)x * (hi - lo)) / size);
}

hipError_t launch_roi_unmap(const float* raw, const int* box, int B, int nk, float nu, float nv, int apply_sigmoid,
                            float* kp_out, hipStream_t s) {
  const int64_t n = (int64_t)B * nk, nb = (n + 255) / 256;
  if (nb > 0x7fffffff) return hipErrorInvalidValue;
  roi_unmap_kernel<<<(unsigned)nb, 256, 0, s>>>(raw, box, B, nk, nu, nv, apply_sigmoid, kp_out);
  return hipGetLastError();
}

}  // namespace spef
