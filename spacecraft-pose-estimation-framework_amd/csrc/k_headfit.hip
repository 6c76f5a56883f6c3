// Head-fit kernels on gfx950: one optimisation step of the URSONet head's two Linear layers over cached backbone
// features (include/spef.h, spef_headfit_step; spef_amd/solver/head_fit.py is the NumPy twin and states every step).
//
//   headfit_dropout_kernel  nn.Dropout(0.2) on the orientation branch's input (src/modeling/head/ursonet.py): Xd = X *
//                           keep / (1 - p), keep from an integer hash of (seed, step, element)
//   (forward)               launch_fc (k_head.hip) on the trainer's weights
//   headfit_loss_kernel     SoftClassLoss (src/solver/loss.py:109) behind SPEUtils.last_activ's softmax
//                           (src/spe/spe_utils.py:75-79), and the row sums of PosRegLoss (loss.py:35-37); G = dLoss/dlogit
//   headfit_finish_kernel   the batch means (torch.mean, loss.py:96), SPELoss.compute_loss's beta * ori + pos
//                           (loss.py:157), PosRegLoss' batch-wide norms and its G, the step counter, Adam's bias corrections
//   headfit_update_kernel   dW = G^T Xsel on the exact f32-input MFMA with torch.optim.SGD / torch.optim.Adam
//                           (src/solver/optimizer.py:45-57) applied from the accumulator registers; the bias likewise
// Nothing here uses atomics, and every sum has a fixed order: a step is deterministic and independent of the grid.
#include <math.h>

#include "spef_common.hpp"
#include "spef_kernels.hpp"
#include "spef_reduce.hpp"

namespace spef {

// ------------------------------------------------------------------------------------------ target encoding
// OrientationSoftClassification.encode (src/spe/classification_utils.py:85-111) and PositionSoftClassification.encode
// (:217-240), one workgroup per (row, head), in fp64 without fused multiply-adds:
//   ori  k_i = exp(-((2 acos(min(1, |q . h_i|)) / pi)^2) / (2 var)), 0 for a masked (redundant) bin
//   pos  k_i = exp(-|t - g_i|^2 / (2 var))
// out_i = float32(k_i / sum k); the sum adds each thread's bins in ascending order, then the threads by
// block_sum256_d. A row with a non-finite input, or whose sum is zero or not finite, is written as NaN and flagged.
__device__ __forceinline__ double encode_kernel_value(bool ori, const double* __restrict__ tab, int i, const double* x,
                                                      double inv2var, const uint8_t* __restrict__ mask) {
#pragma clang fp contract(off)
  if (ori) {
    if (mask && mask[i]) return 0.0;
    const double* h = tab + 4 * (size_t)i;
    const double dot = ((x[0] * h[0] + x[1] * h[1]) + x[2] * h[2]) + x[3] * h[3];
    const double a = 2.0 * acos(fmin(1.0, fabs(dot))) / 3.141592653589793;
    return exp(-(a * a) * inv2var);
  }
  const double* g = tab + 3 * (size_t)i;
  const double d0 = x[0] - g[0], d1 = x[1] - g[1], d2 = x[2] - g[2];
  return exp(-((d0 * d0 + d1 * d1) + d2 * d2) * inv2var);
}

__global__ __launch_bounds__(256) void encode_targets_kernel(const double* __restrict__ quat,
                                                             const double* __restrict__ pos,
                                                             const double* __restrict__ q_bins, int n_ori,
                                                             const double* __restrict__ grid, int n_pos, double ori_i2v,
                                                             double pos_i2v, const uint8_t* __restrict__ mask,
                                                             float* __restrict__ ori_soft, float* __restrict__ pos_soft,
                                                             int* __restrict__ status) {
  __shared__ double sh[4];
  const int b = blockIdx.x, head = blockIdx.y, tid = threadIdx.x;
  const bool ori = head == 0;
  float* out = ori ? ori_soft : pos_soft;
  if (!out) {
    if (tid == 0) status[2 * b + head] = 0;
    return;
  }
  const int n = ori ? n_ori : n_pos, w = ori ? 4 : 3;
  const double* tab = ori ? q_bins : grid;
  const double i2v = ori ? ori_i2v : pos_i2v;
  double x[4] = {0.0, 0.0, 0.0, 0.0};
  bool ok = true;
  for (int j = 0; j < w; ++j) {
    x[j] = (ori ? quat : pos)[(size_t)b * w + j];
    ok = ok && isfinite(x[j]);
  }
  double acc = 0.0;
  for (int i = tid; i < n; i += 256) acc += encode_kernel_value(ori, tab, i, x, i2v, ori ? mask : nullptr);
  const double sum = block_sum256_d(acc, sh);
  ok = ok && isfinite(sum) && sum > 0.0;
  out += (size_t)b * n;
  for (int i = tid; i < n; i += 256)
    out[i] = ok ? (float)(encode_kernel_value(ori, tab, i, x, i2v, ori ? mask : nullptr) / sum) : NAN;
  if (tid == 0) status[2 * b + head] = ok ? 0 : 1;
}

// ------------------------------------------------------------------------------------------ dropout
// The hash of head_fit.dropout_hash: murmur3's 32-bit finaliser over the element index, the seed and the step.
__device__ __forceinline__ uint32_t headfit_hash(uint32_t seed, uint32_t step, uint32_t idx) {
  uint32_t x = idx * 0x9E3779B1u + seed;
  x ^= step * 0x85EBCA77u;
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

__global__ __launch_bounds__(256) void headfit_dropout_kernel(const float* __restrict__ X, float* __restrict__ Xd,
                                                              uint32_t n, uint32_t seed, uint32_t thr, float inv_keep,
                                                              const uint32_t* __restrict__ counter) {
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= n) return;
  const uint32_t h = headfit_hash(seed, counter[0], idx);
  Xd[idx] = h >= thr ? X[idx] * inv_keep : 0.0f;
}

// ------------------------------------------------------------------------------------------ loss and G
// One workgroup per (row, head). Classification: m = max z, d = z - m, s = sum expf(d) (float32, as decode_ori_kernel),
// p = expf(d) / s, log p = d - logf(s); the row loss -sum t * log p adds the float32 products in fp64;
// G = (p - t) * scale_over_B. Regression (position): the row's sum of (pred - target)^2 and of target^2 in fp64; its G
// needs the batch's norm and is written by headfit_finish_kernel.
__global__ __launch_bounds__(256) void headfit_loss_kernel(const float* __restrict__ Zo, const float* __restrict__ To,
                                                           const float* __restrict__ Zp, const float* __restrict__ Tp,
                                                           int n_ori, int n_pos, int Np, int pos_reg, float so, float sp,
                                                           float* __restrict__ G, double* __restrict__ rowloss,
                                                           double* __restrict__ rowaux, int Bmax,
                                                           float* __restrict__ logits_out) {
  __shared__ float shf[2][4];
  __shared__ double shd[4];
  const int b = blockIdx.x, head = blockIdx.y, tid = threadIdx.x;
  const int n = head ? n_pos : n_ori, c0 = head ? n_ori : 0;
  const float* z = (head ? Zp : Zo) + (size_t)b * n;
  float* lo = logits_out ? logits_out + (size_t)b * (n_ori + n_pos) + c0 : nullptr;
  if (head && pos_reg) {
    if (tid == 0) {
      double sq = 0.0, tq = 0.0;
      for (int j = 0; j < 3; ++j) {
        const double t = (double)Tp[3 * (size_t)b + j], d = (double)z[j] - t;
        sq += d * d;
        tq += t * t;
        if (lo) lo[j] = z[j];
      }
      rowloss[Bmax + b] = sq;
      rowaux[b] = tq;
      // the columns past n_ori + 3 of G are padding and stay as spef_headfit_create zeroed them
    }
    return;
  }
  const float* t = (head ? Tp : To) + (size_t)b * n;
  const float scale = head ? sp : so;
  float m = -INFINITY;
  for (int i = tid; i < n; i += 256) m = fmaxf(m, z[i]);
  m = block_max256(m, shf[0]);
  float s = 0.0f;
  for (int i = tid; i < n; i += 256) s += expf(z[i] - m);
  s = block_sum256(s, shf[1]);
  const float ls = logf(s);
  double acc = 0.0;
  float* g = G + (size_t)b * Np + c0;
  for (int i = tid; i < n; i += 256) {
    const float zi = z[i], d = zi - m, p = expf(d) / s, ti = t[i];
    acc += (double)(ti * (d - ls));
    g[i] = (p - ti) * scale;
    if (lo) lo[i] = zi;
  }
  acc = block_sum256_d(acc, shd);
  if (tid == 0) rowloss[(size_t)head * Bmax + b] = -acc;
}

// One workgroup. The batch means in fp64 (thread-strided partial sums, then block_sum256_d: a fixed order), the total,
// PosRegLoss' Frobenius norms over the whole batch with its G, and with `train` the step counter: counter[1] = the index of
// this step (what the update reads), counter[0] = the steps completed. sc[0] = 1 - beta1^t, sc[1] = sqrt(1 - beta2^t), t =
// counter[1] + 1 (torch.optim.Adam's bias corrections, computed in fp64 and rounded to float32).
__global__ __launch_bounds__(256) void headfit_finish_kernel(const double* __restrict__ rowloss,
                                                             const double* __restrict__ rowaux, int B, int Bmax,
                                                             int pos_reg, int norm_distance, double beta,
                                                             const float* __restrict__ Zp, const float* __restrict__ Tp,
                                                             int n_ori, int Np, float* __restrict__ G, int train,
                                                             double beta1, double beta2, uint32_t* __restrict__ counter,
                                                             float* __restrict__ sc, float* __restrict__ loss_out) {
  __shared__ double sh[3][4];
  const int tid = threadIdx.x;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (int b = tid; b < B; b += 256) {
    a0 += rowloss[b];
    a1 += rowloss[Bmax + b];
    if (pos_reg) a2 += rowaux[b];
  }
  a0 = block_sum256_d(a0, sh[0]);
  a1 = block_sum256_d(a1, sh[1]);
  a2 = block_sum256_d(a2, sh[2]);
  const double lo = a0 / (double)B;
  double lp;
  if (pos_reg) {
    const double nd = sqrt(a1), nt = sqrt(a2);
    lp = norm_distance ? nd / nt : nd;
    // d|pred - target|_F / dpred = (pred - target) / |pred - target|_F, zero at a zero norm (where autograd gives NaN)
    for (int e = tid; e < 3 * B; e += 256) {
      const int b = e / 3, j = e - 3 * b;
      double g = 0.0;
      if (nd > 0.0) {
        g = ((double)Zp[e] - (double)Tp[e]) / nd;
        if (norm_distance) g /= nt;
      }
      G[(size_t)b * Np + n_ori + j] = (float)g;
    }
  } else {
    lp = a1 / (double)B;
  }
  if (tid != 0) return;
  if (loss_out) {
    loss_out[0] = (float)(beta * lo + lp);
    loss_out[1] = (float)lo;
    loss_out[2] = (float)lp;
  }
  if (train) {
    const uint32_t t = counter[0];
    counter[1] = t;
    counter[0] = t + 1;
    sc[0] = (float)(1.0 - pow(beta1, (double)t + 1.0));
    sc[1] = (float)sqrt(1.0 - pow(beta2, (double)t + 1.0));
  }
}

// ------------------------------------------------------------------------------------------ backward + optimizer
// The float32 operation order of head_fit.sgd_step / head_fit.adam_step, one rounding per operation (no contraction into
// FMAs: the twin's NumPy float32 arithmetic gives the same bits from the same gradient).
struct HeadFitScalars {
  float lr, momentum, wd, b1, omb1, b2, omb2, eps, bc1, bc2s;
};
template <int OPT>
__device__ __forceinline__ void headfit_apply(float g, float& w, float& s1, float& s2, const HeadFitScalars& o) {
#pragma clang fp contract(off)
  const float t0 = o.wd * w;
  g = g + t0;
  if constexpr (OPT == HF_SGD) {
    const float t1 = o.momentum * s1;
    s1 = t1 + g;
    const float t2 = o.lr * s1;
    w = w - t2;
  } else {
    const float t1 = o.b1 * s1, t2 = o.omb1 * g;
    s1 = t1 + t2;
    const float t3 = o.b2 * s2, t4 = o.omb2 * g, t5 = t4 * g;
    s2 = t3 + t5;
    const float den = sqrtf(s2) / o.bc2s + o.eps;
    const float step = o.lr / o.bc1;
    const float t6 = s1 / den, t7 = step * t6;
    w = w - t7;
  }
}

// dW[i][k] = sum_b G[b][i] Xsel[b][k] as D[m][n] = sum_b A[m][b] B[b][n] with A = X^T (m = column k) and B = G (n = row i)
// on v_mfma_f32_16x16x4_f32: lane l feeds A[m = l&15][b = b0 + (l>>4)] = X[b][k0 + (l&15)] and B[b][n = l&15] = G[b][i0 +
// (l&15)], and holds D[m = 4(l>>4) + r][n = l&15] = dW[i0 + (l&15)][k0 + 4(l>>4) + r], r = 0..3: a float4 of one weight row.
// The MFMA is a k-ordered chain of float32 FMAs, and a wave walks b upwards in steps of 4 (rows past B enter as zeros), so
// every dW element is the same ascending chain whatever the grid. A wave owns 16 rows x 64 columns (4 accumulators), a
// workgroup 16 rows x 256 columns; grid (Np / 16, ceil(K / 256)).
// Rows below n_ori contract with Xo (the dropout copy, or X), the rows from n_ori with X. A 16-row tile that holds both
// kinds (n_ori % 16 != 0, dropout on) runs both operands through the same accumulators, G masked to the rows each belongs
// to: the other kind's products are exact zeros, so each element's chain is unchanged.
// The epilogue reads W and the optimizer state once, applies the step from the accumulators and writes them once; dW goes
// to memory only when grad_out is given. The tile column 0's first 16 lanes also sum the bias gradient over b in
// ascending order and update the bias. Rows at or past n (padding) are never written: they stay exactly zero.
template <int OPT>
__global__ __launch_bounds__(256) void headfit_update_kernel(const float* __restrict__ G, const float* __restrict__ Xo,
                                                             const float* __restrict__ Xp, float* __restrict__ W,
                                                             float* __restrict__ S1, float* __restrict__ S2,
                                                             float* __restrict__ bias, float* __restrict__ bS1,
                                                             float* __restrict__ bS2, float* __restrict__ grad_out,
                                                             const float* __restrict__ lr, const float* __restrict__ sc,
                                                             HeadFitScalars o, int B, int K, int n_ori, int n, int Np) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r16 = lane & 15, kg = lane >> 4;
  const int i0 = blockIdx.x * 16, i = i0 + r16;
  const int kbase = (blockIdx.y * 4 + wave) * 64;
  o.lr = lr[0];
  o.bc1 = sc[0];
  o.bc2s = sc[1];
  const bool dual = Xo != Xp && i0 < n_ori && i0 + 16 > n_ori;
  const float* Xa = i0 < n_ori ? Xo : Xp;
  const bool irow = i < n;
  if (kbase < K) {
    bool tv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) tv[t] = kbase + 16 * t < K;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!dual) {

      for (int b0 = 0; b0 < B; b0 += 4) {
        const int bb = b0 + kg;
        const bool bv = bb < B;
        const float g = bv && irow ? G[(size_t)bb * Np + i] : 0.0f;
        const float* xr = Xa + (size_t)(bv ? bb : 0) * K + kbase + r16;
        float a[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) a[t] = bv && tv[t] ? xr[16 * t] : 0.0f;
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], g, acc[t], 0, 0, 0);
      }
    } else {
      const bool ori = i < n_ori;

      for (int b0 = 0; b0 < B; b0 += 4) {
        const int bb = b0 + kg;
        const bool bv = bb < B;
        const float g = bv && irow ? G[(size_t)bb * Np + i] : 0.0f;
        const float go = ori ? g : 0.0f, gp = ori ? 0.0f : g;
        const size_t off = (size_t)(bv ? bb : 0) * K + kbase + r16;
        float a[4], c[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          a[t] = bv && tv[t] ? Xo[off + 16 * t] : 0.0f;
          c[t] = bv && tv[t] ? Xp[off + 16 * t] : 0.0f;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], go, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(c[t], gp, acc[t], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (!tv[t]) continue;
      const size_t off = (size_t)i * K + kbase + 16 * t + 4 * kg;   // i < Np: inside W and grad_out
      if (grad_out) *reinterpret_cast<float4*>(grad_out + off) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
      if (!irow) continue;
      float4 w = *reinterpret_cast<const float4*>(W + off);
      float4 s1 = *reinterpret_cast<const float4*>(S1 + off);
      float4 s2 = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (OPT == HF_ADAM) s2 = *reinterpret_cast<const float4*>(S2 + off);
      headfit_apply<OPT>(acc[t][0], w.x, s1.x, s2.x, o);
      headfit_apply<OPT>(acc[t][1], w.y, s1.y, s2.y, o);
      headfit_apply<OPT>(acc[t][2], w.z, s1.z, s2.z, o);
      headfit_apply<OPT>(acc[t][3], w.w, s1.w, s2.w, o);
      *reinterpret_cast<float4*>(W + off) = w;
      *reinterpret_cast<float4*>(S1 + off) = s1;
      if constexpr (OPT == HF_ADAM) *reinterpret_cast<float4*>(S2 + off) = s2;
    }
  }
  if (blockIdx.y == 0 && wave == 0 && kg == 0) {
    float db = 0.0f;
    if (irow)
      for (int b = 0; b < B; ++b) db += G[(size_t)b * Np + i];
    if (grad_out) grad_out[(size_t)Np * K + i] = db;
    if (irow) {
      float w = bias[i], s1 = bS1[i], s2 = OPT == HF_ADAM ? bS2[i] : 0.0f;
      headfit_apply<OPT>(db, w, s1, s2, o);
      bias[i] = w;
      bS1[i] = s1;
      if constexpr (OPT == HF_ADAM) bS2[i] = s2;
    }
  }
}

// ------------------------------------------------------------------------------------------ launchers
hipError_t launch_encode_targets(const double* quat, const double* pos, int B, const double* q_bins, int n_ori,
                                 const double* grid, int n_pos, double ori_var, double pos_var, const uint8_t* mask,
                                 float* ori_soft, float* pos_soft, int* status, hipStream_t s) {
  encode_targets_kernel<<<dim3(B, 2), 256, 0, s>>>(quat, pos, q_bins, n_ori, grid, n_pos, 1.0 / (2.0 * ori_var),
                                                   1.0 / (2.0 * pos_var), mask, ori_soft, pos_soft, status);
  return hipGetLastError();
}

hipError_t launch_headfit_dropout(const float* X, float* Xd, int B, int K, uint32_t seed, uint32_t thr, float inv_keep,
                                  const uint32_t* counter, hipStream_t s) {
  const int64_t n = (int64_t)B * K;
  if (n > 0x7fffffff) return hipErrorInvalidValue;
  headfit_dropout_kernel<<<(uint32_t)((n + 255) / 256), 256, 0, s>>>(X, Xd, (uint32_t)n, seed, thr, inv_keep, counter);
  return hipGetLastError();
}

hipError_t launch_headfit_loss(const HeadFitShape& d, const float* Zo, const float* To, const float* Zp, const float* Tp,
                               int B, int pos_reg, float so, float sp, float* G, double* rowloss, double* rowaux,
                               float* logits_out, hipStream_t s) {
  headfit_loss_kernel<<<dim3(B, 2), 256, 0, s>>>(Zo, To, Zp, Tp, d.n_ori, d.n_pos, d.Np, pos_reg, so, sp, G, rowloss,
                                                 rowaux, d.Bmax, logits_out);
  return hipGetLastError();
}

hipError_t launch_headfit_finish(const HeadFitShape& d, const double* rowloss, const double* rowaux, int B, int pos_reg,
                                 int norm_distance, double beta, const float* Zp, const float* Tp, float* G, int train,
                                 double beta1, double beta2, uint32_t* counter, float* sc, float* loss_out,
                                 hipStream_t s) {
  headfit_finish_kernel<<<1, 256, 0, s>>>(rowloss, rowaux, B, d.Bmax, pos_reg, norm_distance, beta, Zp, Tp, d.n_ori, d.Np,
                                          G, train, beta1, beta2, counter, sc, loss_out);
  return hipGetLastError();
}

hipError_t launch_headfit_update(const HeadFitShape& d, const HeadFitOpt& opt, const float* G, const float* Xo,
                                 const float* Xp, int B, float* W, float* S1, float* S2, float* bias, float* bS1,
                                 float* bS2, float* grad_out, const float* lr, const float* sc, hipStream_t s) {
  if (d.K % 16 || d.Np % 16) return hipErrorInvalidValue;
  HeadFitScalars o{};
  o.momentum = (float)opt.momentum;
  o.wd = (float)opt.weight_decay;
  o.b1 = (float)opt.beta1;
  o.omb1 = (float)(1.0 - opt.beta1);
  o.b2 = (float)opt.beta2;
  o.omb2 = (float)(1.0 - opt.beta2);
  o.eps = (float)opt.eps;
  const dim3 grid(d.Np / 16, (d.K + 255) / 256);
  const int n = d.n_ori + d.n_pos;
  if (opt.kind == HF_SGD)
    headfit_update_kernel<HF_SGD><<<grid, 256, 0, s>>>(G, Xo, Xp, W, S1, S2, bias, bS1, bS2, grad_out, lr, sc, o, B, d.K,
                                                       d.n_ori, n, d.Np);
  else
    headfit_update_kernel<HF_ADAM><<<grid, 256, 0, s>>>(G, Xo, Xp, W, S1, S2, bias, bS1, bS2, grad_out, lr, sc, o, B, d.K,
                                                        d.n_ori, n, d.Np);
  return hipGetLastError();
}

}  // namespace spef
