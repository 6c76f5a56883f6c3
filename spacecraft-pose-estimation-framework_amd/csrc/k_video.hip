// Adaptive video filter on gfx950: the reference's TemporalPDF.update_pdf (src/temporal/pdf_compare.py:94-134) and
// the quaternion pole continuity of Inference.predict (src/temporal/inference.py:136-144, :173-180) for batches of
// video frames. Frames are time-major: row t * S + s is time step t of stream s.
//
//   video_scan_kernel       one 256-thread workgroup per (stream, head); the stream's previous filtered PDF stays in
//                           registers across the t loop (PER values per thread, contiguous bins: thread i owns bins
//                           [i * per, (i + 1) * per), per = ceil(n / 256), which makes the Wasserstein prefix sum a
//                           local running sum plus one workgroup scan of the thread totals)
//   video_pole_kernel       one thread per (stream, still / video): sign flips against the stream's pole
//   video_reset_kernel      clears the "have a previous PDF / pole" flags of one stream or of all
//   video_set_state_kernel  loads one stream's state (the Inference engine shares it with the per-frame host filter)
//
// Arithmetic: elementwise float32 (the reference's NumPy on the float32 soft outputs), every sum fp64 in a fixed
// order (spef_reduce.hpp), rounded to float32 where NumPy's float32 sum stood. Nothing depends on how a sequence
// is cut into calls. Every float32 operation is rounded on its own (no FMA contraction in this file; IEEE divide
// and square root) and exp / log are the fp64 functions rounded to float32, so the host twin
// (spef_amd.temporal.filter_sequences) reproduces the kernel to the last bit except where an fp64 sum lands within
// 1e-16 of a float32 rounding boundary. That is not a luxury: the Jensen-Shannon and Kullback-Leibler sums cancel
// to second order in the difference of the PDFs, and at the distances where the filter blends (d ~ 0.01) one ulp
// of noise in the state moves the Jensen-Shannon distance by more than 1e-5 of itself. What does not depend on the state is kept out of the sequential loop: each frame's two
// normalisation sums (sum(cur), and sum(cur / sum(cur)) that compute_distance divides by again) are computed for
// 64 frames at a time by the four waves in parallel, and the next frame's loads are issued before the current
// frame's reductions. The decode of the filtered PDFs runs afterwards over all T * S frames (k_head.hip).
//
// A frame whose sum is not a positive finite number (all zero, a NaN or an infinity in it) is passed to the output
// as it came, with distance NaN, so that the decode flags it; the stream's state is left as it was, and the next
// good frame is filtered against the last good one. The same holds for the state when a blend does not sum to a
// positive finite number (the Jensen-Shannon distance of PDFs with exact zeros is NaN in the reference as well).
#include <math.h>

#include "spef_common.hpp"
#include "spef_kernels.hpp"
#include "spef_reduce.hpp"

#pragma clang fp contract(off)

namespace spef {

constexpr int VCH = 64;   // frames per pass of the state-independent sums

__device__ __forceinline__ bool pos_finite(float v) { return v > 0.0f && v < INFINITY; }   // false for NaN

// exp / log correctly rounded to float32 (the fp64 function, rounded): the same values on the host.
__device__ __forceinline__ float log_ratio(float r) { return (float)log((double)r); }
__device__ __forceinline__ float exp_r(float x) { return (float)exp((double)x); }

// Exclusive prefix sum over the workgroup of one fp64 per thread (thread order); sh[4] is free again after the
// next barrier but one.
__device__ __forceinline__ double block_exscan256_d(double v, double* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) sh[wave] = x;
  double ex = __shfl_up(x, 1, 64);
  if (lane == 0) ex = 0.0;
  __syncthreads();
  double off = 0.0;
  if (wave > 0) off += sh[0];
  if (wave > 1) off += sh[1];
  if (wave > 2) off += sh[2];
  return off + ex;
}

// METRIC is a template parameter: the per-bin loop is straight-line code for the metric in use.
template <int PER, int METRIC>
__global__ __launch_bounds__(256) void video_scan_kernel(const VideoHead h0, const VideoHead h1, int T, int S) {
  constexpr int metric = METRIC;
  __shared__ float sh_s1[VCH], sh_s2[VCH];
  __shared__ double shr[3][4];
  __shared__ double shx[4];
  const VideoHead h = blockIdx.y ? h1 : h0;
  const int s = blockIdx.x, tid = threadIdx.x, n = h.n;
  const int lane = tid & 63, wave = tid >> 6;
  const int per = (n + 255) >> 8;   // <= PER (the launcher picks PER)
  const int i0 = tid * per;
  bool ok[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) ok[j] = j < per && i0 + j < n;

  bool have = h.have[s] != 0;
  float spf = have ? h.state_sum[s] : 1.0f;
  float prev[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) prev[j] = (have && ok[j]) ? h.state[(size_t)s * n + i0 + j] : 0.0f;

  for (int c0 = 0; c0 < T; c0 += VCH) {
    const int tc = min(VCH, T - c0);
    __syncthreads();   // the previous pass's sums have been read
    // ---- state-independent: s1 = sum(cur), s2 = sum(cur / s1), one wave per frame
    for (int tt = wave; tt < tc; tt += 4) {
      const float* x = h.in + ((size_t)(c0 + tt) * S + s) * n;
      double a = 0.0;
      for (int i = lane; i < n; i += 64) a += (double)x[i];
      const float s1f = (float)wave_sum64_d(a);
      double b = 0.0;
      for (int i = lane; i < n; i += 64) b += (double)(x[i] / s1f);
      const float s2f = (float)wave_sum64_d(b);
      if (lane == 0) {
        sh_s1[tt] = s1f;
        sh_s2[tt] = s2f;
      }
    }
    __syncthreads();
    // ---- the recurrence
    float nxt[PER];
    {
      const float* x = h.in + ((size_t)c0 * S + s) * n + i0;
#pragma unroll
      for (int j = 0; j < PER; ++j) nxt[j] = ok[j] ? x[j] : 0.0f;
    }
    for (int tt = 0; tt < tc; ++tt) {
      float cur[PER];
#pragma unroll
      for (int j = 0; j < PER; ++j) cur[j] = nxt[j];
      if (tt + 1 < tc) {
        const float* x = h.in + ((size_t)(c0 + tt + 1) * S + s) * n + i0;
#pragma unroll
        for (int j = 0; j < PER; ++j) nxt[j] = ok[j] ? x[j] : 0.0f;
      }
      const size_t row = (size_t)(c0 + tt) * S + s;
      float* o = h.filt + row * n + i0;
      const float s1f = sh_s1[tt], s2f = sh_s2[tt];
      if (!(pos_finite(s1f) && pos_finite(s2f))) {   // bad frame: passed on as it is, the state stays
#pragma unroll
        for (int j = 0; j < PER; ++j)
          if (ok[j]) o[j] = cur[j];
        if (tid == 0) h.dist[row] = NAN;
        continue;
      }
#pragma unroll
      for (int j = 0; j < PER; ++j) cur[j] = cur[j] / s1f;   // current_pdf / np.sum(current_pdf)
      if (!have) {                                           // first frame after a reset
#pragma unroll
        for (int j = 0; j < PER; ++j) {
          prev[j] = cur[j];
          if (ok[j]) o[j] = cur[j];
        }
        spf = s2f;
        have = true;
        if (tid == 0) h.dist[row] = 0.0f;
        continue;
      }
      // compute_distance: p = cur / sum(cur), q = prev / sum(prev), both float32
      double acc = 0.0;
      if constexpr (metric == VM_WASSERSTEIN) {   // sum_i |cumsum(p)_i - cumsum(q)_i| / n, the cumulative sums in fp64
        double run = 0.0;
        double df[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) {
          df[j] = ok[j] ? (double)(cur[j] / s2f) - (double)(prev[j] / spf) : 0.0;
          run += df[j];
        }
        run = block_exscan256_d(run, shx);
#pragma unroll
        for (int j = 0; j < PER; ++j) {
          run += df[j];
          acc += ok[j] ? fabs(run) : 0.0;
        }
      } else {
        // every bin slot is computed and the unused ones are selected away (adding 0.0 changes nothing): one
        // basic block, so the PER independent divide chains interleave instead of running one after another
#pragma unroll
        for (int j = 0; j < PER; ++j) {
          const float p = cur[j] / s2f, q = prev[j] / spf;
          float e;
          double e2 = 0.0;
          if constexpr (metric == VM_L2) {
            const float d = p - q;
            e = d * d;
          } else if constexpr (metric == VM_KL) {
            const float ps = p + 1e-12f, qs = q + 1e-12f;
            e = ps * log_ratio(ps / qs);
          } else if constexpr (metric == VM_JS) {
            const float mid = 0.5f * (p + q);
            e2 = (double)(p * log_ratio(p / mid));
            e = q * log_ratio(q / mid);
          } else if constexpr (metric == VM_HELLINGER) {
            const float d = sqrtf(p) - sqrtf(q);
            e = d * d;
          } else {
            e = fabsf(p - q);
          }
          acc += ok[j] ? e2 + (double)e : 0.0;
        }
      }
      const float r = (float)block_sum256_d(acc, shr[0]);
      float d;
      if constexpr (metric == VM_L2) d = sqrtf(r);
      else if constexpr (metric == VM_KL) d = r;
      else if constexpr (metric == VM_JS || metric == VM_HELLINGER) d = sqrtf(0.5f * r);
      else if constexpr (metric == VM_TV) d = 0.5f * r;
      else d = r / (float)n;
      float w = exp_r(-h.alpha * d);
      w = w < 0.0f ? 0.0f : (w > 1.0f ? 1.0f : w);   // np.clip: a NaN stays a NaN
      const float ca = w * h.nmix, cb = 1.0f - w;
      float u[PER];
      double su = 0.0;
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        u[j] = ca * cur[j] + cb * prev[j];
        su += ok[j] ? (double)u[j] : 0.0;
      }
      const float suf = (float)block_sum256_d(su, shr[1]);
      double sp = 0.0;
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        u[j] = u[j] / suf;
        sp += ok[j] ? (double)u[j] : 0.0;
      }
#pragma unroll
      for (int j = 0; j < PER; ++j)
        if (ok[j]) o[j] = u[j];
      const float spn = (float)block_sum256_d(sp, shr[2]);
      if (tid == 0) h.dist[row] = d;
      if (pos_finite(suf) && pos_finite(spn)) {
#pragma unroll
        for (int j = 0; j < PER; ++j) prev[j] = ok[j] ? u[j] : 0.0f;
        spf = spn;
      }
    }
  }
  if (have) {
#pragma unroll
    for (int j = 0; j < PER; ++j)
      if (ok[j]) h.state[(size_t)s * n + i0 + j] = prev[j];
    if (tid == 0) {
      h.state_sum[s] = spf;
      h.have[s] = 1;
    }
  }
}

// ------------------------------------------------------------------------------------------ pole continuity
__device__ __forceinline__ float dot4(const float4 a, const float4 b) {
  return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w);
}

// Thread idx: stream idx % S of the video (idx / S == 1) or still (0) quaternions. The first finite quaternion
// after a reset sets the pole; later ones are negated when their dot product with the pole is negative, and move
// the pole only when |dot| > 0.5 (an outlier, or a NaN, does not).
__global__ void video_pole_kernel(float* quat_video, float* quat_still, float* poles, int* pole_have, int T, int S) {
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= 2 * S) return;
  const int s = idx % S, which = idx / S;
  float4* q = reinterpret_cast<float4*>(which ? quat_video : quat_still);
  if (!q) return;
  float4* pp = reinterpret_cast<float4*>(poles) + (size_t)which * S + s;
  int have = pole_have[which * S + s];
  float4 pole = have ? *pp : make_float4(0.f, 0.f, 0.f, 0.f);
  for (int t0 = 0; t0 < T; t0 += 8) {   // 8 loads in flight, then the sequential rule
    float4 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (t0 + k < T) v[k] = q[(size_t)(t0 + k) * S + s];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (t0 + k >= T) break;
      if (!have) {
        if (dot4(v[k], v[k]) > 0.5f) {
          pole = v[k];
          have = 1;
        }
        continue;
      }
      const float dot = dot4(pole, v[k]);
      if (dot < 0.0f) {
        v[k] = make_float4(-v[k].x, -v[k].y, -v[k].z, -v[k].w);
        q[(size_t)(t0 + k) * S + s] = v[k];
      }
      if (fabsf(dot) > 0.5f) pole = v[k];
    }
  }
  if (have) {
    *pp = pole;
    pole_have[which * S + s] = 1;
  }
}

__global__ void video_reset_kernel(int* flags, int S, int stream) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= 4 * S) return;
  if (stream < 0 || idx % S == stream) flags[idx] = 0;
}

// Blocks 0 / 1: the ori / pos PDF of `stream` (bins in the scan kernel's thread order, its sum in the same order);
// block 2: both poles.
__global__ __launch_bounds__(256) void video_set_state_kernel(const VideoHead h0, const VideoHead h1, float* poles,
                                                              int* pole_have, int S, int stream, const float* ori_pdf,
                                                              const float* pos_pdf, const float* still_pole,
                                                              const float* video_pole) {
  __shared__ double sh[4];
  const int tid = threadIdx.x;
  if (blockIdx.x == 2) {
    if (tid < 8) {
      const int which = tid >> 2, k = tid & 3;
      const float* src = which ? video_pole : still_pole;
      if (src) poles[((size_t)which * S + stream) * 4 + k] = src[k];
      if (k == 0) pole_have[which * S + stream] = src ? 1 : 0;
    }
    return;
  }
  const VideoHead h = blockIdx.x ? h1 : h0;
  const float* src = blockIdx.x ? pos_pdf : ori_pdf;
  if (!src) {
    if (tid == 0) h.have[stream] = 0;
    return;
  }
  const int n = h.n, per = (n + 255) >> 8, i0 = tid * per;
  double a = 0.0;
  for (int j = 0; j < per; ++j)
    if (i0 + j < n) {
      const float v = src[i0 + j];
      h.state[(size_t)stream * n + i0 + j] = v;
      a += (double)v;
    }
  const float sum = (float)block_sum256_d(a, sh);
  if (tid == 0) {
    h.state_sum[stream] = sum;
    h.have[stream] = 1;
  }
}

// ------------------------------------------------------------------------------------------ launchers
hipError_t launch_video_scan(const VideoHead& ori, const VideoHead& pos, int T, int S, int metric, hipStream_t s) {
  const int n = ori.n > pos.n ? ori.n : pos.n;
  if (n > 256 * 32 || ori.n < 1 || pos.n < 1 || T < 1 || S < 1) return hipErrorInvalidValue;
  const dim3 grid(S, 2);
#define SPEF_VIDEO_SCAN(M)                                                                \
  case M:                                                                                 \
    if (n <= 256 * 8) video_scan_kernel<8, M><<<grid, 256, 0, s>>>(ori, pos, T, S);       \
    else video_scan_kernel<32, M><<<grid, 256, 0, s>>>(ori, pos, T, S);                   \
    break;
  switch (metric) {
    SPEF_VIDEO_SCAN(VM_L2)
    SPEF_VIDEO_SCAN(VM_KL)
    SPEF_VIDEO_SCAN(VM_JS)
    SPEF_VIDEO_SCAN(VM_HELLINGER)
    SPEF_VIDEO_SCAN(VM_TV)
    SPEF_VIDEO_SCAN(VM_WASSERSTEIN)
    default: return hipErrorInvalidValue;
  }
#undef SPEF_VIDEO_SCAN
  return hipGetLastError();
}

hipError_t launch_video_pole(float* quat_video, float* quat_still, float* poles, int* pole_have, int T, int S,
                             hipStream_t s) {
  video_pole_kernel<<<(2 * S + 63) / 64, 64, 0, s>>>(quat_video, quat_still, poles, pole_have, T, S);
  return hipGetLastError();
}

hipError_t launch_video_reset(int* flags, int S, int stream, hipStream_t s) {
  video_reset_kernel<<<(4 * S + 255) / 256, 256, 0, s>>>(flags, S, stream);
  return hipGetLastError();
}

hipError_t launch_video_set_state(const VideoHead& ori, const VideoHead& pos, float* poles, int* pole_have, int S,
                                  int stream, const float* ori_pdf, const float* pos_pdf, const float* still_pole,
                                  const float* video_pole, hipStream_t s) {
  video_set_state_kernel<<<3, 256, 0, s>>>(ori, pos, poles, pole_have, S, stream, ori_pdf, pos_pdf, still_pole,
                                           video_pole);
  return hipGetLastError();
}

}  // namespace spef
