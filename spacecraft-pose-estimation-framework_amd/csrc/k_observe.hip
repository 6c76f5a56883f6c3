// Histogram observers of the INT8 calibration path on gfx950 (Calibration path): the statistic
// of one activation-quantizer input, accumulated on the device over as many frames as the caller streams.
//
// The statistic of a float32 value x is keyed by b = bits(|x|) as uint32, so no range has to be known beforehand
// and every count is an integer that does not depend on launch geometry or on how the frames are cut into calls:
//   b >= 0x7f800000              non-finite             -> n_nonfinite (and nowhere else)
//   b <  103 << 23               |x| < 2^-24, zeros too -> n_under
//   b >= 135 << 23               |x| >= 2^8             -> n_over
//   otherwise                    bin (b - (103 << 23)) >> 15: 32 binades x 256 sub-bins, relative width <= 2^-8
//   max_bits                     max of b over the finite values (the integer order is the float order)
// A tap's record is OBS_COUNTERS + OBS_BINS uint64: n_total, n_under, n_over, n_nonfinite, max_bits, 0, 0, 0, then
// the bins (spef_amd.quant.observe_host is the NumPy twin).
//
//   observe_kernel<U8>   grid-stride over 16-byte loads (a scalar head up to the first 16-byte boundary and a scalar
//                        tail, so any n >= 1 and any element-aligned pointer work). The bins are privatised per
//                        workgroup in 32 KiB of LDS (uint32, non-returning ds_add_u32; five workgroups fit a CU's
//                        160 KiB). Underflow / overflow / non-finite counts and the max stay in registers and are
//                        reduced per wave: after a ReLU half of all values are zeros and would otherwise serialise on
//                        one LDS address. At the end only the non-zero LDS bins are flushed with 64-bit global atomic
//                        adds, the max with one integer atomic max per workgroup (the waves' maxima meet in the first
//                        words of the flushed LDS array). U8: uint8 pixels, value =
//                        (float)u / 255.0f (one correctly rounded fp32 division, as ToTensor computes it).
//   add_f32_kernel       y += x, one fp32 add per element (the residual join after an observed project conv: the same
//                        single add the GEMM's EPI_RES epilogue makes after the bias, k_f32.hip).
//   observe_reset_kernel zeroes records.
#include "spef_common.hpp"
#include "spef_kernels.hpp"

#pragma clang fp contract(off)

namespace spef {

namespace {

constexpr uint32_t OBS_LO = 103u << 23;   // 2^-24
constexpr uint32_t OBS_HI = 135u << 23;   // 2^8
// values per launch: below 2^32, so neither an LDS bin nor a thread's register count can wrap whatever the grid is
constexpr int64_t OBS_CHUNK = 1ll << 31;

struct ObsAcc {
  uint32_t under = 0, over = 0, nonfinite = 0, mx = 0;
};

__device__ __forceinline__ void obs_put(uint32_t bits, uint32_t* hist, ObsAcc& a) {
  const uint32_t b = bits & 0x7fffffffu;
  if (b >= 0x7f800000u) {
    ++a.nonfinite;
    return;
  }
  a.mx = b > a.mx ? b : a.mx;
  if (b < OBS_LO)
    ++a.under;
  else if (b >= OBS_HI)
    ++a.over;
  else
    atomicAdd(&hist[(b - OBS_LO) >> 15], 1u);   // result unused: ds_add_u32
}

__device__ __forceinline__ uint32_t u8_bits(uint32_t u) { return __float_as_uint((float)u / 255.0f); }

template <bool U8>
__global__ __launch_bounds__(256) void observe_kernel(unsigned long long* __restrict__ st,
                                                      const void* __restrict__ xv, int64_t n, int64_t head,
                                                      int64_t nvec) {
  __shared__ uint32_t hist[OBS_BINS];   // exactly 32 KiB: a word more and only four workgroups fit a CU
  const int tid = threadIdx.x;
  for (int k = tid; k < OBS_BINS; k += 256) hist[k] = 0;
  __syncthreads();

  ObsAcc a;
  constexpr int E = U8 ? 16 : 4;   // values per 16-byte load
  const uint8_t* xb = (const uint8_t*)xv;
  const uint32_t* xw = (const uint32_t*)xv;
  const uint4* body = U8 ? (const uint4*)(xb + head) : (const uint4*)(xw + head);
  auto put16 = [&](const uint4& q) {
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (U8) {
#pragma unroll
        for (int j = 0; j < 4; ++j) obs_put(u8_bits((w[e] >> (8 * j)) & 0xffu), hist, a);
      } else {
        obs_put(w[e], hist, a);
      }
    }
  };
  const int64_t step = (int64_t)gridDim.x * 256;
  int64_t v = (int64_t)blockIdx.x * 256 + tid;
  for (; v + 3 * step < nvec; v += 4 * step) {   // four 16-byte loads in flight per thread
    const uint4 q0 = body[v], q1 = body[v + step], q2 = body[v + 2 * step], q3 = body[v + 3 * step];
    put16(q0);
    put16(q1);
    put16(q2);
    put16(q3);
  }
  for (; v < nvec; v += step) put16(body[v]);
  if (blockIdx.x == 0) {   // scalar head and tail: fewer than E values each
    const int64_t t0 = head + nvec * E;
    if (tid < head) obs_put(U8 ? u8_bits(xb[tid]) : xw[tid], hist, a);
    if (t0 + tid < n) obs_put(U8 ? u8_bits(xb[t0 + tid]) : xw[t0 + tid], hist, a);
  }

#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    a.under += __shfl_xor(a.under, o);
    a.over += __shfl_xor(a.over, o);
    a.nonfinite += __shfl_xor(a.nonfinite, o);
    const uint32_t m = __shfl_xor(a.mx, o);
    a.mx = m > a.mx ? m : a.mx;
  }
  if ((tid & 63) == 0) {
    if (a.under) atomicAdd(&st[1], (unsigned long long)a.under);
    if (a.over) atomicAdd(&st[2], (unsigned long long)a.over);
    if (a.nonfinite) atomicAdd(&st[3], (unsigned long long)a.nonfinite);
  }
  __syncthreads();
  unsigned long long* bins = st + OBS_COUNTERS;
  for (int k = tid; k < OBS_BINS; k += 256) {
    const uint32_t c = hist[k];
    if (c) atomicAdd(&bins[k], (unsigned long long)c);
  }
  __syncthreads();   // the bins are flushed: their first words carry the four waves' maxima
  if ((tid & 63) == 0) hist[tid >> 6] = a.mx;
  __syncthreads();
  if (tid == 0) {
    uint32_t m = hist[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) m = hist[k] > m ? hist[k] : m;
    if (m) atomicMax(&st[4], (unsigned long long)m);
    if (blockIdx.x == 0) atomicAdd(&st[0], (unsigned long long)n);
  }
}

__global__ __launch_bounds__(256) void add_f32_kernel(float* __restrict__ y, const float* __restrict__ x, int64_t n4,
                                                      int64_t n) {
  const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  float4* y4 = reinterpret_cast<float4*>(y);
  const float4* x4 = reinterpret_cast<const float4*>(x);
  for (int64_t i = i0; i < n4; i += step) {
    float4 a = y4[i];
    const float4 b = x4[i];
    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    y4[i] = a;
  }
  for (int64_t i = 4 * n4 + i0; i < n; i += step) y[i] += x[i];
}

__global__ __launch_bounds__(256) void observe_reset_kernel(unsigned long long* __restrict__ st, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) st[i] = 0ull;
}

}  // namespace

hipError_t launch_observe(uint64_t* tap, const void* x, int64_t n, bool u8, int max_blocks, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int64_t es = u8 ? 1 : 4, E = u8 ? 16 : 4;
  if (max_blocks < 1) max_blocks = 1;
  for (int64_t off = 0; off < n; off += OBS_CHUNK) {   // OBS_CHUNK is a multiple of 16: every chunk keeps the alignment
    const int64_t m = n - off < OBS_CHUNK ? n - off : OBS_CHUNK;
    const uint8_t* p = (const uint8_t*)x + off * es;
    int64_t head = (int64_t)((16 - ((uintptr_t)p & 15)) & 15) / es;
    if (head > m) head = m;
    const int64_t nvec = (m - head) / E;
    int64_t grid = (nvec + 256 * 8 - 1) / (256 * 8);   // 8 loads per thread before another workgroup pays its flush
    grid = grid < 1 ? 1 : grid > max_blocks ? max_blocks : grid;
    unsigned long long* st = reinterpret_cast<unsigned long long*>(tap);
    if (u8)
      observe_kernel<true><<<(unsigned)grid, 256, 0, s>>>(st, p, m, head, nvec);
    else
      observe_kernel<false><<<(unsigned)grid, 256, 0, s>>>(st, p, m, head, nvec);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_add_f32(float* y, const float* x, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const bool al = (((uintptr_t)y | (uintptr_t)x) & 15) == 0;
  const int64_t n4 = al ? n / 4 : 0;
  int64_t grid = ((al ? n4 + 3 : n) + 255) / 256;
  grid = grid < 1 ? 1 : grid > (1 << 16) ? (1 << 16) : grid;
  add_f32_kernel<<<(unsigned)grid, 256, 0, s>>>(y, x, n4, n);
  return hipGetLastError();
}

hipError_t launch_observe_reset(uint64_t* st, int64_t n_words, hipStream_t s) {
  if (n_words <= 0) return hipSuccess;
  int64_t grid = (n_words + 255) / 256;
  grid = grid > 4096 ? 4096 : grid;
  observe_reset_kernel<<<(unsigned)grid, 256, 0, s>>>(reinterpret_cast<unsigned long long*>(st), n_words);
  return hipGetLastError();
}

}  // namespace spef
