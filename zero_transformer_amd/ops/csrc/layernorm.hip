// Bias-free LayerNorm forward + backward for gfx950.
// Replaces the XLA-fused LayerNorm of the reference (GPT.py:42,49,98 — 49
// calls/step at 1.3B). Memory-bound: the bf16 fast path is fully vectorized
// (s16x8 loads, G13), keeps the row in registers (one read + one write per
// tensor), and accumulates dw in per-thread registers across the row loop
// (columns are thread-owned), with one atomic pass at kernel end.
// fp32 statistics throughout.

#include "common.h"

#include <hip/hip_fp16.h>

#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

namespace {

// ---------------------------------------------------------------------------
// Fast path: bf16, C % 8 == 0, one s16x8 per thread (C/8 <= 1024). The whole
// row lives in registers. The block is C/8 rounded up to whole waves: the
// reductions (block_reduce_sum, the joint reduce in ln_bwd_vec) count
// blockDim.x / WAVE waves and run a 64-wide butterfly, so a trailing partial
// wave would be dropped from every row statistic. PARTIAL instances carry the
// extra lanes (t * 8 >= C): they load nothing, contribute 0 and store nothing.
// PARTIAL = false (C % 512 == 0) compiles to the unpredicated kernel.
// ---------------------------------------------------------------------------
template <bool PARTIAL>
__global__ __launch_bounds__(1024) void ln_fwd_vec(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ w,
    uint16_t* __restrict__ y, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, long rows, int C, float eps) {
  __shared__ float scratch[16];
  const int t = threadIdx.x;
  const bool live = !PARTIAL || t * 8 < C;
  float wv[8];
  {
    s16x8 w8 = {};
    if (live) w8 = *reinterpret_cast<const s16x8*>(&w[t * 8]);
#pragma unroll
    for (int e = 0; e < 8; ++e) wv[e] = bf16_to_f32((uint16_t)w8[e]);
  }
  const float invC = 1.0f / (float)C;
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    s16x8 x8 = {};
    if (live) x8 = *reinterpret_cast<const s16x8*>(&x[row * C + t * 8]);
    float xv[8];
    float sum = 0.f, sumsq = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      xv[e] = bf16_to_f32((uint16_t)x8[e]);
      sum += xv[e];
      sumsq += xv[e] * xv[e];
    }
    sum = block_reduce_sum(sum, scratch);
    sumsq = block_reduce_sum(sumsq, scratch);
    const float mu = sum * invC;
    const float rstd = rsqrtf(sumsq * invC - mu * mu + eps);
    if (t == 0) {
      mean_out[row] = mu;
      rstd_out[row] = rstd;
    }
    s16x8 y8;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      y8[e] = (short)f32_to_bf16((xv[e] - mu) * rstd * wv[e]);
    if (live) *reinterpret_cast<s16x8*>(&y[row * C + t * 8]) = y8;
  }
}

// dx = rstd * (g - mean(g) - xhat * mean(g*xhat)),  g = w * dy
// dw[c] = sum_rows dy[r,c] * xhat[r,c]  — thread-owned columns, register
// accumulation across the row loop; per-block partial rows written to
// dw_part[block][C] (no atomics — an atomic tail at grid 2048 was 4.2M
// atomicAdds onto 2048 words and dominated the kernel), reduced by
// ln_dw_reduce. The two row statistics reduce together (one barrier set).
template <bool PARTIAL>
__global__ __launch_bounds__(1024) void ln_bwd_vec(
    const uint16_t* __restrict__ dy, const uint16_t* __restrict__ x,
    const uint16_t* __restrict__ w, const float* __restrict__ mean,
    const float* __restrict__ rstd, uint16_t* __restrict__ dx,
    float* __restrict__ dw_part, long rows, int C) {
  __shared__ float scratch[32];
  const int t = threadIdx.x;
  const bool live = !PARTIAL || t * 8 < C;
  float wv[8], dw_acc[8];
  {
    s16x8 w8 = {};
    if (live) w8 = *reinterpret_cast<const s16x8*>(&w[t * 8]);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      wv[e] = bf16_to_f32((uint16_t)w8[e]);
      dw_acc[e] = 0.f;
    }
  }
  const float invC = 1.0f / (float)C;
  const int lane = t & (WAVE - 1), wid = t / WAVE, nw = blockDim.x / WAVE;
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    s16x8 dy8 = {}, x8 = {};
    if (live) {
      dy8 = *reinterpret_cast<const s16x8*>(&dy[row * C + t * 8]);
      x8 = *reinterpret_cast<const s16x8*>(&x[row * C + t * 8]);
    }
    const float mu = mean[row], rs = rstd[row];
    float g[8], xh[8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float d = bf16_to_f32((uint16_t)dy8[e]);
      xh[e] = (bf16_to_f32((uint16_t)x8[e]) - mu) * rs;
      g[e] = d * wv[e];
      s1 += g[e];
      s2 += g[e] * xh[e];
      dw_acc[e] += d * xh[e];
    }
    // joint block reduce of (s1, s2): one LDS round instead of two
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      s1 += __shfl_xor(s1, off, WAVE);
      s2 += __shfl_xor(s2, off, WAVE);
    }
    if (lane == 0) {
      scratch[wid] = s1;
      scratch[16 + wid] = s2;
    }
    __syncthreads();
    s1 = 0.f;
    s2 = 0.f;
    for (int i = 0; i < nw; ++i) {
      s1 += scratch[i];
      s2 += scratch[16 + i];
    }
    __syncthreads();
    s1 *= invC;
    s2 *= invC;
    s16x8 dx8;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      dx8[e] = (short)f32_to_bf16((g[e] - s1 - xh[e] * s2) * rs);
    if (live) *reinterpret_cast<s16x8*>(&dx[row * C + t * 8]) = dx8;
  }
  if (!live) return;
  f32x4 p0 = {dw_acc[0], dw_acc[1], dw_acc[2], dw_acc[3]};
  f32x4 p1 = {dw_acc[4], dw_acc[5], dw_acc[6], dw_acc[7]};
  *reinterpret_cast<f32x4*>(&dw_part[(long)blockIdx.x * C + t * 8]) = p0;
  *reinterpret_cast<f32x4*>(&dw_part[(long)blockIdx.x * C + t * 8 + 4]) = p1;
}

// grid (C/256, NSPLIT): y-block sums its slice of partial rows, one
// atomicAdd per column per slice (C*NSPLIT atomics total — negligible).
__global__ void ln_dw_reduce(const float* __restrict__ dw_part,
                             float* __restrict__ dw, int C, int npart) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const int per = (npart + gridDim.y - 1) / gridDim.y;
  const int b0 = blockIdx.y * per;
  const int b1 = min(npart, b0 + per);
  float s = 0.f;
  for (int b = b0; b < b1; ++b) s += dw_part[(long)b * C + c];
  atomicAdd(&dw[c], s);
}

// ---------------------------------------------------------------------------
// Generic fallback (any dtype / any C)
// ---------------------------------------------------------------------------
template <typename T>
__global__ void ln_fwd_kernel(const T* __restrict__ x, const T* __restrict__ w,
                              T* __restrict__ y, float* __restrict__ mean_out,
                              float* __restrict__ rstd_out, long rows, int C,
                              float eps) {
  __shared__ float scratch[16];
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    const T* xr = x + row * C;
    T* yr = y + row * C;
    float sum = 0.f, sumsq = 0.f;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      float v = to_f32(xr[c]);
      sum += v;
      sumsq += v * v;
    }
    sum = block_reduce_sum(sum, scratch);
    sumsq = block_reduce_sum(sumsq, scratch);
    float mu = sum / C;
    float var = sumsq / C - mu * mu;
    float rstd = rsqrtf(var + eps);
    if (threadIdx.x == 0) {
      mean_out[row] = mu;
      rstd_out[row] = rstd;
    }
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      float v = (to_f32(xr[c]) - mu) * rstd * to_f32(w[c]);
      yr[c] = from_f32<T>(v);
    }
  }
}

template <typename T>
__global__ void ln_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                              const T* __restrict__ w, const float* __restrict__ mean,
                              const float* __restrict__ rstd, T* __restrict__ dx,
                              float* __restrict__ dw_f32, long rows, int C) {
  extern __shared__ float smem[];  // [C] dw accumulator + 16 scratch
  float* dw_local = smem;
  float* scratch = smem + C;
  for (int c = threadIdx.x; c < C; c += blockDim.x) dw_local[c] = 0.f;
  __syncthreads();

  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    const T* dyr = dy + row * C;
    const T* xr = x + row * C;
    T* dxr = dx + row * C;
    const float mu = mean[row], rs = rstd[row];
    float s1 = 0.f, s2 = 0.f;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      float g = to_f32(dyr[c]) * to_f32(w[c]);
      float xh = (to_f32(xr[c]) - mu) * rs;
      s1 += g;
      s2 += g * xh;
    }
    s1 = block_reduce_sum(s1, scratch) / C;
    s2 = block_reduce_sum(s2, scratch) / C;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      float g = to_f32(dyr[c]) * to_f32(w[c]);
      float xh = (to_f32(xr[c]) - mu) * rs;
      dxr[c] = from_f32<T>((g - s1 - xh * s2) * rs);
      dw_local[c] += to_f32(dyr[c]) * xh;
    }
    __syncthreads();
  }
  for (int c = threadIdx.x; c < C; c += blockDim.x)
    atomicAdd(&dw_f32[c], dw_local[c]);
}

// ---------------------------------------------------------------------------
// Fused residual-add + LayerNorm for the DECODE step (inference only):
//   y = x + h;  ln = LN(y) * w
// One kernel instead of an elementwise add + torch LN (each ~4.5 us of
// pure launch/latency at decode's (B, 1, C) rows — 4 such pairs/layer were
// ~0.45 ms of the 2.3 ms/token budget). fp16/bf16, one workgroup per row.
// ---------------------------------------------------------------------------
template <bool F16, bool PARTIAL>
__global__ __launch_bounds__(1024) void add_ln_vec(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ h,
    const uint16_t* __restrict__ w, uint16_t* __restrict__ y,
    uint16_t* __restrict__ ln, long rows, int C, float eps) {
  __shared__ float scratch[16];
  const int t = threadIdx.x;
  auto cvt = [](uint16_t u) {
    if (F16) {
      __half hv = *reinterpret_cast<__half*>(&u);
      return __half2float(hv);
    }
    return bf16_to_f32(u);
  };
  auto enc = [](float f) -> uint16_t {
    if (F16) {
      __half hv = __float2half(f);
      return *reinterpret_cast<uint16_t*>(&hv);
    }
    return f32_to_bf16(f);
  };
  const bool live = !PARTIAL || t * 8 < C;
  float wv[8];
  {
    s16x8 w8 = {};
    if (live) w8 = *reinterpret_cast<const s16x8*>(&w[t * 8]);
#pragma unroll
    for (int e = 0; e < 8; ++e) wv[e] = cvt((uint16_t)w8[e]);
  }
  const float invC = 1.0f / (float)C;
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    s16x8 x8 = {}, h8 = {};
    if (live) {
      x8 = *reinterpret_cast<const s16x8*>(&x[row * C + t * 8]);
      h8 = *reinterpret_cast<const s16x8*>(&h[row * C + t * 8]);
    }
    float v[8];
    float sum = 0.f, sumsq = 0.f;
    s16x8 y8;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      v[e] = cvt((uint16_t)x8[e]) + cvt((uint16_t)h8[e]);
      y8[e] = (short)enc(v[e]);
      sum += v[e];
      sumsq += v[e] * v[e];
    }
    if (live) *reinterpret_cast<s16x8*>(&y[row * C + t * 8]) = y8;
    sum = block_reduce_sum(sum, scratch);
    sumsq = block_reduce_sum(sumsq, scratch);
    const float mu = sum * invC;
    const float rstd = rsqrtf(sumsq * invC - mu * mu + eps);
    s16x8 l8;
#pragma unroll
    for (int e = 0; e < 8; ++e) l8[e] = (short)enc((v[e] - mu) * rstd * wv[e]);
    if (live) *reinterpret_cast<s16x8*>(&ln[row * C + t * 8]) = l8;
  }
}

// ---------------------------------------------------------------------------
// Fused residual-add + dropout + LayerNorm for TRAINING (bf16 vector path):
//   x' = x + dropout(h, p);  y = LN(x') * w
// res_drop_fwd followed by ln_fwd_vec is 5 passes over one activation
// (read x, h, write x'; read x', write y); here 4. The mask is the one of
// residual.hip (rd_bits on the flat element index; a thread's 8 elements
// start at a multiple of 8). x' is rounded to bf16 before the statistics,
// and the statistics and y repeat ln_fwd_vec's arithmetic on the rounded
// value, so x', y, mean, rstd carry the bits of the two-kernel chain.
// DROP = false (p == 0 / eval): no hash, x' = bf16(x + h).
// ---------------------------------------------------------------------------
template <bool PARTIAL, bool DROP>
__global__ __launch_bounds__(1024) void res_ln_fwd_vec(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ h,
    const uint16_t* __restrict__ w, uint16_t* __restrict__ xp,
    uint16_t* __restrict__ y, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, long rows, int C, float eps, uint32_t thr,
    float inv_keep, uint32_t seed) {
  __shared__ float scratch[16];
  const int t = threadIdx.x;
  const bool live = !PARTIAL || t * 8 < C;
  float wv[8];
  {
    s16x8 w8 = {};
    if (live) w8 = *reinterpret_cast<const s16x8*>(&w[t * 8]);
#pragma unroll
    for (int e = 0; e < 8; ++e) wv[e] = bf16_to_f32((uint16_t)w8[e]);
  }
  const float invC = 1.0f / (float)C;
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    const long i = row * C + t * 8;
    s16x8 x8 = {}, h8 = {};
    if (live) {
      x8 = *reinterpret_cast<const s16x8*>(&x[i]);
      h8 = *reinterpret_cast<const s16x8*>(&h[i]);
    }
    uint32_t b0 = 0, b1 = 0;
    if (DROP) {
      b0 = rd_bits(seed, i >> 2);
      b1 = rd_bits(seed, (i >> 2) + 1);
    }
    s16x8 p8;
    float xv[8];
    float sum = 0.f, sumsq = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float hv = bf16_to_f32((uint16_t)h8[e]);
      if (DROP) {
        const uint32_t bits = e < 4 ? b0 : b1;
        const bool keep = ((bits >> (8 * (e & 3))) & 0xffu) >= thr;
        hv = keep ? hv * inv_keep : 0.f;
      }
      const uint16_t r = f32_to_bf16(bf16_to_f32((uint16_t)x8[e]) + hv);
      p8[e] = (short)r;
      xv[e] = bf16_to_f32(r);
      sum += xv[e];
      sumsq += xv[e] * xv[e];
    }
    if (live) *reinterpret_cast<s16x8*>(&xp[i]) = p8;
    sum = block_reduce_sum(sum, scratch);
    sumsq = block_reduce_sum(sumsq, scratch);
    const float mu = sum * invC;
    const float rstd = rsqrtf(sumsq * invC - mu * mu + eps);
    if (t == 0) {
      mean_out[row] = mu;
      rstd_out[row] = rstd;
    }
    s16x8 y8;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      y8[e] = (short)f32_to_bf16((xv[e] - mu) * rstd * wv[e]);
    if (live) *reinterpret_cast<s16x8*>(&y[i]) = y8;
  }
}

// Backward of the above, and of the residual add that consumed x':
//   g  = bf16(d(x') + bf16(LN-dx))   gradient of x (and of x' upstream)
//   dh = mask(g) * inv_keep          as res_drop_bwd
// ln_bwd_vec + torch add + res_drop_bwd is 8 passes (3 + 3 + 2); here 5
// (read dy, x', d(x'); write g, dh). Rounds where the chain rounds (LN-dx,
// the sum, dh from the rounded sum), so g and dh carry its bits; dw_part
// has ln_bwd_vec's layout and goes through ln_dw_reduce. HAS_DXP = false:
// nothing arrives down the residual stream (final norm), g = bf16(LN-dx).
// DROP = false: dh is g, nothing further is written.
template <bool PARTIAL, bool HAS_DXP, bool DROP>
__global__ __launch_bounds__(1024) void res_ln_bwd_vec(
    const uint16_t* __restrict__ dy, const uint16_t* __restrict__ xp,
    const uint16_t* __restrict__ w, const float* __restrict__ mean,
    const float* __restrict__ rstd, const uint16_t* __restrict__ dxp,
    uint16_t* __restrict__ g_out, uint16_t* __restrict__ dh,
    float* __restrict__ dw_part, long rows, int C, uint32_t thr, float inv_keep,
    uint32_t seed) {
  __shared__ float scratch[32];
  const int t = threadIdx.x;
  const bool live = !PARTIAL || t * 8 < C;
  float wv[8], dw_acc[8];
  {
    s16x8 w8 = {};
    if (live) w8 = *reinterpret_cast<const s16x8*>(&w[t * 8]);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      wv[e] = bf16_to_f32((uint16_t)w8[e]);
      dw_acc[e] = 0.f;
    }
  }
  const float invC = 1.0f / (float)C;
  const int lane = t & (WAVE - 1), wid = t / WAVE, nw = blockDim.x / WAVE;
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    const long i = row * C + t * 8;
    s16x8 dy8 = {}, x8 = {}, r8 = {};
    if (live) {
      dy8 = *reinterpret_cast<const s16x8*>(&dy[i]);
      x8 = *reinterpret_cast<const s16x8*>(&xp[i]);
      if (HAS_DXP) r8 = *reinterpret_cast<const s16x8*>(&dxp[i]);
    }
    const float mu = mean[row], rs = rstd[row];
    float g[8], xh[8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float d = bf16_to_f32((uint16_t)dy8[e]);
      xh[e] = (bf16_to_f32((uint16_t)x8[e]) - mu) * rs;
      g[e] = d * wv[e];
      s1 += g[e];
      s2 += g[e] * xh[e];
      dw_acc[e] += d * xh[e];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      s1 += __shfl_xor(s1, off, WAVE);
      s2 += __shfl_xor(s2, off, WAVE);
    }
    if (lane == 0) {
      scratch[wid] = s1;
      scratch[16 + wid] = s2;
    }
    __syncthreads();
    s1 = 0.f;
    s2 = 0.f;
    for (int k = 0; k < nw; ++k) {
      s1 += scratch[k];
      s2 += scratch[16 + k];
    }
    __syncthreads();
    s1 *= invC;
    s2 *= invC;
    uint32_t b0 = 0, b1 = 0;
    if (DROP) {
      b0 = rd_bits(seed, i >> 2);
      b1 = rd_bits(seed, (i >> 2) + 1);
    }
    s16x8 g8, h8;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      uint16_t r = f32_to_bf16((g[e] - s1 - xh[e] * s2) * rs);
      if (HAS_DXP) r = f32_to_bf16(bf16_to_f32((uint16_t)r8[e]) + bf16_to_f32(r));
      g8[e] = (short)r;
      if (DROP) {
        const uint32_t bits = e < 4 ? b0 : b1;
        const bool keep = ((bits >> (8 * (e & 3))) & 0xffu) >= thr;
        h8[e] = keep ? (short)f32_to_bf16(bf16_to_f32(r) * inv_keep) : (short)0;
      }
    }
    if (live) {
      *reinterpret_cast<s16x8*>(&g_out[i]) = g8;
      if (DROP) *reinterpret_cast<s16x8*>(&dh[i]) = h8;
    }
  }
  if (!live) return;
  f32x4 p0 = {dw_acc[0], dw_acc[1], dw_acc[2], dw_acc[3]};
  f32x4 p1 = {dw_acc[4], dw_acc[5], dw_acc[6], dw_acc[7]};
  *reinterpret_cast<f32x4*>(&dw_part[(long)blockIdx.x * C + t * 8]) = p0;
  *reinterpret_cast<f32x4*>(&dw_part[(long)blockIdx.x * C + t * 8 + 4]) = p1;
}

// Vector-path block: one thread per 8 columns, rounded up to whole waves.
inline int vec_block(int C) { return (C / 8 + WAVE - 1) / WAVE * WAVE; }

}  // namespace

// y = x + h and ln = LayerNorm(y) * w in one pass (decode path; no grads).
std::vector<at::Tensor> add_ln_fwd(at::Tensor x, at::Tensor h, at::Tensor w,
                                   double eps) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && h.is_contiguous() &&
              w.is_contiguous());
  TORCH_CHECK(x.scalar_type() == at::kHalf || x.scalar_type() == at::kBFloat16);
  TORCH_CHECK(x.sizes() == h.sizes() && x.scalar_type() == h.scalar_type());
  const int C = x.size(-1);
  TORCH_CHECK(C % 8 == 0 && C / 8 >= 64 && C / 8 <= 1024 && w.numel() == C,
              "add_ln: C/8 must be in [64, 1024]");
  const long rows = x.numel() / C;
  auto y = at::empty_like(x);
  auto ln = at::empty_like(x);
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const int block = vec_block(C);
  const bool partial = block * 8 != C;
  const int grid = int(std::min<long>(rows, 4096));
#define ZTA_ADD_LN(F16V, PARTIALV)                                                 \
  hipLaunchKernelGGL((add_ln_vec<F16V, PARTIALV>), dim3(grid), dim3(block), 0,     \
                     stream, (const uint16_t*)x.data_ptr(),                        \
                     (const uint16_t*)h.data_ptr(), (const uint16_t*)w.data_ptr(), \
                     (uint16_t*)y.data_ptr(), (uint16_t*)ln.data_ptr(), rows, C,   \
                     (float)eps)
  if (x.scalar_type() == at::kHalf) {
    if (partial) ZTA_ADD_LN(true, true);
    else ZTA_ADD_LN(true, false);
  } else {
    if (partial) ZTA_ADD_LN(false, true);
    else ZTA_ADD_LN(false, false);
  }
#undef ZTA_ADD_LN
  return {y, ln};
}

std::vector<at::Tensor> layernorm_fwd(at::Tensor x, at::Tensor w, double eps) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous());
  TORCH_CHECK(w.is_contiguous() && w.dim() == 1);
  const int C = x.size(-1);
  const long rows = x.numel() / C;
  auto y = at::empty_like(x);
  auto mean = at::empty({rows}, x.options().dtype(at::kFloat));
  auto rstd = at::empty({rows}, x.options().dtype(at::kFloat));
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const bool vec = x.scalar_type() == at::kBFloat16 && C % 8 == 0 && C / 8 >= 64 &&
                   C / 8 <= 1024;
  if (vec) {
    const int block = vec_block(C);
    const int grid = int(std::min<long>(rows, 4096));
#define ZTA_LN_FWD(PARTIALV)                                                      \
  hipLaunchKernelGGL(ln_fwd_vec<PARTIALV>, dim3(grid), dim3(block), 0, stream,    \
                     (const uint16_t*)x.data_ptr(), (const uint16_t*)w.data_ptr(), \
                     (uint16_t*)y.data_ptr(), mean.data_ptr<float>(),             \
                     rstd.data_ptr<float>(), rows, C, (float)eps)
    if (block * 8 != C) ZTA_LN_FWD(true);
    else ZTA_LN_FWD(false);
#undef ZTA_LN_FWD
  } else if (x.scalar_type() == at::kBFloat16) {
    hipLaunchKernelGGL(ln_fwd_kernel<uint16_t>, dim3(int(std::min<long>(rows, 2048))),
                       dim3(256), 0, stream, (const uint16_t*)x.data_ptr(),
                       (const uint16_t*)w.data_ptr(), (uint16_t*)y.data_ptr(),
                       mean.data_ptr<float>(), rstd.data_ptr<float>(), rows, C, (float)eps);
  } else if (x.scalar_type() == at::kFloat) {
    hipLaunchKernelGGL(ln_fwd_kernel<float>, dim3(int(std::min<long>(rows, 2048))),
                       dim3(256), 0, stream, x.data_ptr<float>(), w.data_ptr<float>(),
                       y.data_ptr<float>(), mean.data_ptr<float>(), rstd.data_ptr<float>(),
                       rows, C, (float)eps);
  } else {
    TORCH_CHECK(false, "layernorm: unsupported dtype");
  }
  return {y, rstd, mean};
}

std::vector<at::Tensor> layernorm_bwd(at::Tensor dy, at::Tensor x, at::Tensor w,
                                      at::Tensor rstd, at::Tensor mean) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && dy.is_contiguous() &&
              w.is_contiguous());
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kFloat,
              "layernorm: unsupported dtype");
  TORCH_CHECK(dy.scalar_type() == x.scalar_type() && w.scalar_type() == x.scalar_type());
  const int C = x.size(-1);
  const long rows = x.numel() / C;
  auto dx = at::empty_like(x);
  auto dw_f32 = at::zeros({C}, x.options().dtype(at::kFloat));
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const bool vec = x.scalar_type() == at::kBFloat16 && C % 8 == 0 && C / 8 >= 64 &&
                   C / 8 <= 1024;
  if (vec) {
    const int block = vec_block(C);
    // 4096 blocks (16/CU): at 512 the kernel was occupancy-bound (each CU
    // held only 2 x 256-thread blocks walking 64 rows serially through
    // two barriers per row); 2048 measured 5.50 -> 4.05 ms/step at the
    // bench shape. dw_part grows to 32 MB at C=2048 — noise.
    const int grid = int(std::min<long>(rows, 4096));
    auto dw_part = at::empty({grid, C}, x.options().dtype(at::kFloat));
#define ZTA_LN_BWD(PARTIALV)                                                       \
  hipLaunchKernelGGL(ln_bwd_vec<PARTIALV>, dim3(grid), dim3(block), 0, stream,     \
                     (const uint16_t*)dy.data_ptr(), (const uint16_t*)x.data_ptr(), \
                     (const uint16_t*)w.data_ptr(), mean.data_ptr<float>(),        \
                     rstd.data_ptr<float>(), (uint16_t*)dx.data_ptr(),             \
                     dw_part.data_ptr<float>(), rows, C)
    if (block * 8 != C) ZTA_LN_BWD(true);
    else ZTA_LN_BWD(false);
#undef ZTA_LN_BWD
    hipLaunchKernelGGL(ln_dw_reduce, dim3((C + 255) / 256, 64), dim3(256), 0, stream,
                       dw_part.data_ptr<float>(), dw_f32.data_ptr<float>(), C, grid);
  } else {
    const int block = 256;
    const int grid = int(std::min<long>(rows, 1024));
    const size_t smem = ((size_t)C + 16) * sizeof(float);
    // the launch itself is unchecked: an over-limit LDS request would fail
    // silently and hand back uninitialised dx
    const size_t lds_max = at::cuda::getCurrentDeviceProperties()->sharedMemPerBlock;
    TORCH_CHECK(smem <= lds_max, "layernorm_bwd: C=", C, " needs ", smem,
                " bytes of LDS for the dw accumulator, device limit is ", lds_max);
    if (x.scalar_type() == at::kBFloat16) {
      hipLaunchKernelGGL(ln_bwd_kernel<uint16_t>, dim3(grid), dim3(block), smem, stream,
                         (const uint16_t*)dy.data_ptr(), (const uint16_t*)x.data_ptr(),
                         (const uint16_t*)w.data_ptr(), mean.data_ptr<float>(),
                         rstd.data_ptr<float>(), (uint16_t*)dx.data_ptr(),
                         dw_f32.data_ptr<float>(), rows, C);
    } else {
      hipLaunchKernelGGL(ln_bwd_kernel<float>, dim3(grid), dim3(block), smem, stream,
                         dy.data_ptr<float>(), x.data_ptr<float>(), w.data_ptr<float>(),
                         mean.data_ptr<float>(), rstd.data_ptr<float>(), dx.data_ptr<float>(),
                         dw_f32.data_ptr<float>(), rows, C);
    }
  }
  return {dx, dw_f32.to(x.scalar_type())};
}

namespace {

// thr / inv_keep of residual.hip
inline uint32_t drop_thr(double p) { return (uint32_t)(p * 256.0 + 0.5); }
inline float drop_inv_keep(uint32_t thr) {
  return thr ? 256.0f / (256.0f - (float)thr) : 1.0f;
}

void check_res_ln(const at::Tensor& a, const at::Tensor& w, const char* what) {
  TORCH_CHECK(a.is_cuda() && a.is_contiguous() && w.is_contiguous() && w.dim() == 1,
              what, ": contiguous device tensors");
  TORCH_CHECK(a.scalar_type() == at::kBFloat16 && w.scalar_type() == at::kBFloat16,
              what, ": bf16 only");
  const long C = a.size(-1);
  TORCH_CHECK(C % 8 == 0 && C / 8 >= 64 && C / 8 <= 1024 && w.numel() == C, what,
              ": C/8 must be in [64, 1024]");
}

}  // namespace

// x' = x + dropout(h, p), y = LayerNorm(x') * w  ->  {x', y, rstd, mean}
std::vector<at::Tensor> residual_ln_fwd(at::Tensor x, at::Tensor h, at::Tensor w,
                                        double p, int64_t seed, double eps) {
  check_res_ln(x, w, "residual_ln_fwd");
  TORCH_CHECK(h.is_cuda() && h.is_contiguous() && h.scalar_type() == at::kBFloat16 &&
              h.sizes() == x.sizes());
  const int C = x.size(-1);
  const long rows = x.numel() / C;
  auto xp = at::empty_like(x);
  auto y = at::empty_like(x);
  auto mean = at::empty({rows}, x.options().dtype(at::kFloat));
  auto rstd = at::empty({rows}, x.options().dtype(at::kFloat));
  if (rows == 0) return {xp, y, rstd, mean};
  const uint32_t thr = drop_thr(p);
  const float inv_keep = drop_inv_keep(thr);
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const int block = vec_block(C);
  const int grid = int(std::min<long>(rows, 4096));
#define ZTA_RES_LN_FWD(PARTIALV, DROPV)                                              \
  hipLaunchKernelGGL((res_ln_fwd_vec<PARTIALV, DROPV>), dim3(grid), dim3(block), 0,  \
                     stream, (const uint16_t*)x.data_ptr(),                          \
                     (const uint16_t*)h.data_ptr(), (const uint16_t*)w.data_ptr(),   \
                     (uint16_t*)xp.data_ptr(), (uint16_t*)y.data_ptr(),              \
                     mean.data_ptr<float>(), rstd.data_ptr<float>(), rows, C,        \
                     (float)eps, thr, inv_keep, (uint32_t)seed)
  const bool partial = block * 8 != C;
  if (thr) {
    if (partial) ZTA_RES_LN_FWD(true, true);
    else ZTA_RES_LN_FWD(false, true);
  } else {
    if (partial) ZTA_RES_LN_FWD(true, false);
    else ZTA_RES_LN_FWD(false, false);
  }
#undef ZTA_RES_LN_FWD
  return {xp, y, rstd, mean};
}

// -> {g, dh, dw}: g = d(x') + LN-dx (the gradient of x), dh = dropout-masked
// g (the same tensor as g when p == 0), dw of the LayerNorm weight. `dxp` is
// the gradient arriving at x' from further down the residual stream, absent
// when x' fed nothing but the LayerNorm.
std::vector<at::Tensor> residual_ln_bwd(at::Tensor dy, at::Tensor xp, at::Tensor w,
                                        at::Tensor rstd, at::Tensor mean,
                                        c10::optional<at::Tensor> dxp, double p,
                                        int64_t seed) {
  check_res_ln(xp, w, "residual_ln_bwd");
  TORCH_CHECK(dy.is_cuda() && dy.is_contiguous() && dy.scalar_type() == at::kBFloat16 &&
              dy.sizes() == xp.sizes());
  const int C = xp.size(-1);
  const long rows = xp.numel() / C;
  TORCH_CHECK(rstd.scalar_type() == at::kFloat && mean.scalar_type() == at::kFloat &&
              rstd.numel() == rows && mean.numel() == rows);
  const bool has = dxp.has_value() && dxp->defined();
  if (has)
    TORCH_CHECK(dxp->is_cuda() && dxp->is_contiguous() &&
                dxp->scalar_type() == at::kBFloat16 && dxp->sizes() == xp.sizes());
  const uint32_t thr = drop_thr(p);
  const float inv_keep = drop_inv_keep(thr);
  auto g = at::empty_like(xp);
  auto dh = thr ? at::empty_like(xp) : g;
  auto dw_f32 = at::zeros({C}, xp.options().dtype(at::kFloat));
  if (rows == 0) return {g, dh, dw_f32.to(xp.scalar_type())};
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const int block = vec_block(C);
  const int grid = int(std::min<long>(rows, 4096));  // as layernorm_bwd
  auto dw_part = at::empty({grid, C}, xp.options().dtype(at::kFloat));
  const uint16_t* dxp_ptr = has ? (const uint16_t*)dxp->data_ptr() : nullptr;
#define ZTA_RES_LN_BWD(PARTIALV, HASV, DROPV)                                         \
  hipLaunchKernelGGL((res_ln_bwd_vec<PARTIALV, HASV, DROPV>), dim3(grid),             \
                     dim3(block), 0, stream, (const uint16_t*)dy.data_ptr(),          \
                     (const uint16_t*)xp.data_ptr(), (const uint16_t*)w.data_ptr(),   \
                     mean.data_ptr<float>(), rstd.data_ptr<float>(), dxp_ptr,         \
                     (uint16_t*)g.data_ptr(), (uint16_t*)dh.data_ptr(),               \
                     dw_part.data_ptr<float>(), rows, C, thr, inv_keep,               \
                     (uint32_t)seed)
#define ZTA_RES_LN_BWD_P(HASV, DROPV)               \
  do {                                              \
    if (block * 8 != C) ZTA_RES_LN_BWD(true, HASV, DROPV); \
    else ZTA_RES_LN_BWD(false, HASV, DROPV);        \
  } while (0)
  if (has) {
    if (thr) ZTA_RES_LN_BWD_P(true, true);
    else ZTA_RES_LN_BWD_P(true, false);
  } else {
    if (thr) ZTA_RES_LN_BWD_P(false, true);
    else ZTA_RES_LN_BWD_P(false, false);
  }
#undef ZTA_RES_LN_BWD_P
#undef ZTA_RES_LN_BWD
  hipLaunchKernelGGL(ln_dw_reduce, dim3((C + 255) / 256, 64), dim3(256), 0, stream,
                     dw_part.data_ptr<float>(), dw_f32.data_ptr<float>(), C, grid);
  return {g, dh, dw_f32.to(xp.scalar_type())};
}
