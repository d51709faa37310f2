// Single-token (decode) causal ALiBi attention for gfx950: q (B, H, 1, D)
// against a KV cache k/v (B, H, S, D) -> out (B, H, 1, D).
//
// The training kernels tile MFMA over the T^2 score matrix; decode is a
// bandwidth-bound row problem (read the cache once), so this is a
// wave-per-key reduction split over the key range (split-S), in two kernels:
//
//   attn_decode_split_kernel  grid (B*H, SPLITS). Block (bh, split) owns keys
//     [split*chunk, (split+1)*chunk), chunk = ceil(S/SPLITS). Each of its NW
//     waves walks keys j = lo+wave, lo+wave+NW, ... computing
//     score_j = q . k_j (lane-split over D, wave-reduced) and keeps
//     wave-local online-softmax state (m, l, fp32 out accumulator in
//     registers); the waves merge through LDS and the block writes one
//     partial {m, l, acc[D]} to a workspace.
//   attn_decode_merge_kernel  grid B*H, one wave: merges the SPLITS partials
//     of its (b, h), normalises and writes out.
//
// Why two kernels: with one block per (b, h), decode batch 1 is
// LATENCY-bound — the grid is B*H = 16 blocks and each wave walks S/NW keys
// through a serial online-softmax chain (measured 68 us/call at S~160, the
// dominant decode cost). SPLITS = 8 gives 8x the parallelism and ~1/8 the
// serial chain. That one-kernel form (and its ZTA_DECODE_NOSPLIT=1 switch)
// is removed; it can be read at commit c9bc1d5.
//
// DPL is D per lane (ceil(D/64)); D up to 256. S_alloc is the allocated
// cache rows per (b, h) (the base stride); s_used is a device pointer to the
// LIVE number of cached keys — both kernels' launch arguments stay fixed and
// the split kernel reads the length in-kernel, so the pair is
// hipGraph-replayable with a growing cache. fp32 softmax throughout (the
// reference's inference mirror used F.scaled_dot_product_attention,
// torch_compatability/GPT2.py:237 — this is its MI355X-native replacement).

#include "common.h"

#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

namespace {

constexpr int NW = 4;  // waves per block
constexpr float NEG_INF = -3.0e38f;

template <int DPL, bool F16>
__global__ __launch_bounds__(NW * 64) void attn_decode_split_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ v, const float* __restrict__ slopes,
    float* __restrict__ part,  // (BH, SPLITS, 2 + 64*DPL)
    int H, int S_alloc, const int* __restrict__ s_used, int D, float scale,
    int splits) {
  const int S = s_used ? *s_used : S_alloc;
  __shared__ float red[NW * (3 + 64 * DPL)];
  const int bh = blockIdx.x;
  const int split = blockIdx.y;
  const int chunk = (S + splits - 1) / splits;
  const int lo = split * chunk;
  const int hi = min(S, lo + chunk);
  const int h = bh % H;
  const long base = (long)bh * S_alloc * D;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const float slope = slopes[h];
  auto cvt = [](uint16_t u) {
    if (F16) {
      __half hv = *reinterpret_cast<__half*>(&u);
      return __half2float(hv);
    }
    return bf16_to_f32(u);
  };

  float qv[DPL];
#pragma unroll
  for (int e = 0; e < DPL; ++e) {
    const int d = lane + e * 64;
    qv[e] = d < D ? cvt(q[(long)bh * D + d]) : 0.f;
  }
  float m = NEG_INF, l = 0.f;
  float acc[DPL];
#pragma unroll
  for (int e = 0; e < DPL; ++e) acc[e] = 0.f;

  for (int j = lo + wave; j < hi; j += NW) {
    const uint16_t* kr = &k[base + (long)j * D];
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < DPL; ++e) {
      const int d = lane + e * 64;
      if (d < D) s += qv[e] * cvt(kr[d]);
    }
    s = wave_reduce_sum(s);
    s = s * scale + slope * (float)(j - (S - 1));
    float alpha = 1.f;
    if (s > m) {
      alpha = m > 0.5f * NEG_INF ? __expf(m - s) : 0.f;
      m = s;
    }
    const float p = __expf(s - m);
    l = l * alpha + p;
    const uint16_t* vr = &v[base + (long)j * D];
#pragma unroll
    for (int e = 0; e < DPL; ++e) {
      const int d = lane + e * 64;
      acc[e] = acc[e] * alpha + (d < D ? p * cvt(vr[d]) : 0.f);
    }
  }

  // merge this block's NW waves, then write the partial
  float* wr = &red[wave * (3 + 64 * DPL)];
  if (lane == 0) {
    wr[0] = m;
    wr[1] = l;
  }
#pragma unroll
  for (int e = 0; e < DPL; ++e) wr[3 + lane + e * 64] = acc[e];
  __syncthreads();
  if (wave == 0) {
    float mg = NEG_INF;
#pragma unroll
    for (int w = 0; w < NW; ++w) mg = fmaxf(mg, red[w * (3 + 64 * DPL)]);
    float lg = 0.f;
    float og[DPL];
#pragma unroll
    for (int e = 0; e < DPL; ++e) og[e] = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const float mw = red[w * (3 + 64 * DPL)];
      const float f = mw > 0.5f * NEG_INF ? __expf(mw - mg) : 0.f;
      lg += red[w * (3 + 64 * DPL) + 1] * f;
#pragma unroll
      for (int e = 0; e < DPL; ++e)
        og[e] += red[w * (3 + 64 * DPL) + 3 + lane + e * 64] * f;
    }
    float* pr = &part[((long)bh * gridDim.y + split) * (2 + 64 * DPL)];
    if (lane == 0) {
      pr[0] = mg;
      pr[1] = lg;
    }
#pragma unroll
    for (int e = 0; e < DPL; ++e) pr[2 + lane + e * 64] = og[e];
  }
}

template <int DPL, bool F16>
__global__ __launch_bounds__(64) void attn_decode_merge_kernel(
    const float* __restrict__ part, uint16_t* __restrict__ out, int D,
    int splits) {
  const int bh = blockIdx.x;
  const int lane = threadIdx.x;
  const float* base = &part[(long)bh * splits * (2 + 64 * DPL)];
  float mg = NEG_INF;
  for (int s = 0; s < splits; ++s)
    mg = fmaxf(mg, base[s * (2 + 64 * DPL)]);
  float lg = 0.f;
  float og[DPL];
#pragma unroll
  for (int e = 0; e < DPL; ++e) og[e] = 0.f;
  for (int s = 0; s < splits; ++s) {
    const float* pr = &base[s * (2 + 64 * DPL)];
    const float f = pr[0] > 0.5f * NEG_INF ? __expf(pr[0] - mg) : 0.f;
    lg += pr[1] * f;
#pragma unroll
    for (int e = 0; e < DPL; ++e) og[e] += pr[2 + lane + e * 64] * f;
  }
  const float inv = lg > 0.f ? 1.f / lg : 0.f;
#pragma unroll
  for (int e = 0; e < DPL; ++e) {
    const int d = lane + e * 64;
    if (d < D) {
      const float o = og[e] * inv;
      if (F16) {
        __half hv = __float2half(o);
        out[(long)bh * D + d] = *reinterpret_cast<uint16_t*>(&hv);
      } else {
        out[(long)bh * D + d] = f32_to_bf16(o);
      }
    }
  }
}

}  // namespace

// `s_used`: optional 1-element int32 CUDA tensor with the live cache length
// (k/v may be larger preallocated buffers); empty tensor -> use k.size(2).
at::Tensor attn_decode(at::Tensor q, at::Tensor k, at::Tensor v,
                       at::Tensor slopes, at::Tensor s_used) {
  TORCH_CHECK(q.is_cuda() && q.is_contiguous() && q.dim() == 4 && q.size(2) == 1,
              "q must be (B, H, 1, D) contiguous");
  TORCH_CHECK(k.is_contiguous() && v.is_contiguous());
  const int B = q.size(0), H = q.size(1), D = q.size(3);
  const int S_alloc = k.size(2);
  TORCH_CHECK(D <= 256, "attn_decode: head_dim up to 256");
  const int* sp = nullptr;
  if (s_used.numel() > 0) {
    TORCH_CHECK(s_used.is_cuda() && s_used.scalar_type() == at::kInt);
    sp = s_used.data_ptr<int>();
  }
  auto out = at::empty_like(q);
  auto sl = slopes.to(at::kFloat).contiguous();
  const float scale = 1.0f / sqrtf((float)D);
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const int dpl = (D + 63) / 64;
  const bool f16 = q.scalar_type() == at::kHalf;
  TORCH_CHECK(f16 || q.scalar_type() == at::kBFloat16, "bf16 or fp16 only");

  const int splits = 8;  // blocks per (b, h) — see the file header
  auto part = at::empty({(long)B * H, splits, 2 + 64 * (long)dpl},
                        q.options().dtype(at::kFloat));
  dim3 grid(B * H, splits);
#define LAUNCH_SPLIT(DPL, F16V)                                                \
  do {                                                                         \
    hipLaunchKernelGGL((attn_decode_split_kernel<DPL, F16V>), grid,            \
                       dim3(NW * 64), 0, stream,                               \
                       (const uint16_t*)q.data_ptr(),                          \
                       (const uint16_t*)k.data_ptr(),                          \
                       (const uint16_t*)v.data_ptr(), sl.data_ptr<float>(),    \
                       part.data_ptr<float>(), H, S_alloc, sp, D, scale,       \
                       splits);                                                \
    hipLaunchKernelGGL((attn_decode_merge_kernel<DPL, F16V>), dim3(B * H),     \
                       dim3(64), 0, stream, part.data_ptr<float>(),            \
                       (uint16_t*)out.data_ptr(), D, splits);                  \
  } while (0)
  switch (dpl) {
    case 1: if (f16) LAUNCH_SPLIT(1, true); else LAUNCH_SPLIT(1, false); break;
    case 2: if (f16) LAUNCH_SPLIT(2, true); else LAUNCH_SPLIT(2, false); break;
    case 3: if (f16) LAUNCH_SPLIT(3, true); else LAUNCH_SPLIT(3, false); break;
    case 4: if (f16) LAUNCH_SPLIT(4, true); else LAUNCH_SPLIT(4, false); break;
    default: TORCH_CHECK(false, "bad head_dim");
  }
#undef LAUNCH_SPLIT
  return out;
}
