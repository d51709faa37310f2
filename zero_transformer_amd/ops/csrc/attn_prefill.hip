// Prefill attention for gfx950: a block of new rows of the fused projection
// against the KV cache, with per-sequence lengths, a per-sequence number of
// rows already cached, and the cache fill fused in.
//
//   attn_prefill_append(qkv (B, T, 3C), k_cache / v_cache (B, H, S_alloc, D),
//                       slopes (H), lens (B) int32, start (B) int32) -> o (B, T, C)
//
// For sequence b, st = clamp(start[b], 0, S_alloc) rows are already cached and
// n = clamp(lens[b], 0, min(T, S_alloc - st)) rows of qkv are new. K/V rows
// i < n go to cache rows st + i (no other cache row is written). Query row
// i < n sits at position st + i and attends over cache rows [0, st + i] with
// the ALiBi bias slope_h * (j - (st + i)), fp32 softmax statistics. Rows
// i >= n of o are zeros. lens / start are device data read in-kernel: no host
// sync, and an out-of-contract value is clamped because it addresses a write.
//
// Two kernels on one stream, as in decode:
//   prefill_append_kernel  copies the K / V columns of the live qkv rows into
//     the caches, 16 B per lane.
//   prefill_flash_kernel  (attn_kv.h, with the scheme) attends the new rows
//     over cache rows [0, st + i].
// No atomics: the output is deterministic.

#include "attn_kv.h"

#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <type_traits>

namespace {

// One item = 8 elements (16 B) of the K or V columns of one qkv row.
__global__ __launch_bounds__(256) void prefill_append_kernel(
    const uint16_t* __restrict__ qkv, uint16_t* __restrict__ kc,
    uint16_t* __restrict__ vc, const int* __restrict__ lens,
    const int* __restrict__ start, int B, int H, int T, int C, int D, int S_alloc) {
  const int c8n = C / 8;
  const long total = (long)B * T * 2 * c8n;
  for (long it = (long)blockIdx.x * blockDim.x + threadIdx.x; it < total;
       it += (long)gridDim.x * blockDim.x) {
    const int c8 = (int)(it % c8n);
    const int kv = (int)((it / c8n) & 1);
    const long bt = it / (2 * c8n);
    const int i = (int)(bt % T), b = (int)(bt / T);
    const auto [st, n] = seq_range(lens, start, b, T, S_alloc);
    if (i >= n) continue;
    const int col = c8 * 8, h = col / D, d = col % D;
    const s16x8 x = *reinterpret_cast<const s16x8*>(&qkv[bt * 3 * C + (1 + kv) * C + col]);
    uint16_t* dst = kv ? vc : kc;
    *reinterpret_cast<s16x8*>(&dst[(((long)b * H + h) * S_alloc + st + i) * D + d]) = x;
  }
}

template <int D, bool F16>
void launch_prefill(const at::Tensor& qkv, const at::Tensor& kc, const at::Tensor& vc,
                    const at::Tensor& slopes, at::Tensor& o, const int* lens,
                    const int* start, int B, int H, int T, int C, int S_alloc,
                    hipStream_t stream) {
  const size_t smem = 4 * TB * 128 * sizeof(uint16_t);  // 2 tensors x 2 buffers
  constexpr int QROWS = PREFILL_NT / 2;
  dim3 grid(B * H, (T + QROWS - 1) / QROWS);
  hipLaunchKernelGGL((prefill_flash_kernel<D, PREFILL_NT, F16>), grid, dim3(PREFILL_NT),
                     smem, stream, (const uint16_t*)qkv.data_ptr(),
                     (const uint16_t*)kc.data_ptr(), (const uint16_t*)vc.data_ptr(),
                     slopes.data_ptr<float>(), (uint16_t*)o.data_ptr(), lens, start, H,
                     T, C, S_alloc, 1.0f / sqrtf((float)D));
}

}  // namespace

// qkv (B, T, 3C) fp16 / bf16 contiguous; caches (B, H, S_alloc, D) of the same
// dtype, written in place; lens / start (B,) int32 on the device. -> (B, T, C)
at::Tensor attn_prefill_append(at::Tensor qkv, at::Tensor k_cache, at::Tensor v_cache,
                               at::Tensor slopes, at::Tensor lens, at::Tensor start) {
  TORCH_CHECK(qkv.is_cuda() && qkv.is_contiguous() && qkv.dim() == 3 &&
                  qkv.size(2) % 3 == 0,
              "qkv must be (B, T, 3C) contiguous");
  const bool f16 = qkv.scalar_type() == at::kHalf;
  TORCH_CHECK(f16 || qkv.scalar_type() == at::kBFloat16,
              "attn_prefill_append: fp16 or bf16 only");
  const int B = qkv.size(0), T = qkv.size(1), C = qkv.size(2) / 3;
  TORCH_CHECK(k_cache.is_cuda() && v_cache.is_cuda() && k_cache.dim() == 4 &&
                  k_cache.is_contiguous() && v_cache.is_contiguous() &&
                  k_cache.sizes() == v_cache.sizes() &&
                  k_cache.scalar_type() == qkv.scalar_type() &&
                  v_cache.scalar_type() == qkv.scalar_type() &&
                  k_cache.size(0) == B && k_cache.size(1) * k_cache.size(3) == C,
              "k_cache/v_cache must be (B, H, S_alloc, D) contiguous with H*D == C, "
              "of qkv's dtype");
  const int H = k_cache.size(1), S_alloc = k_cache.size(2), D = k_cache.size(3);
  TORCH_CHECK(slopes.numel() == H, "slopes must have one entry per head");
  for (const at::Tensor* t : {&lens, &start})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kInt && t->dim() == 1 &&
                    t->numel() == B && t->is_contiguous(),
                "lens and start must be (B,) contiguous int32 device tensors");
  auto o = at::empty({B, T, C}, qkv.options());
  if (B == 0 || T == 0) return o;
  auto sl = slopes.to(at::kFloat).contiguous();
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const int* lp = lens.data_ptr<int>();
  const int* sp = start.data_ptr<int>();
  const bool ok = attn::with_head_dim(D, [&](auto d) {
    constexpr int DD = decltype(d)::value;
    hipLaunchKernelGGL(prefill_append_kernel,
                       dim3(capped_grid((long)B * T * 2 * (C / 8), 256)), dim3(256), 0,
                       stream, (const uint16_t*)qkv.data_ptr(),
                       (uint16_t*)k_cache.data_ptr(), (uint16_t*)v_cache.data_ptr(), lp,
                       sp, B, H, T, C, D, S_alloc);
    if (f16)
      launch_prefill<DD, true>(qkv, k_cache, v_cache, sl, o, lp, sp, B, H, T, C, S_alloc,
                               stream);
    else
      launch_prefill<DD, false>(qkv, k_cache, v_cache, sl, o, lp, sp, B, H, T, C, S_alloc,
                                stream);
  });
  TORCH_CHECK(ok, "attn_prefill_append: head_dim must be one of 32/64/96/128, got ", D);
  return o;
}
