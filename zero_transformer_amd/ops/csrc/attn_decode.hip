// Single-token (decode) causal ALiBi attention for gfx950: q (B, H, 1, D)
// against a KV cache k/v (B, H, S, D) -> out (B, H, 1, D), with a
// per-sequence live length and an optional fused append of the new K/V row.
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
//
// Per-sequence length: block (bh, split) reads S = s_used[(bh / H) * s_stride]
// (s_stride 0: one length for the batch, 1: one per sequence), so chunk, lo,
// hi and the ALiBi origin S - 1 are per sequence; a sequence shorter than
// SPLITS leaves splits empty (m = NEG_INF partials, skipped by the merge).
// S is device data the host cannot check without a sync, so it is clamped to
// [0, S_alloc] here: with the append below an out-of-contract length would
// otherwise be an out-of-bounds write.
//
// q is addressed q[b * row_stride + h * D + d], so it can be the contiguous
// (B, H, 1, D) tensor (row_stride = H*D) or the first C columns of a
// (B, 3C) fused projection row (row_stride = 3C).
//
// Fused append (k_new / v_new non-null, same addressing as q: columns
// C..2C and 2C..3C of the projection row): key j == S - 1 is read from
// k_new / v_new instead of the cache, and the one wave that processes that
// key — in the single block with lo <= S - 1 < hi — also stores its D values
// into cache row S - 1 of k and v with plain vector stores. No other block
// reads row S - 1 from the cache in this launch (every block takes key S - 1
// from k_new / v_new, and only its owner visits it), so no ordering between
// blocks is needed; the next launch on the stream sees the row. S == 0 has no
// key S - 1 and writes nothing.

#include "attn_kv.h"  // NEG_INF, attn_decode_merge_kernel

#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

namespace {

constexpr int NW = 4;  // waves per block

template <int DPL, bool F16>
__global__ __launch_bounds__(NW * 64) void attn_decode_split_kernel(
    const uint16_t* __restrict__ q, uint16_t* __restrict__ k,
    uint16_t* __restrict__ v, const uint16_t* __restrict__ k_new,
    const uint16_t* __restrict__ v_new, long row_stride,
    const float* __restrict__ slopes,
    float* __restrict__ part,  // (BH, SPLITS, 2 + 64*DPL)
    int H, int S_alloc, const int* __restrict__ s_used, int s_stride, int D,
    float scale, int splits) {
  const int bh = blockIdx.x;
  const int S =
      s_used ? min(max(s_used[(bh / H) * s_stride], 0), S_alloc) : S_alloc;
  __shared__ float red[NW * (3 + 64 * DPL)];
  const int split = blockIdx.y;
  const int chunk = (S + splits - 1) / splits;
  const int lo = split * chunk;
  const int hi = min(S, lo + chunk);
  const int h = bh % H;
  const long base = (long)bh * S_alloc * D;
  const long row = (long)(bh / H) * row_stride + (long)h * D;  // q/k_new/v_new
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
    qv[e] = d < D ? cvt(q[row + d]) : 0.f;
  }
  float m = NEG_INF, l = 0.f;
  float acc[DPL];
#pragma unroll
  for (int e = 0; e < DPL; ++e) acc[e] = 0.f;

  for (int j = lo + wave; j < hi; j += NW) {
    // the appended key: read from the projection row, stored to the cache
    const bool fresh = k_new != nullptr && j == S - 1;
    const uint16_t* kr = fresh ? &k_new[row] : &k[base + (long)j * D];
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < DPL; ++e) {
      const int d = lane + e * 64;
      if (d < D) {
        const uint16_t ku = kr[d];
        if (fresh) k[base + (long)j * D + d] = ku;
        s += qv[e] * cvt(ku);
      }
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
    const uint16_t* vr = fresh ? &v_new[row] : &v[base + (long)j * D];
#pragma unroll
    for (int e = 0; e < DPL; ++e) {
      const int d = lane + e * 64;
      const uint16_t vu = d < D ? vr[d] : (uint16_t)0;
      if (fresh && d < D) v[base + (long)j * D + d] = vu;
      acc[e] = acc[e] * alpha + (d < D ? p * cvt(vu) : 0.f);
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

}  // namespace

namespace {

// Launches the split + merge pair. q/k_new/v_new are addressed
// [b * row_stride + h * D + d]; k_new/v_new may be null (no append).
void launch_decode(const void* q, long row_stride, const void* k_new,
                   const void* v_new, at::Tensor& k, at::Tensor& v,
                   const at::Tensor& slopes, const at::Tensor& s_used, int B,
                   at::Tensor& out) {
  TORCH_CHECK(k.is_cuda() && v.is_cuda() && k.dim() == 4 && k.is_contiguous() &&
                  v.is_contiguous() && k.sizes() == v.sizes() &&
                  k.scalar_type() == v.scalar_type(),
              "k/v must be (B, H, S, D) contiguous, same shape and dtype");
  const int H = k.size(1), S_alloc = k.size(2), D = k.size(3);
  TORCH_CHECK(k.size(0) == B, "k/v batch does not match q");
  TORCH_CHECK(D <= 256, "attn_decode: head_dim up to 256");
  TORCH_CHECK(slopes.numel() == H, "slopes must have one entry per head");
  const int* sp = nullptr;
  int s_stride = 0;
  if (s_used.numel() > 0) {
    TORCH_CHECK(s_used.is_cuda() && s_used.scalar_type() == at::kInt &&
                    s_used.is_contiguous(),
                "s_used must be a contiguous int32 device tensor");
    TORCH_CHECK(s_used.numel() == 1 || s_used.numel() == B,
                "s_used must hold 0, 1 or B elements");
    sp = s_used.data_ptr<int>();
    // B == 1: either stride reads element 0
    s_stride = s_used.numel() == B && B > 1 ? 1 : 0;
  }
  auto sl = slopes.to(at::kFloat).contiguous();
  const float scale = 1.0f / sqrtf((float)D);
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const int dpl = (D + 63) / 64;
  const bool f16 = k.scalar_type() == at::kHalf;
  TORCH_CHECK(f16 || k.scalar_type() == at::kBFloat16, "bf16 or fp16 only");

  const int splits = 8;  // blocks per (b, h) — see the file header
  auto part = at::empty({(long)B * H, splits, 2 + 64 * (long)dpl},
                        k.options().dtype(at::kFloat));
  dim3 grid(B * H, splits);
#define LAUNCH_SPLIT(DPL, F16V)                                                \
  do {                                                                         \
    hipLaunchKernelGGL((attn_decode_split_kernel<DPL, F16V>), grid,            \
                       dim3(NW * 64), 0, stream, (const uint16_t*)q,           \
                       (uint16_t*)k.data_ptr(), (uint16_t*)v.data_ptr(),       \
                       (const uint16_t*)k_new, (const uint16_t*)v_new,         \
                       row_stride, sl.data_ptr<float>(),                       \
                       part.data_ptr<float>(), H, S_alloc, sp, s_stride, D,    \
                       scale, splits);                                         \
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
}

}  // namespace

// `s_used`: optional int32 device tensor with the live cache length (k/v may
// be larger preallocated buffers): 1 element for the whole batch, B elements
// for one length per sequence; empty tensor -> use k.size(2).
at::Tensor attn_decode(at::Tensor q, at::Tensor k, at::Tensor v,
                       at::Tensor slopes, at::Tensor s_used) {
  TORCH_CHECK(q.is_cuda() && q.is_contiguous() && q.dim() == 4 && q.size(2) == 1,
              "q must be (B, H, 1, D) contiguous");
  TORCH_CHECK(k.dim() == 4 && q.size(1) == k.size(1) && q.size(3) == k.size(3) &&
                  q.scalar_type() == k.scalar_type(),
              "q and k/v disagree on heads, head_dim or dtype");
  auto out = at::empty_like(q);
  launch_decode(q.data_ptr(), (long)q.size(1) * q.size(3), nullptr, nullptr, k,
                v, slopes, s_used, q.size(0), out);
  return out;
}

// Decode step on the fused projection: qkv (B, 1, 3C) contiguous, caches
// (B, H, S_alloc, D) written in place at row lens[b] - 1, lens (B,) int32 on
// device INCLUDING the new token. Returns (B, 1, C) — the (B, H, 1, D)
// kernel output is the same memory for one token.
at::Tensor attn_decode_append(at::Tensor qkv, at::Tensor k_cache,
                              at::Tensor v_cache, at::Tensor slopes,
                              at::Tensor lens) {
  TORCH_CHECK(qkv.is_cuda() && qkv.is_contiguous() && qkv.dim() == 3 &&
                  qkv.size(1) == 1 && qkv.size(2) % 3 == 0,
              "qkv must be (B, 1, 3C) contiguous");
  const long B = qkv.size(0), C = qkv.size(2) / 3;
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.size(1) * k_cache.size(3) == C &&
                  k_cache.scalar_type() == qkv.scalar_type(),
              "k_cache/v_cache must be (B, H, S_alloc, D) with H*D == C, of "
              "qkv's dtype");
  TORCH_CHECK(lens.dim() == 1 && lens.numel() == B,
              "lens must be a (B,) int32 device tensor");
  auto out = at::empty({B, 1, C}, qkv.options());
  const uint16_t* row = (const uint16_t*)qkv.data_ptr();
  launch_decode(row, 3 * C, row + C, row + 2 * C, k_cache, v_cache, slopes,
                lens, B, out);
  return out;
}
