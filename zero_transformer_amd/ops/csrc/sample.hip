// Fused, sort-free token sampler with per-row options (gfx950).
//
// One workgroup of 1024 threads per row of logits (B, V), V <= 65536. Thread
// t owns `per` consecutive tokens (per = a multiple of one 16-byte chunk, at
// most 64), reads them from HBM once with dwordx4 loads, applies the
// repetition penalty and keeps the penalised values y in 64 fp32 registers
// for every later phase:
//
//   max / argmax          block reductions (greedy rows stop here)
//   top-k threshold kth   bisection on the order-preserving integer image
//                         of the fp32 value (32 steps; 19 / 16 for fp16 /
//                         bf16 logits, whose images have 13 / 16 zero low
//                         bits), one block-reduced count per step
//   top-p threshold cut   the same bisection with a block-reduced mass
//   draw                  block-wide inclusive scan of the kept weights in
//                         token order against u = uniform01(seed, counter)
//
// Nothing is sorted and nothing is accumulated with atomics: every float
// sum is thread-sequential, then a 64-lane butterfly (the same bits in
// every lane), then the 16 wave totals in wave order, so the result is a
// function of the inputs alone. Weights exp((y - max) / T) are recomputed
// from the resident y where they are needed instead of being held (a second
// 64-register array would not fit the 128-VGPR budget of a 1024-thread
// workgroup).
//
// Rows need not be 16-byte aligned (V = 50257): ownership is laid out from
// the aligned address below the row start, chunks that straddle a row end
// are read element by element, and no byte outside the row is touched.

#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include "common.h"

namespace {

constexpr int THREADS = 1024;
constexpr int NW = THREADS / WAVE;
constexpr int PER = 64;  // resident values per thread
constexpr int MAX_V = THREADS * PER;

// DT: 0 = fp16, 1 = bf16, 2 = fp32
template <int DT>
struct Fmt {
  static constexpr int ES = DT == 2 ? 4 : 2;  // bytes per element
  static constexpr int EPC = 16 / ES;         // elements per 16-byte chunk
  // Low bits of the fp32 image that are zero for every value of the format
  // (23 mantissa bits against 10 / 7): a key's low bits are then all zeros
  // (positive values) or all ones (negative values), two values differ in
  // the bits above, and a bisection over those bits alone finds the same
  // threshold in 19 / 16 steps instead of 32.
  static constexpr int LOW = DT == 0 ? 13 : DT == 1 ? 16 : 0;
};

template <int DT>
ZTA_DEV float widen16(uint16_t h) {
  if constexpr (DT == 0) {
    return float(__builtin_bit_cast(_Float16, h));
  } else {
    return bf16_to_f32(h);
  }
}

// Round to the logits' dtype and widen again (what a torch op on the 16-bit
// tensor leaves behind).
template <int DT>
ZTA_DEV float round_to(float v) {
  if constexpr (DT == 0) {
    return float(_Float16(v));
  } else if constexpr (DT == 1) {
    return bf16_to_f32(f32_to_bf16(v));
  } else {
    return v;
  }
}

template <int DT>
ZTA_DEV float load_one(const char* row, int i) {
  if constexpr (DT == 2) {
    return ((const float*)row)[i];
  } else {
    return widen16<DT>(((const uint16_t*)row)[i]);
  }
}

// Order-preserving map fp32 -> uint32 and back (a <= b  <=>  key(a) <= key(b)
// for non-NaN values; -0 is canonicalised to +0 before it gets here).
ZTA_DEV float key_to_f32(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// The key of the value a bisection over bits [LOW, 32) ended on: a negative
// value's key carries ones in the LOW bits that were not searched.
template <int LOW>
ZTA_DEV uint32_t finish_key(uint32_t k) {
  return (k & 0x80000000u) ? k : (k | ((1u << LOW) - 1u));
}

// Block reductions. `s` holds NW words; consecutive calls alternate between
// two such buffers, so one barrier per call is enough: a buffer is written
// again only after every thread has passed the barrier of the call between.
template <typename T, typename Op>
ZTA_DEV T block_reduce(T v, Op op, uint32_t* s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_xor(v, off, WAVE));
  if ((threadIdx.x & (WAVE - 1)) == 0) s[threadIdx.x / WAVE] = __builtin_bit_cast(uint32_t, v);
  __syncthreads();
  T r = __builtin_bit_cast(T, s[0]);
#pragma unroll
  for (int w = 1; w < NW; ++w) r = op(r, __builtin_bit_cast(T, s[w]));
  return r;
}

struct OpSum {
  template <typename T>
  ZTA_DEV T operator()(T a, T b) const { return a + b; }
};
struct OpMaxF {
  ZTA_DEV float operator()(float a, float b) const { return fmaxf(a, b); }
};
struct OpMinI {
  ZTA_DEV int operator()(int a, int b) const { return a < b ? a : b; }
};
struct OpMaxI {
  ZTA_DEV int operator()(int a, int b) const { return a > b ? a : b; }
};

template <int DT>
__global__ __launch_bounds__(THREADS) void sample_rows_kernel(
    const char* __restrict__ logits, const uint8_t* __restrict__ seen,
    const float* __restrict__ temperature, const int* __restrict__ top_k,
    const float* __restrict__ top_p, const float* __restrict__ penalty,
    const int64_t* __restrict__ seed, const int64_t* __restrict__ counter,
    int64_t* __restrict__ tokens, float* __restrict__ cut_out, int V) {
  constexpr int ES = Fmt<DT>::ES, EPC = Fmt<DT>::EPC, NCH = PER / EPC, LOW = Fmt<DT>::LOW;
  __shared__ uint32_t red[2][NW];
  __shared__ float wconst[2];
  int phase = 0;
#define ZTA_RED (red[(phase++) & 1])

  const int b = blockIdx.x;
  const int t = threadIdx.x;
  const char* row = logits + (size_t)b * V * ES;
  const uint8_t* srow = seen ? seen + (size_t)b * V : nullptr;

  const float T = temperature[b];
  const float r = penalty[b];
  const bool penalise = srow != nullptr && r != 1.0f;

  // thread t owns tokens [i0, i0 + per) clipped to [0, V); row + i0 * ES is
  // 16-byte aligned for every t
  const int mis = int(((uintptr_t)row & 15) / ES);
  const int cpt = (V + mis + THREADS * EPC - 1) / (THREADS * EPC);  // <= NCH
  const int per = cpt * EPC;
  const int i0 = t * per - mis;

  float y[PER];
  float m_loc = -INFINITY;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    if (c < cpt) {
      const int ic = i0 + c * EPC;
      float x[EPC];
      if (ic >= 0 && ic + EPC <= V) {
        union {
          uint4 v;
          uint16_t h[8];
          float f[4];
        } u;
        u.v = *(const uint4*)(row + (ptrdiff_t)ic * ES);
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
          if constexpr (DT == 2) {
            x[e] = u.f[e];
          } else {
            x[e] = widen16<DT>(u.h[e]);
          }
        }
      } else {
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
          const int i = ic + e;
          x[e] = (i >= 0 && i < V) ? load_one<DT>(row, i) : -INFINITY;
        }
      }
      if (penalise) {
        bool s[EPC];
        if (ic >= 0 && ic + EPC <= V && (((uintptr_t)(srow + ic)) & (EPC - 1)) == 0) {
          union {
            uint64_t q;
            uint32_t d;
            uint8_t c[8];
          } u;
          if constexpr (EPC == 8) {
            u.q = *(const uint64_t*)(srow + ic);
          } else {
            u.d = *(const uint32_t*)(srow + ic);
          }
#pragma unroll
          for (int e = 0; e < EPC; ++e) s[e] = u.c[e] != 0;
        } else {
#pragma unroll
          for (int e = 0; e < EPC; ++e) {
            const int i = ic + e;
            s[e] = (i >= 0 && i < V) ? srow[i] != 0 : false;
          }
        }
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
          // fp32, true division, rounded to the logits' dtype: the bits
          // of apply_repetition_penalty_batched
          const float pen = round_to<DT>(x[e] > 0.0f ? x[e] / r : x[e] * r);
          x[e] = s[e] ? pen : x[e];
        }
      }
#pragma unroll
      for (int e = 0; e < EPC; ++e) {
        float v = x[e];
        v = (v != v) ? -INFINITY : v;  // NaN is outside the contract: drop it
        v = (v == 0.0f) ? 0.0f : v;    // -0 -> +0: one key per value
        y[c * EPC + e] = v;
        m_loc = fmaxf(m_loc, v);
      }
    } else {
#pragma unroll
      for (int e = 0; e < EPC; ++e) y[c * EPC + e] = -INFINITY;
    }
  }
  // padding (tokens outside [0, V)) is -inf: weight 0, below every finite
  // threshold, and the index guards below keep it out of the results

  const float m = block_reduce(m_loc, OpMaxF(), ZTA_RED);

  if (!(T > 0.0f)) {  // greedy: lowest index of the maximum
    int first = INT_MAX;
#pragma unroll
    for (int c = NCH - 1; c >= 0; --c) {
      if (c < cpt) {
#pragma unroll
        for (int e = EPC - 1; e >= 0; --e) {
          const int i = i0 + c * EPC + e;
          if (y[c * EPC + e] == m && i >= 0 && i < V) first = i;
        }
      }
    }
    first = block_reduce(first, OpMinI(), ZTA_RED);
    if (t == 0) {
      tokens[b] = first < V ? first : V - 1;
      cut_out[b] = m;
    }
    return;
  }

  // ---- top-k: kth = the k-th largest value, ties counted ----
  float kth = -INFINITY;
  const int k = top_k[b];
  if (k > 0 && k < V) {
    uint32_t key = 0;
    for (int bit = 31; bit >= LOW; --bit) {
      const uint32_t cand = key | (1u << bit);
      const float v = key_to_f32(cand);
      if (v != v) continue;  // a NaN pattern: nothing is >= it (uniform)
      uint32_t cnt = 0;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        if (c < cpt) {
#pragma unroll
          for (int e = 0; e < EPC; ++e) cnt += y[c * EPC + e] >= v ? 1u : 0u;
        }
      }
      cnt = block_reduce(cnt, OpSum(), ZTA_RED);
      if (cnt >= (uint32_t)k) key = cand;
    }
    kth = key_to_f32(finish_key<LOW>(key));
    if (kth != kth) kth = -INFINITY;  // fewer than k values above -inf
  }

  // weight of a value: exp((v - m) / max(T, 1e-5)) as one exp2. The two
  // constants are re-read from LDS by every pass: a load cannot move across
  // the barrier of the reduction between two passes, so the 64 weights are
  // recomputed per pass and not hoisted out of the bisection loop into 64
  // more registers.
  if (t == 0) {
    wconst[0] = m;
    wconst[1] = 1.4426950408889634f / fmaxf(T, 1e-5f);
  }
  __syncthreads();
  auto mass_ge = [&](float v) {  // thread-local sum of w over y >= v, in order
    const float m = wconst[0], scale = wconst[1];
    float acc = 0.0f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (c < cpt) {
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
          const float yv = y[c * EPC + e];
          const float w = __builtin_amdgcn_exp2f((yv - m) * scale);
          acc += yv >= v ? w : 0.0f;
        }
      }
    }
    return acc;
  };

  // ---- top-p: the largest value whose upper mass exceeds p * Z_K ----
  float cut = kth;
  const float p = fmaxf(top_p[b], 0.0f);
  if (p < 1.0f) {
    const float zk = block_reduce(mass_ge(kth), OpSum(), ZTA_RED);
    const float pz = p * zk;
    uint32_t key = 0;
    for (int bit = 31; bit >= LOW; --bit) {
      const uint32_t cand = key | (1u << bit);
      const float v = key_to_f32(cand);
      if (v != v) continue;
      const float mass = block_reduce(mass_ge(fmaxf(v, kth)), OpSum(), ZTA_RED);
      if (mass > pz) key = cand;
    }
    const float c = key_to_f32(finish_key<LOW>(key));
    cut = c >= kth ? c : kth;  // also when no key passed (NaN) or p*Z rounded to Z
  }

  // ---- draw: first token whose inclusive kept mass exceeds u * Z_S ----
  const float u = uniform01((uint64_t)seed[b], (uint64_t)counter[b]);
  const float s_loc = mass_ge(cut);
  float inc = s_loc;  // inclusive scan over the wave, lane order
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const float o = __shfl_up(inc, off, WAVE);
    if ((t & (WAVE - 1)) >= off) inc += o;
  }
  float excl = __shfl_up(inc, 1, WAVE);
  if ((t & (WAVE - 1)) == 0) excl = 0.0f;
  uint32_t* sc = ZTA_RED;
  if ((t & (WAVE - 1)) == WAVE - 1) sc[t / WAVE] = __float_as_uint(inc);
  __syncthreads();
  float base = 0.0f, total = 0.0f;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    if (w == t / WAVE) base = total;
    total += __uint_as_float(sc[w]);
  }
  const float target = u * total;
  const float scale = wconst[1];
  float run = base + excl;
  int first = INT_MAX, last = -1;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    if (c < cpt) {
#pragma unroll
      for (int e = 0; e < EPC; ++e) {
        const float yv = y[c * EPC + e];
        const int i = i0 + c * EPC + e;
        if (yv >= cut && i >= 0 && i < V) {
          run += __builtin_amdgcn_exp2f((yv - m) * scale);
          last = i;
          if (run > target && first == INT_MAX) first = i;
        }
      }
    }
  }
  first = block_reduce(first, OpMinI(), ZTA_RED);
  last = block_reduce(last, OpMaxI(), ZTA_RED);
  if (t == 0) {
    int tok = first != INT_MAX ? first : last;
    tok = tok < 0 ? 0 : (tok < V ? tok : V - 1);
    tokens[b] = tok;
    cut_out[b] = cut;
  }
#undef ZTA_RED
}

}  // namespace

// Per-row sampling of logits (B, V) fp16/bf16/fp32 -> {tokens (B,) int64,
// cut (B,) fp32}; `seen` (B, V) bool or an undefined tensor. Semantics:
// ops.sample_rows / ops.reference.sample_rows.
std::vector<at::Tensor> sample_rows(at::Tensor logits, c10::optional<at::Tensor> seen,
                                    at::Tensor temperature, at::Tensor top_k,
                                    at::Tensor top_p, at::Tensor penalty,
                                    at::Tensor seed, at::Tensor counter) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.is_contiguous(),
              "sample_rows: logits must be a contiguous (B, V) device tensor");
  const int64_t B = logits.size(0), V = logits.size(1);
  const auto st = logits.scalar_type();
  TORCH_CHECK(st == at::kHalf || st == at::kBFloat16 || st == at::kFloat,
              "sample_rows: fp16, bf16 or fp32 logits");
  const int es = st == at::kFloat ? 4 : 2;
  const bool aligned = (uintptr_t)logits.data_ptr() % 16 == 0 && (V * es) % 16 == 0;
  TORCH_CHECK(V >= 1 && V + (aligned ? 0 : 16 / es - 1) <= MAX_V,
              "sample_rows: V = ", V, " exceeds the kernel's ", MAX_V);
  auto row_vec = [&](const at::Tensor& x, at::ScalarType want, const char* name) {
    TORCH_CHECK(x.is_cuda() && x.get_device() == logits.get_device() &&
                    x.scalar_type() == want && x.dim() == 1 && x.size(0) == B &&
                    x.is_contiguous(),
                "sample_rows: ", name, " must be a contiguous (B,) tensor of the "
                "documented dtype on the device of logits");
  };
  row_vec(temperature, at::kFloat, "temperature");
  row_vec(top_k, at::kInt, "top_k");
  row_vec(top_p, at::kFloat, "top_p");
  row_vec(penalty, at::kFloat, "penalty");
  row_vec(seed, at::kLong, "seed");
  row_vec(counter, at::kLong, "counter");
  const uint8_t* seen_p = nullptr;
  if (seen.has_value() && seen->defined()) {
    TORCH_CHECK(seen->is_cuda() && seen->get_device() == logits.get_device() &&
                    seen->scalar_type() == at::kBool && seen->dim() == 2 &&
                    seen->size(0) == B && seen->size(1) == V && seen->is_contiguous(),
                "sample_rows: seen must be a contiguous (B, V) bool tensor");
    seen_p = (const uint8_t*)seen->data_ptr();
  }
  at::Tensor tokens = at::empty({B}, logits.options().dtype(at::kLong));
  at::Tensor cut = at::empty({B}, logits.options().dtype(at::kFloat));
  if (B == 0) return {tokens, cut};
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
#define ZTA_SAMPLE_LAUNCH(DT)                                                      \
  hipLaunchKernelGGL((sample_rows_kernel<DT>), dim3((unsigned)B), dim3(THREADS), 0, \
                     stream, (const char*)logits.data_ptr(), seen_p,               \
                     temperature.data_ptr<float>(), top_k.data_ptr<int>(),         \
                     top_p.data_ptr<float>(), penalty.data_ptr<float>(),           \
                     seed.data_ptr<int64_t>(), counter.data_ptr<int64_t>(),        \
                     tokens.data_ptr<int64_t>(), cut.data_ptr<float>(), int(V))
  if (st == at::kHalf) {
    ZTA_SAMPLE_LAUNCH(0);
  } else if (st == at::kBFloat16) {
    ZTA_SAMPLE_LAUNCH(1);
  } else {
    ZTA_SAMPLE_LAUNCH(2);
  }
#undef ZTA_SAMPLE_LAUNCH
  return {tokens, cut};
}
