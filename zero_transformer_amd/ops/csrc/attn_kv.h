// What the KV-cache attention ops (attn_prefill.hip, attn_paged.hip,
// attn_decode.hip) share: the element-type helpers, the per-sequence range
// and page lookup, the flash kernel of the contiguous prompt pass, whose
// scheme the paged one follows, and the one merge kernel of the split-S
// decode.
//
// prefill_flash_kernel<D, NT, F16>  grid (B*H, q blocks) — the
//   grid-orientation rule of the training forward. It is the round-1
//   flash_fwd_kernel scheme (attention_fwd.hip header: swapped QK^T,
//   in-register P, transpose-read V), correct at every head dim, with these
//   differences:
//     - Q comes from qkv (row stride 3C); K/V tiles are staged FROM THE
//       CACHE, where a 64-key tile is one contiguous 64*D*2-byte block;
//     - the key loop runs from cache row 0 to the block's diagonal at
//       st + q0 + rows; only sub-tiles that touch a wave's diagonal, or a
//       wave with dead rows, evaluate the mask;
//     - a block whose first row is >= n writes its zeros and returns before
//       any barrier; dead rows of a live block are stored as zeros;
//     - the tile-ready barrier is attn::tile_barrier<0>() (s_waitcnt
//       vmcnt(0) in front of s_barrier): the LDS-DMA of the tile is waited
//       for, which a plain __syncthreads() does not do;
//     - fp16 or bf16 (MFMA 32x32x16 f16 / bf16; P and O are rounded to
//       nearest even in either type); no dropout, no lse;
//     - O leaves as whole rows, 16 B per lane, through the idle K/V
//       buffers (the epilogue of flash_fwd_v2_kernel).
//   QROWS q rows per block = 32 per wave; see PREFILL_NT for the choice.
//   paged_flash_kernel (attn_paged.hip) is this body with other staging
//   calls; why it is a second body is said there.
//
// Everything sits in an unnamed namespace, as it did in the .hip files: each
// file instantiates its own kernels, under the symbols they always had.
#pragma once

#include "attn_tiles.h"
#include "common.h"

#include <hip/hip_fp16.h>

namespace {

using attn::TB;
using attn::swz;

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;

constexpr float NEG_INF = -3.0e38f;

// Two f32 -> one packed word of the element type, round to nearest even.
template <bool F16>
ZTA_DEV unsigned pack2(float a, float b) {
  if constexpr (F16) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, f16x2));
  } else {
    unsigned w;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(w) : "v"(a), "v"(b));
    return w;
  }
}

// Fragments travel as bf16x8 bit patterns (the transpose-read helpers of
// attn_tiles.h are element-type agnostic); the MFMA picks the type.
template <bool F16>
ZTA_DEV f32x16 mfma16(bf16x8 a, bf16x8 b, f32x16 c) {
  if constexpr (F16) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a),
                                                  __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  } else {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
}

// attn::c_to_a_frags for either element type (same register shuffle).
template <bool F16>
ZTA_DEV void p_to_a_frags(const float* x, bf16x8* pa) {
  unsigned w[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j] = pack2<F16>(x[2 * j], x[2 * j + 1]);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    auto r0 = __builtin_amdgcn_permlane32_swap(w[4 * j + 0], w[4 * j + 2], false, false);
    w[4 * j + 0] = r0[0];
    w[4 * j + 2] = r0[1];
    auto r1 = __builtin_amdgcn_permlane32_swap(w[4 * j + 1], w[4 * j + 3], false, false);
    w[4 * j + 1] = r1[0];
    w[4 * j + 3] = r1[1];
  }
  union {
    unsigned u[4];
    bf16x8 v8;
  } cvt;
  cvt.u[0] = w[0]; cvt.u[1] = w[1]; cvt.u[2] = w[2]; cvt.u[3] = w[3];
  pa[0] = cvt.v8;
  cvt.u[0] = w[4]; cvt.u[1] = w[5]; cvt.u[2] = w[6]; cvt.u[3] = w[7];
  pa[1] = cvt.v8;
}

// Rows already cached (st) and new rows (n) of sequence b, clamped to the
// cap rows its cache can hold: they address writes.
struct SeqRange {
  int st, n;
};
ZTA_DEV SeqRange seq_range(const int* lens, const int* start, int b, int T, int cap) {
  const int st = min(max(start[b], 0), cap);
  const int n = min(max(lens[b], 0), min(T, cap - st));
  return {st, n};
}

// Pool geometry: P pages of R rows; a sequence's table row has M entries.
struct Pool {
  int P, R, M;
};

// Page of logical page index pi (< M) of sequence b, clamped to the pool.
ZTA_DEV int page_of(const int* __restrict__ bt, int b, int pi, Pool pl) {
  return min(max(bt[(long)b * pl.M + pi], 0), pl.P - 1);
}

template <int D, int NT, bool F16>
__global__ __launch_bounds__(NT, 2) void prefill_flash_kernel(
    const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ kc,
    const uint16_t* __restrict__ vc, const float* __restrict__ slopes,
    uint16_t* __restrict__ o, const int* __restrict__ lens,
    const int* __restrict__ start, int H, int T, int C, int S_alloc, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // double-buffered LDS-DMA staging: layout [k0 | v0 | k1 | v1]
  uint16_t* lds0 = (uint16_t*)smem;

  const int bh = blockIdx.x;
  const auto [h, QS, base, kbase_, vbase_, obase] = attn::planes<D>(bh, H, T, C);
  const auto [st, n] = seq_range(lens, start, bh / H, T, S_alloc);
  constexpr int QROWS = NT / 2;  // 32 q rows per wave
  constexpr int LPR = D / 8;     // lanes (16 B each) per O row
  const int q0 = blockIdx.y * QROWS;

  if (q0 >= n) {  // block-uniform: nothing live here, zeros and out
    const int rows = min(QROWS, T - q0);
    for (int idx = threadIdx.x; idx < rows * LPR; idx += NT)
      *reinterpret_cast<s16x8*>(
          &o[obase + (long)(q0 + idx / LPR) * C + (idx % LPR) * 8]) = s16x8{};
    return;
  }

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int li = lane & 31;
  const int hi = lane >> 5;
  const int qw = q0 + wave * 32;
  const int qi = qw + li;   // THIS lane's q row (swapped layout)
  const bool ok = qi < n;
  const int pw = st + qw;   // position of the wave's first row
  const int pi = st + qi;   // position of this lane's row
  const long cbase = (long)bh * S_alloc * D;  // this (b, h)'s cache plane
  constexpr float LOG2E = 1.4426950408889634f;
  constexpr float DEFER_THR = 11.5f;  // ~8 nats in log2 bits
  const float scale2 = scale * LOG2E;
  const float slope2 = slopes[h] * LOG2E;

  constexpr int KS = D / 16;
  constexpr int DB = D / 32;

  bf16x8 q_frag[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s)
    q_frag[s] = ok ? *reinterpret_cast<const bf16x8*>(
                         &qkv[base + (long)qi * QS + s * 16 + 8 * hi])
                   : bf16x8{};

  float m_run = NEG_INF, l_run = 0.f;
  f32x16 o_acc[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d) o_acc[d] = f32x16{};

  // keys of this block: cache rows [0, kv_end), all written (the append
  // kernel ran before on the stream); staging clamps later rows to kv_end-1
  const int kv_end = st + min(n, q0 + QROWS);
  attn::glds_stage<D, NT / 64>(kc, cbase, D, 0, kv_end, lds0);
  attn::glds_stage<D, NT / 64>(vc, cbase, D, 0, kv_end, lds0 + TB * 128);
  for (int kt = 0; kt < kv_end; kt += TB) {
    const int cur = (kt / TB) & 1;
    const uint16_t* k_lds = lds0 + (cur ? 2 * TB * 128 : 0);
    const uint16_t* v_lds = lds0 + TB * 128 + (cur ? 2 * TB * 128 : 0);
    // one barrier per tile: waits this wave's LDS-DMA (vmcnt(0)) and protects
    // the buffer the next prefetch overwrites
    attn::tile_barrier<0>();
    if (kt + TB < kv_end) {
      uint16_t* nxt = lds0 + (cur ? 0 : 2 * TB * 128);
      attn::glds_stage<D, NT / 64>(kc, cbase, D, kt + TB, kv_end, nxt);
      attn::glds_stage<D, NT / 64>(vc, cbase, D, kt + TB, kv_end, nxt + TB * 128);
    }
    if (qw >= n) continue;  // a wave of dead rows only keeps the barriers

#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const int kt32 = kt + sub * 32;
      if (kt32 > pw + 31 || kt32 >= kv_end) continue;  // fully masked for this wave

      // ---- S^T tile: C[i=key][j=q] = mfma(A=K, B=Q^T) ----
      f32x16 s_acc{};
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int kk = s * 16 + 8 * hi;
        const int krow = sub * 32 + li;
        bf16x8 a_frag = *reinterpret_cast<const bf16x8*>(
            (char*)k_lds + swz(krow, krow * 256 + kk * 2));
        s_acc = mfma16<F16>(a_frag, q_frag[s], s_acc);
      }

      // ---- in-lane softmax for q row `qi`; reg r holds key kt32+crow(r,hi),
      // log2 domain. The mask (causal, dead row) is evaluated only where the
      // sub-tile can reach it: wave-uniform test. ----
      float sv_[16];
      float tile_max = NEG_INF;
      if (kt32 + 31 <= pw && qw + 31 < n) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kj = kt32 + attn::crow(r, hi);
          sv_[r] = s_acc[r] * scale2 + slope2 * (float)(kj - pi);
          tile_max = fmaxf(tile_max, sv_[r]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kj = kt32 + attn::crow(r, hi);
          float x = s_acc[r] * scale2 + slope2 * (float)(kj - pi);
          if (kj > pi || !ok) x = NEG_INF;
          sv_[r] = x;
          tile_max = fmaxf(tile_max, x);
        }
      }
      tile_max = fmaxf(tile_max, __shfl_xor(tile_max, 32, 64));

      // defer-max with threshold (T13), as in flash_fwd_kernel
      float alpha = 1.f;
      const bool valid = tile_max > 0.5f * NEG_INF;
      if (!__all(tile_max <= m_run + DEFER_THR)) {
        const float mn = valid ? fmaxf(m_run, tile_max) : m_run;
        alpha = (m_run > 0.5f * NEG_INF) ? exp2f(m_run - mn) : (valid ? 0.f : 1.f);
        m_run = mn;
      }
      float p[16];
      float row_sum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p[r] = (valid && m_run > 0.5f * NEG_INF) ? exp2f(sv_[r] - m_run) : 0.f;
        row_sum += p[r];
      }
      row_sum += __shfl_xor(row_sum, 32, 64);
      l_run = l_run * alpha + row_sum;

      // ---- rescale O by alpha of each reg's q row (broadcast via shfl) ----
      if (!__all(alpha == 1.f)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float ar = __shfl(alpha, attn::crow(r, hi), 64);
#pragma unroll
          for (int d = 0; d < DB; ++d) o_acc[d][r] *= ar;
        }
      }

      // ---- P -> element-type A-fragments in-register (T12) ----
      bf16x8 pa[2];
      p_to_a_frags<F16>(p, pa);

      // ---- O += P @ V : V^T B-fragments via pipelined tr-reads ----
      attn::TrPair vp[2];
      attn::tr_pair_issue(v_lds, sub * 32, 0, &vp[0]);
#pragma unroll
      for (int d = 0; d < DB; ++d) {
        if (d + 1 < DB) attn::tr_pair_issue(v_lds, sub * 32, (d + 1) * 32, &vp[(d + 1) & 1]);
        attn::TrPair& t = vp[d & 1];
        if (d + 1 < DB)
          attn::tr_pair_wait<4>(&t);
        else
          attn::tr_pair_wait<0>(&t);
        o_acc[d] = mfma16<F16>(pa[0], t.a, o_acc[d]);
        o_acc[d] = mfma16<F16>(pa[1], t.b, o_acc[d]);
      }
    }
  }

  // ---- epilogue: O normalised in registers (1/l of row crow(r,hi) lives in
  // that lane), written in the element type into this wave's 32-row x D
  // slice of the idle K/V buffers and stored as whole rows, 16 B per lane;
  // rows >= n leave as zeros. ----
  const float inv_l = l_run > 0.f ? 1.f / l_run : 0.f;
  __syncthreads();  // every wave is done with the last K/V tile
  char* ot = smem + wave * (32 * D * 2);
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    const int row0 = attn::crow(r, hi);  // r even: row(r+1) = row0 + 1
    const float il0 = __shfl(inv_l, row0, 64);
    const float il1 = __shfl(inv_l, row0 + 1, 64);
#pragma unroll
    for (int d = 0; d < DB; ++d) {
      const unsigned w = pack2<F16>(o_acc[d][r] * il0, o_acc[d][r + 1] * il1);
      uint16_t* dst = (uint16_t*)(ot + row0 * (D * 2)) + d * 32 + li;
      dst[0] = (uint16_t)w;
      dst[D] = (uint16_t)(w >> 16);
    }
  }
  // same-wave LDS write -> read: DS ops of one wave execute in order
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int c = 0; c < 32 * LPR / 64; ++c) {
    const int idx = c * 64 + lane;
    const int row = idx / LPR, col = (idx % LPR) * 8;
    const s16x8 v8 = *reinterpret_cast<const s16x8*>(ot + row * (D * 2) + col * 2);
    if (qw + row < T)
      *reinterpret_cast<s16x8*>(&o[obase + (long)(qw + row) * C + col]) =
          qw + row < n ? v8 : s16x8{};
  }
}

// 128 q rows per block (four waves). Measured against 64 and 256 rows at the
// 1.3B head shape (H 16, D 128, fp16; profiles/PERF.md "Native prefill"):
// 256 rows lose at batch 1 (T 1024: 72 vs 59 us, T 2048: 136 vs 111 us per
// call), 64 rows lose at batch 16 T 1024 (337 vs 225 us) and at batch 1
// T 2048 (128 vs 111 us); at T 128 the three are within 2 %.
constexpr int PREFILL_NT = 256;

// Split-S decode, second kernel: grid B*H, one wave. Merges the `splits`
// partials {m, l, acc[64 * DPL]} of its (b, h), normalises and writes out;
// an empty split's partial (m = NEG_INF) has weight 0.
template <int DPL, bool F16>
__global__ __launch_bounds__(64) void attn_decode_merge_kernel(
    const float* __restrict__ part, uint16_t* __restrict__ out, int D, int splits) {
  const int bh = blockIdx.x;
  const int lane = threadIdx.x;
  const float* base = &part[(long)bh * splits * (2 + 64 * DPL)];
  float mg = NEG_INF;
  for (int s = 0; s < splits; ++s) mg = fmaxf(mg, base[s * (2 + 64 * DPL)]);
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
