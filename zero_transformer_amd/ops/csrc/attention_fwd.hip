// Fused causal ALiBi flash attention forward for gfx950 (CDNA4 MFMA).
//
// Replaces the reference's dense O(T^2) materialized attention
// (layers.py:159-178: q@k^T, +alibi, tril mask, fp32 softmax, dropout, @v)
// with a flash-style online-softmax kernel; softmax statistics stay fp32 end
// to end (the bf16-softmax failure of logs/580.md:94-98 cannot happen by
// construction). ALiBi is the true bias slope*(j-i) (shift-equivalent to the
// reference's single-row mask, layers.py:33-44). Dropout uses a counter RNG
// so backward regenerates the identical mask without storing it.
//
// Structure (the CDNA4 guide's swapped-QK^T recipe, §B attention), shared by
// both kernels in this file:
//   * 8 waves/block, each owning 32 q rows (QB = 256); K/V staged per
//     64-key tile into double-buffered row-major XOR-swizzled (T2) LDS
//     images by direct LDS-DMA (global_load_lds_dwordx4, attn::glds_stage):
//     the next tile's DMA issues while this tile computes, one barrier per
//     tile and no staging registers.
//   * QK^T is computed SWAPPED — mfma(A=K, B=Q^T) — so the C column index
//     is the q row: each lane holds a full P-row segment in registers and
//     the softmax row-reduce is in-lane + one exchange with lane^32, with
//     scalar running m/l. No P round-trip through LDS: P -> bf16
//     A-fragments via v_cvt_pk_bf16_f32 + v_permlane32_swap (T12).
//   * PV B-fragments (V^T) via ds_read_b64_tr_b16 hardware transpose reads
//     of the row-major V tile (T10) — no transposed staging copy.
//   * defer-max (T13): the O rescale is skipped while the tile max stays
//     within DEFER_THR bits of the running max; log2-domain scores.
//
// Two kernels:
//   flash_fwd_kernel<D, 512, 2>   the round-1 kernel. Every head dim below
//     128, and head dim 128 under ZTA_FWD_V1=1 (in-process A/B arm).
//   flash_fwd_v2_kernel<128, DROP> the default at head dim 128. The kernel
//     was issue-bound (two waves per SIMD, each ~44 % ACTIVE_INST, 432 VALU
//     per 16 MFMA); it does the same arithmetic with ~83 VALU per 16 MFMA
//     (~154 with dropout) — table in profiles/PERF.md:
//       - a padding row (qi >= T) computes row T-1 and is never stored, so
//         the running max is finite after the first tile and no `valid`
//         select guards the exponentials; raw v_exp_f32, a masked score of
//         -3e38 gives exactly 0;
//       - the causal / T mask is evaluated only on tiles that touch the
//         wave's diagonal or the tail (wave-uniform test, two score bodies);
//       - scale + ALiBi is one FMA per element with a wave-uniform addend;
//         the per-lane part of the bias joins the exponent offset (lb - m);
//       - dropout is a template parameter (no hash at p = 0), its 1/(1-p)
//         is applied once in the epilogue;
//       - ONE max / defer / rescale decision per staged 64-key tile, both S
//         tiles live; l accumulates per half-wave, the halves add at the end;
//       - LDS addresses are a lane constant + DS immediates
//         (attn::tr_pair_issue_imm), K fragments of sub-tile 1 load under
//         sub-tile 0's MFMAs;
//       - O is normalised in registers, staged as bf16 through the idle K/V
//         buffers and stored as whole rows, 16 B per lane (was 64
//         global_store_short per lane).
//     Not done: a hand-placed overlap of softmax with the matrix pipe
//     (T15 / sm-split) — the compiler's own schedule already runs sub-tile
//     1's exponentials between sub-tile 0's P.V MFMAs; nothing beyond that
//     was measured. The soft-max diet and the epilogue were measured
//     together, not one after the other.
//     Head dims 32/64/96 are NOT routed to it: the template compiles for
//     them with no spills and 32 and 96 match the reference, but at head
//     dim 64 without dropout the rows held by lanes 0-31 of the O
//     accumulator came out wrong (lse exact, dropout variant exact). The
//     cause was not found, so those head dims keep the round-1 kernel.
//     One codegen trap was found on the way and is padded by hand
//     (mfma_settle): inline-asm VALU readers of MFMA results get no hazard
//     wait states from the compiler.
//
// Fragment maps (gfx950, §3): A: lane l holds A[i=l%32][k=8*(l/32)+e];
// B: B[k=8*(l/32)+e][j=l%32]; C/D: col=lane&31, row=(reg&3)+8*(reg>>2)+4*(lane>>5).

#include "attn_tiles.h"
#include "common.h"

#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <type_traits>
#include <utility>

namespace {

using attn::NW;
using attn::RB;
using attn::TB;
using attn::swz;

constexpr float NEG_INF = -3.0e38f;

// qkv is the fused projection output (B, T, 3C) with C = H*D (q at column
// offset h*D, k at C + h*D, v at 2C + h*D); o is (B, T, C). This is the
// natural layout of the model's single qkv GEMM — no transposes or
// .contiguous() copies on either side of the op.
template <int D, int NT, int MINW>
__global__ __launch_bounds__(NT, MINW) void flash_fwd_kernel(
    const uint16_t* __restrict__ qkv, const float* __restrict__ slopes,
    uint16_t* __restrict__ o, float* __restrict__ lse, int H, int T, int C,
    float scale, float p_drop, uint32_t seed) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // double-buffered LDS-DMA staging: layout [k0 | v0 | k1 | v1]
  uint16_t* lds0 = (uint16_t*)smem;

  const int bh = blockIdx.x;  // grid: (BH, tiles) — consecutive blocks share the
  // tile index so per-CU work is balanced across the causal triangle
  const auto [h, QS, base, kbase, vbase, obase] = attn::planes<D>(bh, H, T, C);
  constexpr int RBX = NT / 2;  // NT=512: 256 q rows; NT=256: 128 q rows
  const int q0 = blockIdx.y * RBX;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int li = lane & 31;
  const int hi = lane >> 5;
  const int qw = q0 + wave * 32;
  const int qi = qw + li;  // THIS lane's q row (swapped layout)
  const float slope = slopes[h];
  // log2-domain softmax constants (see the softmax block below)
  constexpr float LOG2E = 1.4426950408889634f;
  constexpr float LN2 = 0.6931471805599453f;
  constexpr float DEFER_THR = 11.5f;  // ~8 nats in log2 bits
  const float scale2 = scale * LOG2E;
  const float slope2 = slope * LOG2E;
  const uint32_t drop_thr = attn::drop_thr(p_drop);
  const float inv_keep = attn::drop_inv_keep(drop_thr);

  constexpr int KS = D / 16;
  constexpr int DB = D / 32;

  // Q fragments (B operand of the swapped QK^T): lane l holds
  // Q[qw + l%32][8*(l/32) + e] per k-step — a 16 B row-major load.
  bf16x8 q_frag[KS];
  {
    const bool ok = qi < T;
#pragma unroll
    for (int s = 0; s < KS; ++s)
      q_frag[s] = ok ? *reinterpret_cast<const bf16x8*>(
                           &qkv[base + (long)qi * QS + s * 16 + 8 * hi])
                     : bf16x8{};
  }

  float m_run = NEG_INF, l_run = 0.f;
  f32x16 o_acc[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d) o_acc[d] = f32x16{};

  if (NT == 512 && __builtin_amdgcn_readfirstlane(threadIdx.x) >= 256)
    __builtin_amdgcn_s_setprio(1);  // static priority for the younger half (T5)

  attn::glds_stage<D, NT / 64>(qkv, kbase, QS, 0, T, lds0);
  attn::glds_stage<D, NT / 64>(qkv, vbase, QS, 0, T, lds0 + TB * 128);
  const int kv_end = min(T, q0 + RBX);
  for (int kt = 0; kt < kv_end; kt += TB) {
    const int cur = (kt / TB) & 1;
    const uint16_t* k_lds = lds0 + (cur ? 2 * TB * 128 : 0);
    const uint16_t* v_lds = lds0 + TB * 128 + (cur ? 2 * TB * 128 : 0);
    // one barrier per tile: waits in-flight LDS-DMA and protects the
    // buffer the next prefetch overwrites
    __syncthreads();
    attn::lds_acquire();
    if (kt + TB < kv_end) {
      uint16_t* nxt = lds0 + (cur ? 0 : 2 * TB * 128);
      attn::glds_stage<D, NT / 64>(qkv, kbase, QS, kt + TB, T, nxt);
      attn::glds_stage<D, NT / 64>(qkv, vbase, QS, kt + TB, T, nxt + TB * 128);
    }

#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const int kt32 = kt + sub * 32;
      if (kt32 > qw + 31 || kt32 >= T) continue;  // fully masked for this wave

      // ---- S^T tile: C[i=key][j=q] = mfma(A=K, B=Q^T) ----
      f32x16 s_acc{};
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int kk = s * 16 + 8 * hi;
        const int krow = sub * 32 + li;
        bf16x8 a_frag = *reinterpret_cast<const bf16x8*>(
            (char*)k_lds + swz(krow, krow * 256 + kk * 2));
        s_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_frag, q_frag[s], s_acc, 0, 0, 0);
      }

      // ---- in-lane softmax for q row `qi`; reg r holds key kt32+crow(r,hi).
      // Scores are folded into the log2 domain (scale2/slope2 pre-multiplied
      // by log2(e)) so the exponentials are raw v_exp_f32 (exp2f) with no
      // hidden per-element multiply; m/l run in log2 space and the lse
      // converts back at the epilogue. ----
      float sv_[16];
      float tile_max = NEG_INF;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kj = kt32 + attn::crow(r, hi);
        float x = s_acc[r] * scale2 + slope2 * (float)(kj - qi);
        if (kj > qi || kj >= T || qi >= T) x = NEG_INF;
        sv_[r] = x;
        tile_max = fmaxf(tile_max, x);
      }
      tile_max = fmaxf(tile_max, __shfl_xor(tile_max, 32, 64));

      // defer-max with threshold (T13): keep the stale m while the tile max
      // is within DEFER_THR bits — p stays <= 2^DEFER_THR (fp32-safe) and
      // the O-rescale is skipped far more often on the rising ALiBi scores.
      float alpha = 1.f;
      const bool valid = tile_max > 0.5f * NEG_INF;
      if (!__all(tile_max <= m_run + DEFER_THR)) {
        const float mn = valid ? fmaxf(m_run, tile_max) : m_run;
        // alpha = exp2(old_m - new_m); 0 when old_m was -inf (O, l still 0)
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

      // ---- dropout on the PV path (denominator keeps the full softmax) ----
      if (drop_thr) {
        const int bhT_qi = bh * T + qi;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int kbase = kt32 + 8 * g + 4 * hi;  // keys kbase..kbase+3 = regs 4g..4g+3
          const uint32_t bits = drop_bits32(seed, bhT_qi, kbase >> 2);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const bool keep = ((bits >> (8 * e)) & 0xffu) >= drop_thr;
            p[4 * g + e] = keep ? p[4 * g + e] * inv_keep : 0.f;
          }
        }
      }

      // ---- rescale O by alpha of each reg's q row (broadcast via shfl) ----
      if (!__all(alpha == 1.f)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float ar = __shfl(alpha, attn::crow(r, hi), 64);
#pragma unroll
          for (int d = 0; d < DB; ++d) o_acc[d][r] *= ar;
        }
      }

      // ---- P -> bf16 A-fragments in-register (T12) ----
      bf16x8 pa[2];
      attn::c_to_a_frags(p, pa);

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
        o_acc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[0], t.a, o_acc[d], 0, 0, 0);
        o_acc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[1], t.b, o_acc[d], 0, 0, 0);
      }
    }
  }

  // ---- epilogue: O rows are crow(r,hi); l/m live in the row's lane.
  // m_run is log2-domain: the stored lse converts back to natural log
  // (the backward kernels consume ln-domain lse). ----
  const float inv_l = l_run > 0.f ? 1.f / l_run : 0.f;
  if (hi == 0 && qi < T)
    lse[(long)bh * T + qi] = l_run > 0.f ? m_run * LN2 + __logf(l_run) : NEG_INF;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = attn::crow(r, hi);
    const int qr = qw + row;
    if (qr >= T) continue;
    const float il = __shfl(inv_l, row, 64);
#pragma unroll
    for (int d = 0; d < DB; ++d)
      o[obase + (long)qr * C + d * 32 + li] = f32_to_bf16(o_acc[d][r] * il);
  }
}

template <class F, int... I>
ZTA_DEV void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
// f(integral_constant<int, 0>) ... f(integral_constant<int, N-1>): the loop
// index is a constant expression (DS immediate offsets need one).
template <int N, class F>
ZTA_DEV void static_for(F&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

ZTA_DEV float as_f32(unsigned u) { return __builtin_bit_cast(float, u); }
ZTA_DEV unsigned as_u32(float f) { return __builtin_bit_cast(unsigned, f); }
// value of lane ^ 32 combined with the own value by `op` (one
// v_permlane32_swap, no LDS round trip)
ZTA_DEV float half_max(float x) {
  auto r = __builtin_amdgcn_permlane32_swap(as_u32(x), as_u32(x), false, false);
  return fmaxf(as_f32(r[0]), as_f32(r[1]));
}
// single v_add_f32: keeps the compiler from SLP-packing the exponent
// offsets into v_pk_add_f32, which is slower beside MFMAs than two adds
ZTA_DEV float add1(float a, float b) {
  float r;
  asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// single v_fma_f32 (same reason: no v_pk_fma_f32). Its first operand is an
// MFMA result: see mfma_settle.
ZTA_DEV float fma1(float a, float b, float c) {
  float r;
  asm("v_fma_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
// The compiler pads the MFMA-result -> VALU-read hazard only for readers it
// can see; inline-asm readers get no wait states (observed: wrong scores in
// the mask-free body, whose first instruction after the last QK^T MFMA is
// such a reader). 20 wait states cover the 16-pass case; every later asm
// reader depends on this statement through the "+v" operands.
ZTA_DEV void mfma_settle(f32x16& a, f32x16& b) {
  asm volatile("s_nop 15\n\ts_nop 3" : "+v"(a), "+v"(b));
}
ZTA_DEV float half_sum(float x) {
  auto r = __builtin_amdgcn_permlane32_swap(as_u32(x), as_u32(x), false, false);
  return as_f32(r[0]) + as_f32(r[1]);
}

// Default forward at head dim 128 (see the file header): same tiling,
// staging and fragment maps as flash_fwd_kernel<D, 512, 2>; the per-element
// softmax work is cut down, the dropout path is a template parameter and O
// leaves through LDS.
template <int D, bool DROP>
__global__ __launch_bounds__(512, 2) void flash_fwd_v2_kernel(
    const uint16_t* __restrict__ qkv, const float* __restrict__ slopes,
    uint16_t* __restrict__ o, float* __restrict__ lse, int H, int T, int C,
    float scale, float p_drop, uint32_t seed) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint16_t* lds0 = (uint16_t*)smem;  // [k0 | v0 | k1 | v1], 16 KiB each

  const int bh = blockIdx.x;
  const auto [h, QS, base, kbase, vbase, obase] = attn::planes<D>(bh, H, T, C);
  const int q0 = blockIdx.y * RB;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int li = lane & 31;
  const int hi = lane >> 5;
  const int qw = q0 + wave * 32;
  const int qi = qw + li;
  // A padding row (qi >= T) does the arithmetic of row T-1 and is never
  // stored: every row then sees key 0 in its first sub-tile, the running
  // max is finite from there on and no select guards the exponentials.
  const int qc = min(qi, T - 1);
  constexpr float LOG2E = 1.4426950408889634f;
  constexpr float LN2 = 0.6931471805599453f;
  constexpr float DEFER_THR = 11.5f;  // ~8 nats in log2 bits
  const float scale2 = scale * LOG2E;
  const float slope2 = slopes[h] * LOG2E;
  const uint32_t drop_thr = attn::drop_thr(p_drop);

  constexpr int KS = D / 16;
  constexpr int DB = D / 32;

  // ALiBi: the score of key kt + 32u + crow0(r) + 4*hi for row qc is
  //   s*scale2 + slope2*crow0(r)  +  slope2*(kt + 32u + 4*hi - qc)
  // = one FMA with a wave-uniform constant + a per-lane, per-sub-tile term
  // that is folded into the exponent offset (lb - m) below.
  float cst[16];
#pragma unroll
  for (int r = 0; r < 16; ++r)
    cst[r] = as_f32(__builtin_amdgcn_readfirstlane(
        as_u32(slope2 * (float)((r & 3) + 8 * (r >> 2)))));

  bf16x8 q_frag[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s)
    q_frag[s] = *reinterpret_cast<const bf16x8*>(
        &qkv[base + (long)qc * QS + s * 16 + 8 * hi]);

  float m_run = NEG_INF;
  float l_half = 0.f;  // this half-wave's keys only; halves add at the end
  f32x16 o_acc[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d) o_acc[d] = f32x16{};

  // dropout hash, row term: drop_bits32(seed, bh*T + qc, kg) =
  // mix32(hq ^ kg * 0x85ebca6b) (uint32 wrap arithmetic, bit-identical)
  const uint32_t hq = seed ^ ((uint32_t)(bh * T + qc) * 0x9e3779b9u);

  if (__builtin_amdgcn_readfirstlane(threadIdx.x) >= 256)
    __builtin_amdgcn_s_setprio(1);  // static priority for the younger half (T5)

  attn::glds_stage<D, NW>(qkv, kbase, QS, 0, T, lds0);
  attn::glds_stage<D, NW>(qkv, vbase, QS, 0, T, lds0 + TB * 128);
  const int kv_end = min(T, q0 + RB);
  for (int kt = 0; kt < kv_end; kt += TB) {
    const int cur = (kt / TB) & 1;
    __syncthreads();
    attn::lds_acquire();
    if (kt + TB < kv_end) {
      uint16_t* nxt = lds0 + (cur ? 0 : 2 * TB * 128);
      attn::glds_stage<D, NW>(qkv, kbase, QS, kt + TB, T, nxt);
      attn::glds_stage<D, NW>(qkv, vbase, QS, kt + TB, T, nxt + TB * 128);
    }
    if (kt > qw) continue;  // both sub-tiles above this wave's diagonal

    // Both 32-key sub-tiles are always computed: a sub-tile above the wave's
    // diagonal or past T is wholly masked (p = 0 exactly), which keeps the
    // MFMA / accumulator code free of branches (a branch around the
    // accumulation splits the accumulators' live ranges). Only the score
    // block has two forms: the wave-uniform interior test selects a body
    // without the causal / T mask (kj > qc covers kj >= T, qc <= T-1).
    //
    // lane-constant swizzle terms, recomputed per tile: K rows are li + 32u,
    // 16 B chunk (2s + hi) ^ (li & 7); bits 1-2 of s go through the XOR
    // (four addresses), everything else is a DS immediate.
    const char* kl = (const char*)lds0 + (cur ? 4 * TB * 128 : 0) + li * 256;
    const int kx = (16 * hi) ^ ((li & 7) << 4);
    const int vl = (int)(size_t)((const char*)lds0 + (cur ? 6 * TB * 128 : 2 * TB * 128)) +
                   attn::tr_lane_off(lane);

    // ---- S^T = K Q^T. The K fragments of sub-tile 0 are all in flight
    // before its first MFMA and those of sub-tile 1 load under sub-tile 0's
    // MFMAs (left alone, the compiler waits out each read's LDS latency right
    // before the MFMA that consumes it). ----
    auto k_frag = [&](int u, int s) {
      return *reinterpret_cast<const bf16x8*>(
          kl + (kx ^ ((s & 3) << 5)) + (s >> 2) * 128 + u * 32 * 256);
    };
    f32x16 s_acc[2] = {f32x16{}, f32x16{}};
    bf16x8 kf0[KS], kf1[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) kf0[s] = k_frag(0, s);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      kf1[s] = k_frag(1, s);
      s_acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf0[s], q_frag[s], s_acc[0], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < KS; ++s)
      s_acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf1[s], q_frag[s], s_acc[1], 0, 0, 0);
    mfma_settle(s_acc[0], s_acc[1]);

    // ---- scores (log2 domain, without the per-lane term lb) ----
    const int dl = qc - kt - 4 * hi;  // key offset c of this lane is live iff c <= dl
    float y[2][16];
    float mx[2] = {NEG_INF, NEG_INF};
    if (kt + 63 <= qw && kt + 63 < T) {
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          y[u][r] = fma1(s_acc[u][r], scale2, cst[r]);
          mx[u] = fmaxf(mx[u], y[u][r]);
        }
    } else {
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float x = fma1(s_acc[u][r], scale2, cst[r]);
          y[u][r] = (r & 3) + 8 * (r >> 2) + 32 * u > dl ? NEG_INF : x;
          mx[u] = fmaxf(mx[u], y[u][r]);
        }
    }
    const float lb0 = slope2 * (float)(-dl);
    const float lb1 = slope2 * (float)(32 - dl);
    // key kt <= qc is in the tile: the row max is finite
    const float tmax = half_max(fmaxf(mx[0] + lb0, mx[1] + lb1));

    // ---- ONE defer-max decision for the staged tile (T13): every P.V of
    // earlier tiles is complete, this tile's P is exponentiated after it.
    if (!__all(tmax <= m_run + DEFER_THR)) {
      const float mn = fmaxf(m_run, tmax);
      const float alpha = __builtin_amdgcn_exp2f(m_run - mn);  // 0 on the first tile
      m_run = mn;
      l_half *= alpha;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float ar = __shfl(alpha, attn::crow(r, hi), 64);
#pragma unroll
        for (int d = 0; d < DB; ++d) o_acc[d][r] *= ar;
      }
    }

    // ---- P = exp2(y + lb - m): raw v_exp_f32, a masked score gives 0 ----
    bf16x8 pa[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const float t = (u ? lb1 : lb0) - m_run;
      float p[16];
      float rs = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p[r] = __builtin_amdgcn_exp2f(add1(y[u][r], t));
        rs += p[r];
      }
      l_half += rs;  // the denominator keeps the full softmax
      if (DROP) {
        // keys kt + 32u + 8g + 4hi + e = regs 4g + e share one hash word;
        // the 1/(1-p) rescale is applied once, in the epilogue
        const uint32_t kg0 = (uint32_t)((kt >> 2) + 8 * u + hi) * 0x85ebca6bu;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const uint32_t bits = mix32(hq ^ (kg0 + (uint32_t)(2 * g) * 0x85ebca6bu));
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (((bits >> (8 * e)) & 0xffu) < drop_thr) p[4 * g + e] = 0.f;
        }
      }
      attn::c_to_a_frags(p, pa[u]);
    }

    // ---- O += P V: V^T B-fragments by pipelined transpose reads ----
    attn::TrPair vp[2];
    attn::tr_pair_issue_imm<0, 0>(vl, &vp[0]);
    static_for<2 * DB>([&](auto ic) {
      constexpr int i = decltype(ic)::value;
      constexpr int u = i / DB, d = i % DB;
      if constexpr (i + 1 < 2 * DB)
        attn::tr_pair_issue_imm<32 * ((i + 1) / DB), 32 * ((i + 1) % DB)>(vl, &vp[(i + 1) & 1]);
      attn::TrPair& tp = vp[i & 1];
      if constexpr (i + 1 < 2 * DB)
        attn::tr_pair_wait<4>(&tp);
      else
        attn::tr_pair_wait<0>(&tp);
      o_acc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[u][0], tp.a, o_acc[d], 0, 0, 0);
      o_acc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[u][1], tp.b, o_acc[d], 0, 0, 0);
    });
  }

  // ---- epilogue. lse: m is log2-domain, the stored value is ln-domain.
  // O: normalised in registers (1/l of row crow(r,hi) lives in that lane),
  // written as bf16 into this wave's 32-row x D slice of the idle K/V
  // buffers and stored as whole rows, 16 B per lane. ----
  const float l_run = half_sum(l_half);
  if (hi == 0 && qi < T) lse[(long)bh * T + qi] = m_run * LN2 + __logf(l_run);
  float inv_l = 1.f / l_run;
  if (DROP) inv_l *= 256.0f / (256.0f - (float)drop_thr);

  __syncthreads();  // every wave is done with the last K/V tile
  char* ot = smem + wave * (32 * D * 2);
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    const int row0 = attn::crow(r, hi);  // r even: row(r+1) = row0 + 1
    const float il0 = __shfl(inv_l, row0, 64);
    const float il1 = __shfl(inv_l, row0 + 1, 64);
#pragma unroll
    for (int d = 0; d < DB; ++d) {
      unsigned w;
      asm("v_cvt_pk_bf16_f32 %0, %1, %2"
          : "=v"(w)
          : "v"(o_acc[d][r] * il0), "v"(o_acc[d][r + 1] * il1));
      uint16_t* dst = (uint16_t*)(ot + row0 * (D * 2)) + d * 32 + li;
      dst[0] = (uint16_t)w;
      dst[D] = (uint16_t)(w >> 16);
    }
  }
  // same-wave LDS write -> read: DS ops of one wave execute in order
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  constexpr int LPR = D / 8;  // lanes (16 B each) per row
#pragma unroll
  for (int c = 0; c < 32 * LPR / 64; ++c) {
    const int idx = c * 64 + lane;
    const int row = idx / LPR, col = (idx % LPR) * 8;
    const s16x8 v8 = *reinterpret_cast<const s16x8*>(ot + row * (D * 2) + col * 2);
    if (qw + row < T)
      *reinterpret_cast<s16x8*>(&o[obase + (long)(qw + row) * C + col]) = v8;
  }
}

template <int D>
void launch_fwd(const at::Tensor& qkv, const at::Tensor& slopes, at::Tensor& o,
                at::Tensor& lse, int B, int H, int T, int C, float scale,
                float p_drop, uint32_t seed, hipStream_t stream) {
  const size_t smem = 4 * TB * 128 * sizeof(uint16_t);  // 2 tensors x 2 buffers
  // ZTA_FWD_V1=1: the round-1 kernel (in-process A/B arm and fallback).
  // Head dims below 128 stay on it: see the file header.
  static const bool v1 = [] {
    const char* e = getenv("ZTA_FWD_V1");
    return e && e[0] == '1';
  }();
  dim3 grid(B * H, (T + RB - 1) / RB);
  auto k = flash_fwd_kernel<D, 512, 2>;
  if constexpr (D == 128) {
    if (!v1)
      k = attn::drop_thr(p_drop) ? flash_fwd_v2_kernel<D, true>
                                             : flash_fwd_v2_kernel<D, false>;
  }
  hipLaunchKernelGGL(k, grid, dim3(512), smem, stream,
                     (const uint16_t*)qkv.data_ptr(), slopes.data_ptr<float>(),
                     (uint16_t*)o.data_ptr(), lse.data_ptr<float>(), H, T, C,
                     scale, p_drop, seed);
}

}  // namespace

std::vector<at::Tensor> attn_fwd(at::Tensor qkv, at::Tensor slopes, int64_t H_,
                                 double p_drop, int64_t seed) {
  TORCH_CHECK(qkv.is_cuda() && qkv.is_contiguous() && qkv.dim() == 3,
              "qkv must be (B, T, 3C) contiguous");
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16, "attn_fwd: bf16 only");
  const int B = qkv.size(0), T = qkv.size(1), H = (int)H_;
  const int C = qkv.size(2) / 3;
  TORCH_CHECK(qkv.size(2) == 3 * C && C % H == 0, "bad qkv shape");
  const int D = C / H;
  auto o = at::empty({B, T, C}, qkv.options());
  auto lse = at::empty({B, H, T}, qkv.options().dtype(at::kFloat));
  auto sl = slopes.to(at::kFloat).contiguous();
  const float scale = 1.0f / sqrtf((float)D);
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const bool ok = attn::with_head_dim(D, [&](auto d) {
    launch_fwd<decltype(d)::value>(qkv, sl, o, lse, B, H, T, C, scale, (float)p_drop,
                                   (uint32_t)seed, stream);
  });
  TORCH_CHECK(ok, "attn_fwd: head_dim must be one of 32/64/96/128, got ", D);
  return {o, lse};
}
