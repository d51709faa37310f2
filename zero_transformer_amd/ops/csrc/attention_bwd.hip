// Flash attention backward for gfx950 (CDNA4 MFMA) with P recomputed from
// the saved per-row LSE — no O(T^2) tensor is ever materialized (the
// reference's autograd attention backward re-materializes the dense probs;
// SURVEY.md §2.3 "Backward of all above"). Two schemes, three flash kernels
// (flash_bwd_fused_kernel | flash_dq_kernel + flash_dkdv4_kernel), all after
// the delta kernel:
//
// FUSED (head_dim 128, the default there): delta kernel, then ONE
// key-stationary kernel (flash_bwd_fused_kernel) that computes S and dP
// once and forms all of dV, dK and dQ from them — five MFMA products per
// tile pair instead of the two-kernel scheme's seven, one softmax / dropout
// regeneration instead of two. dQ is summed across the key blocks of a
// (b, h) with no-return f32 atomics into an f32 scratch (zeroed per call),
// then converted to bf16 into the q columns of dqkv. Everything runs on the
// caller's stream. f32 atomics make dQ differ in the last bits from run to
// run; dK and dV are bitwise reproducible.
//
// TWO-KERNEL (all head dims; bitwise reproducible): the FA2-style dQ and
// dKdV kernels below, which write disjoint columns of dqkv and run
// concurrently, dQ on the caller's stream and dKdV on a side stream.
// ZTA_BWD_FUSED=0 selects it process-wide, ZTA_BWD_FUSED=1 the fused scheme;
// the binding's trailing `fused` argument (-1 default / 0 / 1) selects per
// call. Head dims other than 128 always take the two-kernel path.
//
//   delta[b,h,i] = sum_d dO * O                  (delta kernel)
//   dQ kernel : per 256-row Q block (8 waves x 32 rows), loop 64-key tiles:
//       S^T = K Q^T, dP^T = V dO^T   (swapped MFMA: C[i=key][j=q], so each
//       lane owns one q row — lse/delta are lane scalars),
//       dS^T = sc * P^T (M∘dP^T/keep - delta),
//       dQ += dS K  with dS^T -> A-fragments fully in-register
//       (v_cvt_pk_bf16_f32 + v_permlane32_swap, same transform as the fwd)
//       and K^T B-fragments via ds_read_b64_tr_b16 hardware-transpose reads
//       of the row-major XOR-swizzled K tile (no transposed staging copy).
//   dKdV kernel: per 128-key KV block (4 waves x 32 keys, one wave per SIMD
//       with the whole register file: K/V resident in registers, no spills),
//       loop 64-row Q tiles:
//       S = Q K^T, dP = dO V^T       (C[i=q][j=key]: key is lane-resident),
//       dV += P^T dO, dK += sc*(dS^T) Q  with P^T / dS^T A-fragments
//       in-register and Q^T / dO^T B-fragments via tr-reads.
//
// The dropout mask M regenerates from the counter RNG (common.h
// drop_bits32) with the forward's seed. All softmax math fp32. Tile staging
// is direct LDS-DMA (global_load_lds_dwordx4, attn::glds_stage) into
// double-buffered swizzled images: the prefetch for tile t+1 issues right
// after tile t becomes visible, one barrier per tile.

#include "attn_tiles.h"
#include "common.h"

#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <type_traits>

namespace {

using attn::RB;
using attn::TB;
using attn::c_to_a_frags;
using attn::swz;

// log2-domain softmax recompute: p = exp2(s*scale2 + slope2*(j-i) - lse2)
// with scale2/slope2/lse2 pre-multiplied by log2(e) — raw v_exp_f32, no
// hidden per-element multiply (matches the forward's folded softmax).
constexpr float LOG2E = 1.4426950408889634f;
// Backward scheme when ZTA_BWD_FUSED is unset (see the file header).
constexpr bool BWD_FUSED_DEFAULT = true;

// ---------------------------------------------------------------------------
// dout/o are (B, T, C); delta is (B, H, T): row index r = (b*H + h)*T + t
// maps to plane offset (b*T + t)*C + h*D.
__global__ void delta_kernel(const uint16_t* __restrict__ dout,
                             const uint16_t* __restrict__ o,
                             float* __restrict__ delta, long rows, int H, int T,
                             int C, int D) {
  const int wid = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int nw = gridDim.x * blockDim.x / WAVE;
  for (long row = wid; row < rows; row += nw) {
    const long b = row / ((long)H * T);
    const int h = (int)((row / T) % H);
    const int t = (int)(row % T);
    const long off = (b * T + t) * C + h * D;
    float s = 0.f;
    for (int d = lane; d < D; d += WAVE)
      s += bf16_to_f32(dout[off + d]) * bf16_to_f32(o[off + d]);
    s = wave_reduce_sum(s);
    if (lane == 0) delta[row] = s;
  }
}

// Vectorized variant for D % 64 == 0 (the 64/128 head dims): 8 lanes per
// row (dwordx4 loads), 8 rows per wave, 3-shfl group reduce — the one-row-
// per-wave form above was latency-bound on its serial 6-shfl chain with
// scalar 2 B loads (~2.1 TB/s).
__global__ void delta_kernel_v8(const uint16_t* __restrict__ dout,
                                const uint16_t* __restrict__ o,
                                float* __restrict__ delta, long rows, int H,
                                int T, int C, int D) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int sub = lane & 7;    // lane within the row group
  const int rsub = lane >> 3;  // row within the wave's 8
  const long wid = ((long)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const long nw = (long)gridDim.x * blockDim.x / WAVE;
  const int dpl = D / 8;  // elements per lane, multiple of 8 by dispatch
  for (long r0 = wid * 8; r0 < rows; r0 += nw * 8) {
    const long row = r0 + rsub;
    float s = 0.f;
    if (row < rows) {
      const long b = row / ((long)H * T);
      const int h = (int)((row / T) % H);
      const int t = (int)(row % T);
      const long off = (b * T + t) * C + h * D + sub * dpl;
      for (int e = 0; e < dpl; e += 8) {
        s16x8 a = *reinterpret_cast<const s16x8*>(&dout[off + e]);
        s16x8 c = *reinterpret_cast<const s16x8*>(&o[off + e]);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          s += bf16_to_f32((uint16_t)a[j]) * bf16_to_f32((uint16_t)c[j]);
      }
    }
#pragma unroll
    for (int off8 = 4; off8 > 0; off8 >>= 1) s += __shfl_xor(s, off8, WAVE);
    if (sub == 0 && row < rows) delta[row] = s;
  }
}

// ---------------------------------------------------------------------------
// dQ kernel: 8 waves x 32 q rows = 256-row Q block; loop 64-key KV tiles.
// LDS: two buffers of k_lds 64x[256B] | v_lds 64x[256B], swizzled (64 KiB)
// ---------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(512, 2) void flash_dq_kernel(
    const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    const float* __restrict__ slopes, uint16_t* __restrict__ dqkv, int H, int T,
    int C, float scale, float p_drop, uint32_t seed) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // double-buffered LDS-DMA staging: layout [k0 | v0 | k1 | v1]
  uint16_t* lds0 = (uint16_t*)smem;

  const int bh = blockIdx.x;  // grid: (BH, tiles) for per-CU load balance
  const auto [h, QS, base, kbase, vbase, dobase] = attn::planes<D>(bh, H, T, C);
  const int q0 = blockIdx.y * RB;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int li = lane & 31, hi = lane >> 5;
  const int qw = q0 + wave * 32;
  const int qi = qw + li;  // this lane's q row
  const float slope = slopes[h];
  const float scale2 = scale * LOG2E;
  const float slope2 = slope * LOG2E;
  const uint32_t thr = attn::drop_thr(p_drop);
  const float inv_keep = attn::drop_inv_keep(thr);

  constexpr int KS = D / 16;
  constexpr int DB = D / 32;

  // Literal on purpose, like the epilogue store and their twins in
  // flash_dkdv4_kernel: shared helpers for either changed both kernels'
  // instruction schedules at every head dim (tools/kernel_isa.py).
  bf16x8 q_frag[KS], do_frag[KS];
  {
    const bool ok = qi < T;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      if (ok) {
        q_frag[s] = *reinterpret_cast<const bf16x8*>(&qkv[base + (long)qi * QS + s * 16 + 8 * hi]);
        do_frag[s] = *reinterpret_cast<const bf16x8*>(&dout[dobase + (long)qi * C + s * 16 + 8 * hi]);
      } else {
        q_frag[s] = bf16x8{};
        do_frag[s] = bf16x8{};
      }
    }
  }
  const float lse2_q = (qi < T ? lse[(long)bh * T + qi] : 0.f) * LOG2E;
  const float delta_q = qi < T ? delta[(long)bh * T + qi] : 0.f;

  f32x16 dq_acc[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d) dq_acc[d] = f32x16{};

  if (__builtin_amdgcn_readfirstlane(threadIdx.x) >= 256)
    __builtin_amdgcn_s_setprio(1);  // static priority for the younger half (T5)

  attn::glds_stage<D, 8>(qkv, kbase, QS, 0, T, lds0);
  attn::glds_stage<D, 8>(qkv, vbase, QS, 0, T, lds0 + TB * 128);
  const int kv_end = min(T, q0 + RB);
  for (int kt = 0; kt < kv_end; kt += TB) {
    const int cur = (kt / TB) & 1;
    const uint16_t* k_lds = lds0 + (cur ? 2 * TB * 128 : 0);
    const uint16_t* v_lds = lds0 + TB * 128 + (cur ? 2 * TB * 128 : 0);
    // ONE barrier per tile: waits this tile's in-flight LDS-DMA (vmcnt)
    // AND guarantees everyone is done reading the buffer the next
    // prefetch overwrites (last read two iterations ago).
    __syncthreads();
    attn::lds_acquire();
    if (kt + TB < kv_end) {
      uint16_t* nxt = lds0 + (cur ? 0 : 2 * TB * 128);
      attn::glds_stage<D, 8>(qkv, kbase, QS, kt + TB, T, nxt);
      attn::glds_stage<D, 8>(qkv, vbase, QS, kt + TB, T, nxt + TB * 128);
    }

#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const int kt32 = kt + sub * 32;
      if (kt32 > qw + 31 || kt32 >= T) continue;  // fully masked for this wave

      // S^T = K Q^T ; dP^T = V dO^T   (C[i=key][j=q], q = lane's row)
      f32x16 s_acc{}, dpt_acc{};
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int kk = s * 16 + 8 * hi;
        const int krow = sub * 32 + li;
        bf16x8 ka = *reinterpret_cast<const bf16x8*>((char*)k_lds + swz(krow, krow * 256 + kk * 2));
        bf16x8 va = *reinterpret_cast<const bf16x8*>((char*)v_lds + swz(krow, krow * 256 + kk * 2));
        s_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, q_frag[s], s_acc, 0, 0, 0);
        dpt_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, do_frag[s], dpt_acc, 0, 0, 0);
      }

      // dS^T[key][q] per register (key = kt32 + crow(r,hi), q = qi)
      float ds[16];
      if (thr) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int kbase = kt32 + 8 * g + 4 * hi;
          const uint32_t bits = drop_bits32(seed, bh * T + qi, kbase >> 2);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 4 * g + e;
            const int kj = kbase + e;
            float p = 0.f;
            if (!(kj > qi || kj >= T || qi >= T))
              p = exp2f(s_acc[r] * scale2 + slope2 * (float)(kj - qi) - lse2_q);
            const bool keep = ((bits >> (8 * e)) & 0xffu) >= thr;
            const float dp = keep ? dpt_acc[r] * inv_keep : 0.f;
            ds[r] = scale * p * (dp - delta_q);
          }
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kj = kt32 + attn::crow(r, hi);
          float p = 0.f;
          if (!(kj > qi || kj >= T || qi >= T))
            p = exp2f(s_acc[r] * scale2 + slope2 * (float)(kj - qi) - lse2_q);
          ds[r] = scale * p * (dpt_acc[r] - delta_q);
        }
      }

      bf16x8 dsa[2];
      c_to_a_frags(ds, dsa);  // A[i=q][k=key]

      // dQ += dS K : B[k=key][j=d] via pipelined tr-reads of the K tile
      attn::TrPair kp[2];
      attn::tr_pair_issue(k_lds, sub * 32, 0, &kp[0]);
#pragma unroll
      for (int d = 0; d < DB; ++d) {
        if (d + 1 < DB) attn::tr_pair_issue(k_lds, sub * 32, (d + 1) * 32, &kp[(d + 1) & 1]);
        attn::TrPair& t = kp[d & 1];
        if (d + 1 < DB)
          attn::tr_pair_wait<4>(&t);
        else
          attn::tr_pair_wait<0>(&t);
        dq_acc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dsa[0], t.a, dq_acc[d], 0, 0, 0);
        dq_acc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dsa[1], t.b, dq_acc[d], 0, 0, 0);
      }
    }
  }

  // epilogue: dQ rows crow(r,hi)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = attn::crow(r, hi);
    const int qr = qw + row;
    if (qr >= T) continue;
#pragma unroll
    for (int d = 0; d < DB; ++d)
      dqkv[base + (long)qr * QS + d * 32 + li] = f32_to_bf16(dq_acc[d][r]);
  }
}

// ---------------------------------------------------------------------------
// dKdV kernel: 4 waves x 32 keys = 128-key block; loop 64-row Q tiles.
// 256 threads, ONE wave per SIMD, whole register file per wave (no
// 2-waves/SIMD cap) — K/V resident AND no spills, at the cost of losing the
// partner wave's latency hiding. The 8-wave form it replaced spilled at head
// dims 96 and 128 (profiles/PERF.md).
// ---------------------------------------------------------------------------
constexpr int RB4 = 128;  // 4 waves x 32 keys

template <int D>
__global__ __launch_bounds__(256, 1) void flash_dkdv4_kernel(
    const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    const float* __restrict__ slopes, uint16_t* __restrict__ dqkv, int H, int T,
    int C, float scale, float p_drop, uint32_t seed) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // LDS-DMA double buffers [q0 | do0 | q1 | do1] + 2x (lse, delta) slices
  uint16_t* lds0 = (uint16_t*)smem;
  float* stats0 = (float*)(lds0 + 4 * TB * 128);

  const int bh = blockIdx.x;
  const auto [h, QS, base, kbase, vbase, dobase] = attn::planes<D>(bh, H, T, C);
  const int k0 = blockIdx.y * RB4;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int li = lane & 31, hi = lane >> 5;
  const int kw = k0 + wave * 32;
  const int kj = kw + li;
  const float slope = slopes[h];
  const float scale2 = scale * LOG2E;
  const float slope2 = slope * LOG2E;
  const uint32_t thr = attn::drop_thr(p_drop);
  const float inv_keep = attn::drop_inv_keep(thr);

  constexpr int KS = D / 16;
  constexpr int DB = D / 32;

  bf16x8 k_frag[KS], v_frag[KS];  // literal loop: see flash_dq_kernel
  {
    const bool ok = kj < T;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      if (ok) {
        k_frag[s] = *reinterpret_cast<const bf16x8*>(&qkv[kbase + (long)kj * QS + s * 16 + 8 * hi]);
        v_frag[s] = *reinterpret_cast<const bf16x8*>(&qkv[vbase + (long)kj * QS + s * 16 + 8 * hi]);
      } else {
        k_frag[s] = bf16x8{};
        v_frag[s] = bf16x8{};
      }
    }
  }

  f32x16 dk_acc[DB], dv_acc[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d) {
    dk_acc[d] = f32x16{};
    dv_acc[d] = f32x16{};
  }

  const int t256 = threadIdx.x;
  auto stage_stats = [&](int qt, float* dst) {
    // lse slice then delta slice, plain LDS stores (tiny)
    if (t256 < TB) {
      const int qg = qt + t256;
      dst[t256] = (qg < T ? lse[(long)bh * T + qg] : 0.f) * LOG2E;
      dst[TB + t256] = qg < T ? delta[(long)bh * T + qg] : 0.f;
    }
  };

  attn::glds_stage<D, 4>(qkv, base, QS, k0, T, lds0);
  attn::glds_stage<D, 4>(dout, dobase, C, k0, T, lds0 + TB * 128);
  stage_stats(k0, stats0);
  for (int qt = k0; qt < T; qt += TB) {
    const int cur = ((qt - k0) / TB) & 1;
    const uint16_t* q_lds = lds0 + (cur ? 2 * TB * 128 : 0);
    const uint16_t* do_lds = lds0 + TB * 128 + (cur ? 2 * TB * 128 : 0);
    const float* lse_s = stats0 + (cur ? 2 * TB : 0);
    const float* delta_s = lse_s + TB;
    __syncthreads();
    attn::lds_acquire();
    if (qt + TB < T) {
      uint16_t* nxt = lds0 + (cur ? 0 : 2 * TB * 128);
      attn::glds_stage<D, 4>(qkv, base, QS, qt + TB, T, nxt);
      attn::glds_stage<D, 4>(dout, dobase, C, qt + TB, T, nxt + TB * 128);
      stage_stats(qt + TB, stats0 + (cur ? 0 : 2 * TB));
    }

#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const int q32 = qt + sub * 32;
      if (q32 + 31 < kw || q32 >= T) continue;

      f32x16 s_acc{}, dp_acc{};
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int kk = s * 16 + 8 * hi;
        const int qrow = sub * 32 + li;
        bf16x8 qa = *reinterpret_cast<const bf16x8*>((char*)q_lds + swz(qrow, qrow * 256 + kk * 2));
        bf16x8 da = *reinterpret_cast<const bf16x8*>((char*)do_lds + swz(qrow, qrow * 256 + kk * 2));
        s_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa, k_frag[s], s_acc, 0, 0, 0);
        dp_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da, v_frag[s], dp_acc, 0, 0, 0);
      }

      // Pre-issue d-block 0's eight transpose reads so their LDS latency
      // hides under the softmax VALU below. The softmax's own lse_s /
      // delta_s loads are lgkm-counted and interleave with this group, so
      // the group is drained with a FULL lgkmcnt(0) wait after the
      // transforms (a counted wait would be unsafe here); d-blocks 1..3
      // keep the counted-wait pipeline (no interleaving DS ops there).
      attn::TrQuad qq[2];
      attn::tr_quad_issue(do_lds, q_lds, sub * 32, 0, &qq[0]);

      float p_pv[16], ds[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = attn::crow(r, hi);
        const int qi = q32 + row;
        const float lq = lse_s[sub * 32 + row];
        const float dq_ = delta_s[sub * 32 + row];
        const bool masked = kj > qi || kj >= T || qi >= T;
        const float x = masked ? -3.0e38f
                               : s_acc[r] * scale2 + slope2 * (float)(kj - qi) - lq;
        const float p = exp2f(x);
        float dp = dp_acc[r];
        float ppv = p;
        if (thr) {
          const uint32_t bits = drop_bits32(seed, bh * T + qi, kj >> 2);
          const bool keep = ((bits >> (8 * (kj & 3))) & 0xffu) >= thr;
          dp = keep ? dp * inv_keep : 0.f;
          ppv = keep ? p * inv_keep : 0.f;
        }
        p_pv[r] = ppv;
        ds[r] = scale * p * (dp - dq_);
      }

      bf16x8 pa[2], dsa[2];
      c_to_a_frags(p_pv, pa);
      c_to_a_frags(ds, dsa);

      attn::tr_quad_wait<0>(&qq[0]);  // full drain (see pre-issue note)
#pragma unroll
      for (int d = 0; d < DB; ++d) {
        if (d + 1 < DB)
          attn::tr_quad_issue(do_lds, q_lds, sub * 32, (d + 1) * 32, &qq[(d + 1) & 1]);
        attn::TrQuad& t = qq[d & 1];
        if (d > 0) {
          if (d + 1 < DB)
            attn::tr_quad_wait<8>(&t);
          else
            attn::tr_quad_wait<0>(&t);
        }
        dv_acc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[0], t.x.a, dv_acc[d], 0, 0, 0);
        dv_acc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[1], t.x.b, dv_acc[d], 0, 0, 0);
        dk_acc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dsa[0], t.y.a, dk_acc[d], 0, 0, 0);
        dk_acc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dsa[1], t.y.b, dk_acc[d], 0, 0, 0);
      }
    }
  }

#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = attn::crow(r, hi);
    const int kr = kw + row;
    if (kr >= T) continue;
#pragma unroll
    for (int d = 0; d < DB; ++d) {
      dqkv[kbase + (long)kr * QS + d * 32 + li] = f32_to_bf16(dk_acc[d][r]);
      dqkv[vbase + (long)kr * QS + d * 32 + li] = f32_to_bf16(dv_acc[d][r]);
    }
  }
}

// ---------------------------------------------------------------------------
// Fused backward (D = 128): one key-stationary kernel, five products per tile
// pair. A workgroup owns 256 keys of one (b, h): 4 waves x 64 keys (two
// 32-key lane groups), dK/dV accumulators and V fragments resident, and
// sweeps 32-row query slices from its first key to T. Per slice each wave
// computes S, dP, P and dS once for its keys, accumulates dV/dK as in
// flash_dkdv4_kernel, and drops dS (bf16 A-fragment words) into a shared
// [key][q] LDS tile. After an LDS-only barrier wave w forms the slice's dQ
// columns [32w, 32w+32) over all active keys of the block (A = transpose
// reads of the dS tile, B = transpose reads of the block's K image) and
// adds it into the f32 scratch with no-return atomics: one accumulator
// register is two 128 B row segments. No workgroup waits on another.
// Softmax: the lane's 16 rows of lse and delta are read once per slice as
// 4 + 4 16-byte LDS reads ahead of the MFMAs and shared by both key groups;
// lse * log2e and the row part of the ALiBi term fold into one row constant,
// the key part is one lane constant per group. Two variants, chosen per
// slice by a wave-uniform branch around the softmax only (as dropout on /
// off is): INTERIOR when every one of the wave's 64 keys is at or below
// every row of the slice and the slice lies below T (no compare, no select;
// at least 7 of 9 slices at T = 2048), MASKED for diagonal and tail slices (exponent
// computed unconditionally, then selected to 0: no divergent region).
// Dropout: the four lanes of a quad own four keys of one drop_bits32 word
// and the same 16 rows, so each hashes 4 of the 16 rows and the quad
// exchanges the words by DPP quad_perm; every lane keeps its own byte.
// LDS: K image 256x[256B] | q0 do0 q1 do1 32x[256B] | dS 2x 256x[64B] |
//      (lse, delta) 2x 64 f32 = 128.5 KiB. No vector-memory load inside the
// slice loop returns to a register (Q, dO, lse and delta all arrive by
// LDS-DMA): a register load would make the compiler wait on vmcnt, which
// retires in order and would drain the dQ atomics issued before it.
// Registers: the 256 dK/dV accumulators fill the accumulation file, so the
// transient S / dP / dQ tiles run through attn::mfma_sdp2 / mfma_quad_acc
// (arch-VGPR destinations). 256 + 256 registers, no scratch; re-check with
// -Rpass-analysis=kernel-resource-usage after any edit.
// ---------------------------------------------------------------------------
constexpr int FKB = 256;  // keys per fused-backward workgroup
constexpr int FQS = 32;   // query rows per slice
constexpr size_t FUSED_SMEM =
    (size_t)(FKB * 128 + 4 * FQS * 128 + 2 * FKB * 32) * sizeof(uint16_t) +
    4 * FQS * sizeof(float);

template <int D>
__global__ __launch_bounds__(256, 1) void flash_bwd_fused_kernel(
    const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    const float* __restrict__ slopes, uint16_t* __restrict__ dqkv,
    float* __restrict__ dq32, int H, int T, int C, float scale, float p_drop,
    uint32_t seed) {
  static_assert(D == 128, "fused backward covers head_dim 128 only");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint16_t* k_img = (uint16_t*)smem;
  uint16_t* lds0 = k_img + FKB * 128;        // [q0 | do0 | q1 | do1]
  uint16_t* ds0 = lds0 + 4 * FQS * 128;      // two [256 keys][32 q] dS tiles
  float* stats0 = (float*)(ds0 + 2 * FKB * 32);  // two [lse 32 | delta 32]

  const int bh = blockIdx.x;  // grid: (BH, key blocks), heaviest block first
  const auto [h, QS, base, kbase, vbase, dobase] = attn::planes<D>(bh, H, T, C);
  const int k0 = blockIdx.y * FKB;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int li = lane & 31, hi = lane >> 5;
  const int kw = k0 + wave * 64;  // this wave's first key
  const float slope = slopes[h];
  const float scale2 = scale * LOG2E;
  const float slope2 = slope * LOG2E;
  const uint32_t thr = attn::drop_thr(p_drop);
  const float inv_keep = attn::drop_inv_keep(thr);

  constexpr int KS = D / 16;
  constexpr int DB = D / 32;

  bf16x8 v_frag[2][KS];
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const int kj = kw + 32 * g + li;
#pragma unroll
    for (int s = 0; s < KS; ++s)
      v_frag[g][s] = kj < T ? *reinterpret_cast<const bf16x8*>(
                                  &qkv[vbase + (long)kj * QS + s * 16 + 8 * hi])
                            : bf16x8{};
  }

  f32x16 dk_acc[2][DB], dv_acc[2][DB];
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int d = 0; d < DB; ++d) {
      dk_acc[g][d] = f32x16{};
      dv_acc[g][d] = f32x16{};
    }

#pragma unroll
  for (int i = 0; i < FKB / TB; ++i)
    attn::glds_stage<D, 4>(qkv, kbase, QS, k0 + TB * i, T, k_img + i * TB * 128);
  attn::glds_stage<D, 4, FQS>(qkv, base, QS, k0, T, lds0);
  attn::glds_stage<D, 4, FQS>(dout, dobase, C, k0, T, lds0 + FQS * 128);
  if (wave == 0) attn::glds_stats32(lse, delta, (long)bh * T, k0, T, stats0);

  // Settle the V loads here: left pending into the loop, their first use
  // would carry a vmcnt(0) in every slice and drain the dQ atomics with it.
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int s = 0; s < KS; ++s) asm volatile("" : "+v"(v_frag[g][s]));

  const int kend64 = min(FKB, (T - k0 + 63) & ~63);  // keys of this block, /64 up
  float* const dq_col = dq32 + ((long)(bh / H) * T) * C + h * D + 32 * wave;

  // One loop over 32-row query slices, each staged one slice ahead into
  // the other (Q, dO, stats) buffer. A single loop body (no per-slice
  // specialization) keeps the 256 resident accumulators in one live range
  // each.
#pragma unroll 1
  for (int q32 = k0; q32 < T; q32 += FQS) {
    // Loop-local opaque lane id: LDS addresses derived from it are
    // recomputed per slice instead of being hoisted out of the loop, where
    // a few hundred lane constants would be spilled around it.
    int lv = lane;
    asm volatile("" : "+v"(lv));
    const int li = lv & 31, hi = lv >> 5;
    const int sl = (q32 - k0) >> 5;  // slice number within the block
    const int cur = sl & 1;
    const uint16_t* q_lds = lds0 + cur * (2 * FQS * 128);
    const uint16_t* do_lds = q_lds + FQS * 128;
    const float* lse_s = stats0 + cur * (2 * FQS);
    const float* delta_s = lse_s + FQS;
    uint16_t* ds_t = ds0 + cur * (FKB * 32);
    // slice-ready barrier: waits this slice's LDS-DMA (first time: all of
    // it, K image included) and frees the buffers the next prefetch
    // overwrites. Later slices leave the previous slice's dQ atomics in
    // flight: a slice that has a successor lies wholly below T, so each wave
    // issued exactly 16 atomic instructions after that DMA group.
    if (sl == 0)
      attn::tile_barrier<0>();
    else
      attn::tile_barrier<16>();
    if (q32 + FQS < T) {
      uint16_t* nxt = lds0 + (cur ^ 1) * (2 * FQS * 128);
      attn::glds_stage<D, 4, FQS>(qkv, base, QS, q32 + FQS, T, nxt, lv);
      attn::glds_stage<D, 4, FQS>(dout, dobase, C, q32 + FQS, T, nxt + FQS * 128, lv);
      if (wave == 0)
        attn::glds_stats32(lse, delta, (long)bh * T, q32 + FQS, T,
                           stats0 + (cur ^ 1) * (2 * FQS), lv);
    }

    // Every wave runs every slice, also the few diagonal slices that lie
    // wholly above its keys (they contribute p = 0): the waves meet at the
    // barrier below anyway, and a branch around the accumulation would
    // split the live ranges of the 256 resident accumulators.
    {
      // Key groups run one after the other through S/dP and the softmax
      // (scheduling fences keep the register peak at one group's worth);
      // K rows come from the K image, V fragments are resident.
      attn::TrQuad qq[2];
      bf16x8 pa[2][2], dsa[2][2];
      // Row statistics of the lane's 16 rows (four runs of four consecutive
      // floats), read once ahead of the MFMAs and shared by both key groups:
      // rowc = lse * log2e + slope2 * row (the row part of the ALiBi term
      // folded into the exponent's row constant) and delta.
      float rowc[16], dlt[16];
      {
        const float srow0 = slope2 * (float)(4 * hi);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f32x4 l4 = *reinterpret_cast<const f32x4*>(lse_s + 8 * j + 4 * hi);
          const f32x4 d4 = *reinterpret_cast<const f32x4*>(delta_s + 8 * j + 4 * hi);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            rowc[4 * j + i] = l4[i] * LOG2E + (slope2 * (float)(8 * j + i) + srow0);
            dlt[4 * j + i] = d4[i];
          }
        }
      }
      // No element of this wave's 64 keys x 32 rows is masked: every key is
      // at or below every row and the slice lies wholly below T.
      const bool interior = kw + 63 <= q32 && q32 + FQS <= T;
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        // S = Q K^T ; dP = dO V^T  (C[i=q][j=key])
        // (arch-VGPR accumulators: attn::mfma_sdp2, two k-steps a statement)
        f32x16 s_acc, dp_acc;
        const int krow = wave * 64 + g * 32 + li;
#pragma unroll
        for (int s4 = 0; s4 < KS; s4 += 2) {
          bf16x8 qa[2], da[2], kb[2];
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            const int kk = (s4 + s) * 16 + 8 * hi;
            qa[s] = *reinterpret_cast<const bf16x8*>((char*)q_lds + swz(li, li * 256 + kk * 2));
            da[s] = *reinterpret_cast<const bf16x8*>((char*)do_lds + swz(li, li * 256 + kk * 2));
            kb[s] = *reinterpret_cast<const bf16x8*>((char*)k_img + swz(krow, krow * 256 + kk * 2));
          }
          if (s4 == 0)
            attn::mfma_sdp2<true>(s_acc, dp_acc, qa, da, kb, &v_frag[g][s4]);
          else
            attn::mfma_sdp2<false>(s_acc, dp_acc, qa, da, kb, &v_frag[g][s4]);
        }
        __builtin_amdgcn_sched_barrier(0);

        // d-block 0's transpose reads hide under the last group's softmax;
        // drained with a full lgkmcnt(0) (compiler DS ops interleave here,
        // see flash_dkdv4_kernel).
        if (g == 1) attn::tr_quad_issue(do_lds, q_lds, 0, 0, &qq[0], lv);

        float p_pv[16], ds[16];
        const int kj = kw + 32 * g + li;
        // exponent = s*scale2 + slope2*(kj - qi) - lse2 with the ALiBi term
        // split as slope2*(kj - q32) (one lane constant per group, the
        // integer difference exact) minus the row part held in rowc.
        const int kd = kj - q32;
        const float akey = slope2 * (float)kd;
        auto softmax = [&](auto drop, auto mask) {
          // Row r = 4j + i of the lane is slice row 8j + i + 4*hi (literal
          // attn::crow, as at the dQ atomics and the epilogue below: with the
          // helper the same values come out of a different instruction
          // schedule, which nobody has timed).
          // Masked variant: row is masked iff kj > qi, kj >= T or qi >= T,
          // i.e. 8j + i < mlo or 8j + i >= mhi with the lane's 4*hi taken out.
          const int mlo = (kj < T ? kd : 2 * FQS) - 4 * hi;
          const int mhi = T - q32 - 4 * hi;
          // Dropout: the four lanes of a quad hold four keys of one key quad
          // and the same 16 rows, so they need the same 16 drop_bits32 words
          // and each keeps another byte. Quad lane ql hashes the rows of run
          // j = ql; every lane then takes run j's words from quad lane j by
          // DPP. The row term is formed incrementally (uint32 wrap
          // arithmetic, bit-identical): (bh*T + q32 + row) * 0x9e3779b9.
          uint32_t hq[4] = {};
          const int kshift = 8 * (lv & 3);  // = 8 * (kj & 3)
          if (decltype(drop)::value) {
            const uint32_t hrow =
                (uint32_t)(bh * T + q32 + 4 * hi + 8 * (lv & 3)) * 0x9e3779b9u;
            const uint32_t hkey = seed ^ ((uint32_t)(kj >> 2) * 0x85ebca6bu);
#pragma unroll
            for (int i = 0; i < 4; ++i) hq[i] = mix32(hkey ^ (hrow + (uint32_t)i * 0x9e3779b9u));
          }
          auto run = [&](auto jc) {
            constexpr int j = decltype(jc)::value;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int r = 4 * j + i;
              const float x = (s_acc[r] * scale2 + akey) - rowc[r];
              float p = __builtin_amdgcn_exp2f(x);  // raw v_exp_f32
              if (decltype(mask)::value) {
                // computed unconditionally, then selected: no divergent region
                const bool masked = 8 * j + i < mlo || 8 * j + i >= mhi;
                p = masked ? 0.f : p;
              }
              float dp = dp_acc[r];
              float ppv = p;
              if (decltype(drop)::value) {
                const uint32_t bits = (uint32_t)__builtin_amdgcn_update_dpp(
                    0, (int)hq[i], j * 0x55 /* quad_perm:[j,j,j,j] */, 0xf, 0xf, true);
                const bool keep = ((bits >> kshift) & 0xffu) >= thr;
                dp = keep ? dp * inv_keep : 0.f;
                ppv = keep ? p * inv_keep : 0.f;
              }
              p_pv[r] = ppv;
              ds[r] = scale * p * (dp - dlt[r]);
            }
          };
          run(std::integral_constant<int, 0>{});
          run(std::integral_constant<int, 1>{});
          run(std::integral_constant<int, 2>{});
          run(std::integral_constant<int, 3>{});
        };
        // Wave-uniform branches around the softmax only (never around an
        // accumulation): dropout on / off, masked / interior.
        if (thr) {
          if (interior)
            softmax(std::true_type{}, std::false_type{});
          else
            softmax(std::true_type{}, std::true_type{});
        } else {
          if (interior)
            softmax(std::false_type{}, std::false_type{});
          else
            softmax(std::false_type{}, std::true_type{});
        }
        c_to_a_frags(p_pv, pa[g]);  // A[i=key][k=q]
        c_to_a_frags(ds, dsa[g]);
        // the same words are the dS tile's [key][q] rows: 16 B per lane
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
          *reinterpret_cast<bf16x8*>((char*)ds_t + krow * 64 + (s2 * 16 + 8 * hi) * 2) = dsa[g][s2];
        __builtin_amdgcn_sched_barrier(0);
      }

      attn::tr_quad_wait<0>(&qq[0]);
#pragma unroll
      for (int d = 0; d < DB; ++d) {
        if (d + 1 < DB)
          attn::tr_quad_issue(do_lds, q_lds, 0, (d + 1) * 32, &qq[(d + 1) & 1], lv);
        attn::TrQuad& t = qq[d & 1];
        if (d > 0) {
          if (d + 1 < DB)
            attn::tr_quad_wait<8>(&t);
          else
            attn::tr_quad_wait<0>(&t);
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          dv_acc[g][d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[g][0], t.x.a, dv_acc[g][d], 0, 0, 0);
          dv_acc[g][d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[g][1], t.x.b, dv_acc[g][d], 0, 0, 0);
          dk_acc[g][d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dsa[g][0], t.y.a, dk_acc[g][d], 0, 0, 0);
          dk_acc[g][d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dsa[g][1], t.y.b, dk_acc[g][d], 0, 0, 0);
        }
      }
    }

    // dS tile complete: all 256 key rows written (zeros where masked)
    attn::lds_barrier();

    // dQ[32 q][32w..32w+32) = dS[q][keys] K[keys][d] over those keys, two
    // 32-key steps per trip (software-pipelined transpose reads).
    const int nkp = min(kend64, (q32 + 32 - k0 + 63) & ~63) >> 5;  // even, >= 2
    f32x16 dq = f32x16{};
    attn::TrQuad kq[2];
    // The last trip is peeled so that no read in flight meets an if / else
    // join: joined there, the compiler may place the register copies of the
    // join ahead of the wait on one side (it cannot see the reads inside
    // the asm) and copy fragments that have not arrived.
    attn::tr_dsk_issue(ds_t, k_img, 0, 32 * wave, &kq[0], lv);
    int kp = 0;
#pragma unroll 1
    for (; kp + 2 < nkp; kp += 2) {
      attn::tr_dsk_issue(ds_t, k_img, (kp + 1) * 32, 32 * wave, &kq[1], lv);
      attn::tr_quad_wait<8>(&kq[0]);
      attn::mfma_quad_acc(dq, kq[0]);
      attn::tr_dsk_issue(ds_t, k_img, (kp + 2) * 32, 32 * wave, &kq[0], lv);
      attn::tr_quad_wait<8>(&kq[1]);
      attn::mfma_quad_acc(dq, kq[1]);
    }
    attn::tr_dsk_issue(ds_t, k_img, (kp + 1) * 32, 32 * wave, &kq[1], lv);
    attn::tr_quad_wait<8>(&kq[0]);
    attn::mfma_quad_acc(dq, kq[0]);
    attn::tr_quad_wait<0>(&kq[1]);
    attn::mfma_quad_acc(dq, kq[1]);
    // one register = rows crow(r,0) and crow(r,1), 128 B each; left in flight
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qr = q32 + (r & 3) + 8 * (r >> 2) + 4 * hi;  // literal crow: see softmax
      if (qr < T) unsafeAtomicAdd(dq_col + (long)qr * C + li, dq[r]);
    }
  }

  // epilogue: dK/dV rows crow(r,hi) of each key group
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kr = kw + 32 * g + (r & 3) + 8 * (r >> 2) + 4 * hi;  // literal crow
      if (kr >= T) continue;
#pragma unroll
      for (int d = 0; d < DB; ++d) {
        dqkv[kbase + (long)kr * QS + d * 32 + li] = f32_to_bf16(dk_acc[g][d][r]);
        dqkv[vbase + (long)kr * QS + d * 32 + li] = f32_to_bf16(dv_acc[g][d][r]);
      }
    }
}

// f32 dQ scratch (B, T, C) -> bf16 q columns of dqkv (row stride 3C); eight
// elements per thread: two 16 B loads, one 16 B store. C % 8 == 0.
__global__ void dq_convert_kernel(const float* __restrict__ dq32,
                                  uint16_t* __restrict__ dqkv, long rows, int C) {
  const int cpr = C / 8;  // 8-element chunks per row
  const long n = rows * cpr;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x) {
    const long row = i / cpr;
    const int c = (int)(i % cpr) * 8;
    const f32x4 a = *reinterpret_cast<const f32x4*>(&dq32[row * C + c]);
    const f32x4 b = *reinterpret_cast<const f32x4*>(&dq32[row * C + c + 4]);
    s16x8 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[j] = (short)f32_to_bf16(a[j]);
      o[4 + j] = (short)f32_to_bf16(b[j]);
    }
    *reinterpret_cast<s16x8*>(&dqkv[row * 3 * C + c]) = o;
  }
}

// Two-kernel path: dq and dkdv are independent (disjoint column ranges of
// dqkv) and each is stall-bound on its own, so they run CONCURRENTLY, dq on
// the caller's stream and dkdv on this side stream, forked and joined with
// the two events below: each kernel's blocks fill CUs and wait cycles the
// other leaves idle. (A 4-wave dQ beside the 4-wave dKdV measured slower than
// this 8-wave dQ: profiles/PERF.md.)
inline hipStream_t bwd_side_stream() {
  static hipStream_t s = [] {
    hipStream_t t;
    (void)hipStreamCreateWithFlags(&t, hipStreamNonBlocking);
    return t;
  }();
  return s;
}
inline hipEvent_t bwd_event(int i) {
  auto make = [] {
    hipEvent_t t;
    (void)hipEventCreateWithFlags(&t, hipEventDisableTiming);
    return t;
  };
  static hipEvent_t e[2] = {make(), make()};
  return e[i];
}

template <int D>
void launch_bwd(const at::Tensor& qkv, const at::Tensor& dout, const at::Tensor& lse,
                const at::Tensor& delta, const at::Tensor& slopes, at::Tensor& dqkv,
                int B, int H, int T, int C, float scale, float p_drop,
                uint32_t seed, hipStream_t stream) {
  auto launch = [&](auto kernel, int rows, int threads, size_t smem, hipStream_t s) {
    hipLaunchKernelGGL(kernel, dim3(B * H, (T + rows - 1) / rows), dim3(threads), smem, s,
                       (const uint16_t*)qkv.data_ptr(), (const uint16_t*)dout.data_ptr(),
                       lse.data_ptr<float>(), delta.data_ptr<float>(),
                       slopes.data_ptr<float>(), (uint16_t*)dqkv.data_ptr(), H, T, C,
                       scale, p_drop, seed);
  };
  // two double-buffered 64-row tiles; dkdv adds the (lse, delta) slices
  const size_t smem_dq = 4 * TB * 128 * sizeof(uint16_t);
  const size_t smem_kv = smem_dq + 4 * TB * sizeof(float);
  hipStream_t side = bwd_side_stream();
  (void)hipEventRecord(bwd_event(0), stream);
  (void)hipStreamWaitEvent(side, bwd_event(0), 0);
  launch(flash_dq_kernel<D>, RB, 512, smem_dq, stream);
  launch(flash_dkdv4_kernel<D>, RB4, 256, smem_kv, side);
  (void)hipEventRecord(bwd_event(1), side);
  (void)hipStreamWaitEvent(stream, bwd_event(1), 0);
}

// Fused path, all on the caller's stream: (scratch already zeroed, delta
// done) fused kernel, then the f32 -> bf16 dQ convert.
void launch_bwd_fused(const at::Tensor& qkv, const at::Tensor& dout,
                      const at::Tensor& lse, const at::Tensor& delta,
                      const at::Tensor& slopes, at::Tensor& dqkv, at::Tensor& dq32,
                      int B, int H, int T, int C, float scale, float p_drop,
                      uint32_t seed, hipStream_t stream) {
  static const bool attr_ok = [] {
    return hipFuncSetAttribute((const void*)flash_bwd_fused_kernel<128>,
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)FUSED_SMEM) == hipSuccess;
  }();
  TORCH_CHECK(attr_ok, "attn_bwd: fused kernel needs ", FUSED_SMEM, " B of LDS");
  dim3 grid(B * H, (T + FKB - 1) / FKB);
  hipLaunchKernelGGL(flash_bwd_fused_kernel<128>, grid, dim3(256), FUSED_SMEM, stream,
                     (const uint16_t*)qkv.data_ptr(), (const uint16_t*)dout.data_ptr(),
                     lse.data_ptr<float>(), delta.data_ptr<float>(),
                     slopes.data_ptr<float>(), (uint16_t*)dqkv.data_ptr(),
                     dq32.data_ptr<float>(), H, T, C, scale, p_drop, seed);
  TORCH_CHECK(hipGetLastError() == hipSuccess, "attn_bwd: fused kernel launch failed");
  const long rows = (long)B * T;
  hipLaunchKernelGGL(dq_convert_kernel, dim3(capped_grid(rows * (C / 8), 256)),
                     dim3(256), 0, stream, dq32.data_ptr<float>(),
                     (uint16_t*)dqkv.data_ptr(), rows, C);
}

// Process-wide default of the backward scheme: ZTA_BWD_FUSED=0 selects the
// two-kernel path, ZTA_BWD_FUSED=1 the fused kernel.
inline bool bwd_fused_default() {
  static const bool v = [] {
    const char* e = getenv("ZTA_BWD_FUSED");
    return e ? e[0] != '0' : BWD_FUSED_DEFAULT;
  }();
  return v;
}

}  // namespace

std::vector<at::Tensor> attn_bwd(at::Tensor dout, at::Tensor qkv, at::Tensor slopes,
                                 at::Tensor o, at::Tensor lse, int64_t H_,
                                 double p_drop, int64_t seed, int64_t fused) {
  // Everything the kernels take on trust is checked here, before any launch:
  // they reinterpret the buffers as bf16 / f32 bits and index them by
  // (B, T, C) and (B, H, T) alone.
  TORCH_CHECK(qkv.is_cuda() && qkv.is_contiguous() && qkv.dim() == 3,
              "attn_bwd: qkv must be (B, T, 3C) contiguous on the GPU");
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16, "attn_bwd: qkv must be bf16");
  TORCH_CHECK(H_ > 0, "attn_bwd: H must be positive, got ", H_);
  const int B = qkv.size(0), T = qkv.size(1), H = (int)H_;
  const int C = qkv.size(2) / 3;
  TORCH_CHECK(qkv.size(2) == 3 * C && C % H == 0,
              "attn_bwd: qkv last dim must be 3C with C % H == 0, got ", qkv.size(2),
              " for H = ", H);
  const int D = C / H;
  TORCH_CHECK(D == 32 || D == 64 || D == 96 || D == 128,
              "attn_bwd: head_dim must be 32/64/96/128, got ", D);
  auto check_act = [&](const at::Tensor& t, const char* name) {
    TORCH_CHECK(t.device() == qkv.device(), "attn_bwd: ", name, " must be on qkv's device");
    TORCH_CHECK(t.scalar_type() == at::kBFloat16, "attn_bwd: ", name, " must be bf16");
    TORCH_CHECK(t.dim() == 3 && t.size(0) == B && t.size(1) == T && t.size(2) == C,
                "attn_bwd: ", name, " must be (B, T, C)");
    TORCH_CHECK(t.is_contiguous(), "attn_bwd: ", name, " must be contiguous");
  };
  check_act(dout, "dout");
  check_act(o, "o");
  TORCH_CHECK(lse.device() == qkv.device(), "attn_bwd: lse must be on qkv's device");
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.dim() == 3 && lse.size(0) == B &&
                  lse.size(1) == H && lse.size(2) == T,
              "attn_bwd: lse must be float32 (B, H, T)");
  TORCH_CHECK(lse.is_contiguous(), "attn_bwd: lse must be contiguous");
  TORCH_CHECK(slopes.device() == qkv.device(), "attn_bwd: slopes must be on qkv's device");
  TORCH_CHECK(slopes.numel() == H, "attn_bwd: slopes must have H = ", H,
              " elements, got ", slopes.numel());
  auto dqkv = at::empty_like(qkv);
  auto delta = at::empty({B, H, T}, qkv.options().dtype(at::kFloat));
  auto sl = slopes.to(at::kFloat).contiguous();
  const float scale = 1.0f / sqrtf((float)D);
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  // fused < 0: process default (ZTA_BWD_FUSED); head dims the fused kernel
  // does not cover take the two-kernel path.
  const bool use_fused = D == 128 && (fused < 0 ? bwd_fused_default() : fused != 0);
  at::Tensor dq32;
  if (use_fused) dq32 = at::zeros({B, T, C}, qkv.options().dtype(at::kFloat));
  {
    const long rows = (long)B * H * T;
    const int block = 256;
    if (D % 64 == 0) {
      hipLaunchKernelGGL(delta_kernel_v8, dim3(capped_grid(rows * 8, block)),
                         dim3(block), 0, stream, (const uint16_t*)dout.data_ptr(),
                         (const uint16_t*)o.data_ptr(), delta.data_ptr<float>(),
                         rows, H, T, C, D);
    } else {
      hipLaunchKernelGGL(delta_kernel, dim3(capped_grid(rows * WAVE, block)),
                         dim3(block), 0, stream, (const uint16_t*)dout.data_ptr(),
                         (const uint16_t*)o.data_ptr(), delta.data_ptr<float>(),
                         rows, H, T, C, D);
    }
  }
  if (use_fused) {
    launch_bwd_fused(qkv, dout, lse, delta, sl, dqkv, dq32, B, H, T, C, scale,
                     (float)p_drop, (uint32_t)seed, stream);
    return {dqkv};
  }
  const bool ok = attn::with_head_dim(D, [&](auto d) {
    launch_bwd<decltype(d)::value>(qkv, dout, lse, delta, sl, dqkv, B, H, T, C, scale,
                                   (float)p_drop, (uint32_t)seed, stream);
  });
  TORCH_CHECK(ok, "attn_bwd: head_dim must be 32/64/96/128, got ", D);
  return {dqkv};
}
