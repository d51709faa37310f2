// Paged KV cache attention for gfx950: the prefill and decode kernel pairs of
// attn_prefill.hip / attn_decode.hip with the cache addressed through a
// per-sequence block table instead of a (B, H, S_alloc, D) tensor.
//
//   k_pool / v_pool  (P, H, R, D) contiguous, fp16 or bf16: P pages of R rows.
//   block_table      (B, M) int32 on the device. Logical cache row j of
//                    sequence b lives in page block_table[b, j / R], row
//                    j % R; a sequence holds at most M * R rows.
//
//   attn_prefill_paged(qkv (B, T, 3C), k_pool, v_pool, slopes (H),
//                      block_table, lens (B), start (B)) -> o (B, T, C)
//   attn_decode_paged(qkv (B, 1, 3C), k_pool, v_pool, slopes (H),
//                     block_table, lens (B)) -> o (B, 1, C)
//
// Semantics are those of attn_prefill_append / attn_decode_append with
// S_alloc = M * R (see those files' headers for the schemes; only what paging
// changes is described here). R % 64 == 0 = attn::TB, so a staged 64-key tile
// never straddles a page and stays one contiguous 64*D*2-byte block.
//
// Device data that addresses a write is clamped: lengths to [0, M * R], page
// ids to [0, P). A table entry is used as a page id only for a page that holds
// a live row of the call (index < ceil(live rows / R)); what later entries
// hold is irrelevant.
//
// Prefill: the append kernel looks its destination page up per 16 B item. The
// flash kernel gives each tile's glds_stage its own base (the page's
// (page * H + h) * R * D), first row (kt % R) and a PAGE-LOCAL row limit, so
// the clamp of dead rows stays inside the live page. The page id is
// wave-uniform (a scalar load); the id of tile kt + 2 TB is loaded while tile
// kt + TB is being prefetched, so the load is never on the prefetch's issue
// path. (An outstanding scalar load only makes the counted lgkmcnt waits of
// attn_tiles.h wait longer: DS ops still retire in order.)
//
// Decode: block (bh, split) walks its key range page segment by page segment:
// one table lookup per segment, then the contiguous kernel's per-wave key
// order j = lo + wave, lo + wave + NW, ... inside it. The sequence's table row
// is loaded alongside its length, lane i holding entry i, and a segment takes
// its page id from that register: a lookup in memory would put one more
// dependent round trip between the length and the first key. The page index
// is a shift where R is a power of two. (Step times of the three variants:
// profiles/PERF.md "Paged KV".) Rows of more than 64 entries look up in
// memory. Partition (chunk = ceil(S / 8)), per-wave order and merge are those
// of attn_decode.hip, so the result does not depend on R or on the table.
//
// The helpers and the merge kernel are those of attn_kv.h. paged_flash_kernel
// is a second copy of prefill_flash_kernel's body (attn_kv.h), differing only
// in the staging calls (`stage`, `pg_next` here; the two glds_stage pairs
// there): a change to the scheme has to be made in both. One source body was
// tried in three forms (tools/kernel_isa.py against both kernels). The tile
// body and epilogue as ZTA_DEV functions, or the whole body as a ZTA_DEV
// template under two thin kernels, change the contiguous kernel (D 32: 123 ->
// 112 / 111 VGPRs; D 128: 210 -> 212; D 96: 188 -> 176). One __global__
// template with `if constexpr (PAGED)` at the staging sites and the paged
// arguments (bt, pl) last leaves all eight contiguous instantiations the same
// and the paged ones the same but for the argument order (+1..2 instructions,
// same registers), yet the paged prompt pass measured slower with it than
// with this copy, 1.3B fp16, paged column of tools/decode_bench.py --prefill
// --paged, copy / template / copy / template in one session, ms:
//   batch 1, prompt 128    3.48 / 3.23 / 3.40 / 3.41
//   batch 1, prompt 1024   5.55 / 5.79 / 5.62 / 5.77   (again 5.59 / 5.72 /
//                          5.49 / 5.61 / 5.50 / 5.73)
//   batch 1, prompt 2048   8.86 / 9.34 / 8.86 / 8.89   (again 8.94 / 8.92 /
//                          8.88 / 8.97 / 8.91 / 8.86)
//   batch 16, uniform 128  6.92 / 6.78 / 6.58 / 6.70
//   batch 16, 54..119      6.44 / 6.45 / 6.45 / 6.44
// The 1024 row is beyond the copy's own spread both times, so the copy stays.
// Kernel traces put 0.8 us per call (54.2 -> 55.0 us) of that in the kernel;
// the rest is not explained (profiles/PERF.md "Shared KV flash kernel").
// The decode split kernels here and in attn_decode.hip are separate on
// purpose: moving only the block-merge tail into a ZTA_DEV function, or
// running the contiguous case as one segment of the paged segment loop,
// changed all eight contiguous instantiations (36-97 lines each) of the
// latency-bound kernel of batch-1 decode.
// No atomics: both ops are deterministic.

#include "attn_kv.h"

#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <type_traits>

namespace {

// One item = 8 elements (16 B) of the K or V columns of one qkv row.
__global__ __launch_bounds__(256) void paged_append_kernel(
    const uint16_t* __restrict__ qkv, uint16_t* __restrict__ kp,
    uint16_t* __restrict__ vp, const int* __restrict__ bt,
    const int* __restrict__ lens, const int* __restrict__ start, int B, int H, int T,
    int C, int D, Pool pl) {
  const int c8n = C / 8;
  const long total = (long)B * T * 2 * c8n;
  for (long it = (long)blockIdx.x * blockDim.x + threadIdx.x; it < total;
       it += (long)gridDim.x * blockDim.x) {
    const int c8 = (int)(it % c8n);
    const int kv = (int)((it / c8n) & 1);
    const long row = it / (2 * c8n);
    const int i = (int)(row % T), b = (int)(row / T);
    const auto [st, n] = seq_range(lens, start, b, T, pl.M * pl.R);
    if (i >= n) continue;
    const int col = c8 * 8, h = col / D, d = col % D;
    const s16x8 x = *reinterpret_cast<const s16x8*>(&qkv[row * 3 * C + (1 + kv) * C + col]);
    const int j = st + i;  // < M * R, so j / R < M
    const int page = page_of(bt, b, j / pl.R, pl);
    uint16_t* dst = kv ? vp : kp;
    *reinterpret_cast<s16x8*>(
        &dst[(((long)page * H + h) * pl.R + j % pl.R) * D + d]) = x;
  }
}

template <int D, int NT, bool F16>
__global__ __launch_bounds__(NT, 2) void paged_flash_kernel(
    const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ kp,
    const uint16_t* __restrict__ vp, const float* __restrict__ slopes,
    uint16_t* __restrict__ o, const int* __restrict__ bt, const int* __restrict__ lens,
    const int* __restrict__ start, int H, int T, int C, Pool pl, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // double-buffered LDS-DMA staging: layout [k0 | v0 | k1 | v1]
  uint16_t* lds0 = (uint16_t*)smem;

  const int bh = blockIdx.x;
  const int b = bh / H;
  const auto [h, QS, base, kbase_, vbase_, obase] = attn::planes<D>(bh, H, T, C);
  const auto [st, n] = seq_range(lens, start, b, T, pl.M * pl.R);
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

  // keys of this block: logical rows [0, kv_end), all written (the append
  // kernel ran before on the stream). Tile kt lies in logical page kt / R at
  // rows kt % R ..; rows past the page's live ones are clamped to its last
  // live row, min(kv_end - page start, R) - 1.
  const int kv_end = st + min(n, q0 + QROWS);
  const long plane = (long)pl.R * D;  // one (page, head) plane
  const int head = h;  // (a structured binding cannot be captured)
  auto stage = [&](int kt, int page, uint16_t* buf) {
    const int r0 = kt % pl.R;
    const int lim = min(kv_end - (kt - r0), pl.R);
    const long pbase = ((long)page * H + head) * plane;
    attn::glds_stage<D, NT / 64>(kp, pbase, D, r0, lim, buf);
    attn::glds_stage<D, NT / 64>(vp, pbase, D, r0, lim, buf + TB * 128);
  };
  stage(0, page_of(bt, b, 0, pl), lds0);
  // page of the tile the next prefetch stages, loaded one iteration ahead
  int pg_next = TB < kv_end ? page_of(bt, b, TB / pl.R, pl) : 0;
  for (int kt = 0; kt < kv_end; kt += TB) {
    const int cur = (kt / TB) & 1;
    const uint16_t* k_lds = lds0 + (cur ? 2 * TB * 128 : 0);
    const uint16_t* v_lds = lds0 + TB * 128 + (cur ? 2 * TB * 128 : 0);
    // one barrier per tile: waits this wave's LDS-DMA (vmcnt(0)) and protects
    // the buffer the next prefetch overwrites
    attn::tile_barrier<0>();
    if (kt + TB < kv_end) {
      stage(kt + TB, pg_next, lds0 + (cur ? 0 : 2 * TB * 128));
      if (kt + 2 * TB < kv_end) pg_next = page_of(bt, b, (kt + 2 * TB) / pl.R, pl);
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

      // defer-max with threshold, as in prefill_flash_kernel
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

      // ---- P -> element-type A-fragments in-register ----
      bf16x8 pa[2];
      p_to_a_frags<F16>(p, pa);

      // ---- O += P @ V : V^T B-fragments via pipelined tr-reads ----
      attn::TrPair vfr[2];
      attn::tr_pair_issue(v_lds, sub * 32, 0, &vfr[0]);
#pragma unroll
      for (int d = 0; d < DB; ++d) {
        if (d + 1 < DB) attn::tr_pair_issue(v_lds, sub * 32, (d + 1) * 32, &vfr[(d + 1) & 1]);
        attn::TrPair& t = vfr[d & 1];
        if (d + 1 < DB)
          attn::tr_pair_wait<4>(&t);
        else
          attn::tr_pair_wait<0>(&t);
        o_acc[d] = mfma16<F16>(pa[0], t.a, o_acc[d]);
        o_acc[d] = mfma16<F16>(pa[1], t.b, o_acc[d]);
      }
    }
  }

  // ---- epilogue: O normalised in registers, written in the element type
  // into this wave's 32-row x D slice of the idle K/V buffers and stored as
  // whole rows, 16 B per lane; rows >= n leave as zeros. ----
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

// ---------------------------------------------------------------------------
// Decode
// ---------------------------------------------------------------------------

constexpr int NW = 4;  // waves per block

template <int DPL, bool F16>
__global__ __launch_bounds__(NW * 64) void paged_decode_split_kernel(
    const uint16_t* __restrict__ qkv,  // (B, 3C): q | k_new | v_new per row
    uint16_t* __restrict__ kp, uint16_t* __restrict__ vp,
    const float* __restrict__ slopes,
    float* __restrict__ part,  // (BH, SPLITS, 2 + 64*DPL)
    const int* __restrict__ bt, const int* __restrict__ lens, int H, int C, int D,
    Pool pl, int r_shift,  // log2(R) if R is a power of two, else -1
    float scale, int splits) {
  const int bh = blockIdx.x;
  const int b = bh / H, h = bh % H;
  const int S = min(max(lens[b], 0), pl.M * pl.R);
  __shared__ float red[NW * (3 + 64 * DPL)];
  const int split = blockIdx.y;
  const int chunk = (S + splits - 1) / splits;
  const int lo = split * chunk;
  const int hi = min(S, lo + chunk);
  const long row = (long)b * 3 * C + (long)h * D;  // q; k_new at + C, v_new at + 2C
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  // independent of S: issued together with the length and the q loads
  const int my_entry = bt[(long)b * pl.M + min(lane, pl.M - 1)];
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
    qv[e] = d < D ? cvt(qkv[row + d]) : 0.f;
  }
  float m = NEG_INF, l = 0.f;
  float acc[DPL];
#pragma unroll
  for (int e = 0; e < DPL; ++e) acc[e] = 0.f;

  // page segment by page segment; inside one, this wave's keys in the order
  // of attn_decode_split_kernel (j = lo + wave, + NW, ...)
  for (int j = lo + wave; j < hi;) {
    // wave-uniform, < M because j < S <= M * R. This sits between the length
    // and the first key: a shift where R allows it, not an integer division
    const int pidx = r_shift >= 0 ? j >> r_shift : j / pl.R;
    const int seg_end = min(hi, (pidx + 1) * pl.R);
    const int entry =
        pl.M <= 64 ? __builtin_amdgcn_readlane(my_entry, __builtin_amdgcn_readfirstlane(pidx))
                   : bt[(long)b * pl.M + pidx];
    const int page = min(max(entry, 0), pl.P - 1);
    // element offset of logical row 0 of this page's (page, h) plane
    const long base = (((long)page * H + h) * pl.R - (long)pidx * pl.R) * D;
    for (; j < seg_end; j += NW) {
      // the appended key: read from the projection row, stored to its page
      const bool fresh = j == S - 1;
      const uint16_t* kr = fresh ? &qkv[row + C] : &kp[base + (long)j * D];
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < DPL; ++e) {
        const int d = lane + e * 64;
        if (d < D) {
          const uint16_t ku = kr[d];
          if (fresh) kp[base + (long)j * D + d] = ku;
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
      const uint16_t* vr = fresh ? &qkv[row + 2 * C] : &vp[base + (long)j * D];
#pragma unroll
      for (int e = 0; e < DPL; ++e) {
        const int d = lane + e * 64;
        const uint16_t vu = d < D ? vr[d] : (uint16_t)0;
        if (fresh && d < D) vp[base + (long)j * D + d] = vu;
        acc[e] = acc[e] * alpha + (d < D ? p * cvt(vu) : 0.f);
      }
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

// Shared argument checks; returns the pool geometry.
Pool check_paged(const char* op, const at::Tensor& qkv, const at::Tensor& kp,
                 const at::Tensor& vp, const at::Tensor& slopes, const at::Tensor& bt,
                 std::initializer_list<const at::Tensor*> per_seq) {
  TORCH_CHECK(qkv.is_cuda() && qkv.is_contiguous() && qkv.dim() == 3 &&
                  qkv.size(2) % 3 == 0,
              op, ": qkv must be (B, T, 3C) contiguous");
  TORCH_CHECK(qkv.scalar_type() == at::kHalf || qkv.scalar_type() == at::kBFloat16, op,
              ": fp16 or bf16 only");
  const long B = qkv.size(0), C = qkv.size(2) / 3;
  TORCH_CHECK(kp.is_cuda() && vp.is_cuda() && kp.dim() == 4 && kp.is_contiguous() &&
                  vp.is_contiguous() && kp.sizes() == vp.sizes() &&
                  kp.scalar_type() == qkv.scalar_type() &&
                  vp.scalar_type() == qkv.scalar_type() &&
                  kp.size(1) * kp.size(3) == C && kp.size(0) >= 1,
              op, ": k_pool/v_pool must be (P, H, R, D) contiguous with P >= 1 and "
              "H*D == C, of qkv's dtype");
  TORCH_CHECK(kp.size(2) % TB == 0 && kp.size(2) > 0, op,
              ": rows per page must be a positive multiple of ", TB);
  TORCH_CHECK(slopes.numel() == kp.size(1), op, ": slopes must have one entry per head");
  TORCH_CHECK(bt.is_cuda() && bt.scalar_type() == at::kInt && bt.dim() == 2 &&
                  bt.size(0) == B && bt.size(1) >= 1 && bt.is_contiguous(),
              op, ": block_table must be a (B, M) contiguous int32 device tensor, M >= 1");
  TORCH_CHECK(bt.size(1) * kp.size(2) < (1L << 31), op, ": M * R must fit in int32");
  for (const at::Tensor* t : per_seq)
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kInt && t->dim() == 1 &&
                    t->numel() == B && t->is_contiguous(),
                op, ": lens / start must be (B,) contiguous int32 device tensors");
  return {(int)kp.size(0), (int)kp.size(2), (int)bt.size(1)};
}

}  // namespace

at::Tensor attn_prefill_paged(at::Tensor qkv, at::Tensor k_pool, at::Tensor v_pool,
                              at::Tensor slopes, at::Tensor block_table, at::Tensor lens,
                              at::Tensor start) {
  const Pool pl = check_paged("attn_prefill_paged", qkv, k_pool, v_pool, slopes,
                              block_table, {&lens, &start});
  const bool f16 = qkv.scalar_type() == at::kHalf;
  const int B = qkv.size(0), T = qkv.size(1), C = qkv.size(2) / 3;
  const int H = k_pool.size(1), D = k_pool.size(3);
  auto o = at::empty({B, T, C}, qkv.options());
  if (B == 0 || T == 0) return o;
  auto sl = slopes.to(at::kFloat).contiguous();
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const int* tp = block_table.data_ptr<int>();
  const int* lp = lens.data_ptr<int>();
  const int* sp = start.data_ptr<int>();
  const bool ok = attn::with_head_dim(D, [&](auto d) {
    constexpr int DD = decltype(d)::value;
    hipLaunchKernelGGL(paged_append_kernel,
                       dim3(capped_grid((long)B * T * 2 * (C / 8), 256)), dim3(256), 0,
                       stream, (const uint16_t*)qkv.data_ptr(),
                       (uint16_t*)k_pool.data_ptr(), (uint16_t*)v_pool.data_ptr(), tp, lp,
                       sp, B, H, T, C, D, pl);
    const size_t smem = 4 * TB * 128 * sizeof(uint16_t);  // 2 tensors x 2 buffers
    constexpr int QROWS = PREFILL_NT / 2;
    dim3 grid(B * H, (T + QROWS - 1) / QROWS);
    auto launch = [&](auto f16c) {
      hipLaunchKernelGGL((paged_flash_kernel<DD, PREFILL_NT, decltype(f16c)::value>), grid,
                         dim3(PREFILL_NT), smem, stream, (const uint16_t*)qkv.data_ptr(),
                         (const uint16_t*)k_pool.data_ptr(),
                         (const uint16_t*)v_pool.data_ptr(), sl.data_ptr<float>(),
                         (uint16_t*)o.data_ptr(), tp, lp, sp, H, T, C, pl,
                         1.0f / sqrtf((float)DD));
    };
    if (f16)
      launch(std::true_type{});
    else
      launch(std::false_type{});
  });
  TORCH_CHECK(ok, "attn_prefill_paged: head_dim must be one of 32/64/96/128, got ", D);
  return o;
}

at::Tensor attn_decode_paged(at::Tensor qkv, at::Tensor k_pool, at::Tensor v_pool,
                             at::Tensor slopes, at::Tensor block_table, at::Tensor lens) {
  const Pool pl = check_paged("attn_decode_paged", qkv, k_pool, v_pool, slopes,
                              block_table, {&lens});
  TORCH_CHECK(qkv.size(1) == 1, "attn_decode_paged: qkv must be (B, 1, 3C)");
  const bool f16 = qkv.scalar_type() == at::kHalf;
  const long B = qkv.size(0), C = qkv.size(2) / 3;
  const int H = k_pool.size(1), D = k_pool.size(3);
  TORCH_CHECK(D <= 256, "attn_decode_paged: head_dim up to 256");
  auto out = at::empty({B, 1, C}, qkv.options());
  if (B == 0) return out;
  auto sl = slopes.to(at::kFloat).contiguous();
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const int dpl = (D + 63) / 64;
  const int splits = 8;  // blocks per (b, h), as attn_decode.hip
  const int r_shift = (pl.R & (pl.R - 1)) == 0 ? __builtin_ctz(pl.R) : -1;
  auto part = at::empty({B * H, splits, 2 + 64 * (long)dpl},
                        qkv.options().dtype(at::kFloat));
  dim3 grid(B * H, splits);
  auto launch = [&](auto dplc, auto f16c) {
    constexpr int DPL = decltype(dplc)::value;
    constexpr bool F = decltype(f16c)::value;
    hipLaunchKernelGGL((paged_decode_split_kernel<DPL, F>), grid, dim3(NW * 64), 0, stream,
                       (const uint16_t*)qkv.data_ptr(), (uint16_t*)k_pool.data_ptr(),
                       (uint16_t*)v_pool.data_ptr(), sl.data_ptr<float>(),
                       part.data_ptr<float>(), block_table.data_ptr<int>(),
                       lens.data_ptr<int>(), H, (int)C, D, pl, r_shift,
                       1.0f / sqrtf((float)D), splits);
    hipLaunchKernelGGL((attn_decode_merge_kernel<DPL, F>), dim3(B * H), dim3(64), 0,
                       stream, part.data_ptr<float>(), (uint16_t*)out.data_ptr(), D, splits);
  };
  auto by_type = [&](auto dplc) {
    if (f16)
      launch(dplc, std::true_type{});
    else
      launch(dplc, std::false_type{});
  };
  switch (dpl) {
    case 1: by_type(std::integral_constant<int, 1>{}); break;
    case 2: by_type(std::integral_constant<int, 2>{}); break;
    case 3: by_type(std::integral_constant<int, 3>{}); break;
    case 4: by_type(std::integral_constant<int, 4>{}); break;
    default: TORCH_CHECK(false, "bad head_dim");
  }
  return out;
}
