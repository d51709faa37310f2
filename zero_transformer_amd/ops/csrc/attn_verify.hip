// Speculative-decoding verify attention for gfx950: T <= 16 new query rows per
// sequence against a long KV cache, split over the keys.
//
//   attn_verify_append(qkv (B, T, 3C), k_cache / v_cache (B, H, S_alloc, D),
//                      slopes (H), lens (B), start (B)) -> o (B, T, C)
//   attn_verify_paged(qkv (B, T, 3C), k_pool / v_pool (P, H, R, D), slopes (H),
//                     block_table (B, M), lens (B), start (B)) -> o (B, T, C)
//
// Semantics are those of attn_prefill_append / attn_prefill_paged (their file
// headers): st = clamp(start[b]), n = clamp(lens[b]); K/V rows i < n go to
// cache rows st + i; query row i < n attends over rows [0, st + i] with the
// bias slope * (j - (st + i)); rows i >= n of o are zeros. The rounding points
// are the flash kernels' too: fp32 scores and statistics, P rounded to the
// element type for the value product, the normaliser summed from the
// unrounded P, one rounding of the normalised output.
//
// Why another kernel: the prefill grid is (B*H, ceil(T/32)), 16 workgroups at
// batch 1 on the 1.3B shape, each walking all keys with a 32-row tile that is
// mostly padding; the decode kernels split the keys but take one row on VALU
// dot products. Here the cache is streamed once for all T rows by
// B*H*8 workgroups.
//
// Three launches on one stream:
//   verify_append_kernel<Addr>  copies the K / V columns of the live rows into
//     the cache, 16 B per lane, so that the split kernel reads every key from
//     the cache.
//   verify_split_kernel<D, F16, Addr>  grid (B*H, 8), four waves. The keys
//     [0, st + n) are cut into tiles of 32, aligned to 32 (so a tile never
//     straddles a page: R % 64 == 0); split s owns the contiguous tiles
//     [s * tps, (s + 1) * tps), tps = ceil(tiles / 8), and wave w of it takes
//     tiles w, w + 4, ... of that chunk. Waves never share a tile, so the
//     key loop has NO workgroup barrier and no LDS-DMA.
//   attn_decode_merge_kernel (attn_kv.h)  unchanged: one partial
//     {m, l, acc[64 * DPL]} per (b, t, h) and split, m in natural-log units
//     (the kernel works in log2 units and converts once), indexed
//     ((b * T + t) * H + h), which is also where the row goes in o (B, T, C).
//     An empty chunk and a row i >= n leave m = NEG_INF, l = 0, acc = 0: weight
//     0 in the merge, and a row whose every partial is so is written as zeros.
//
// Fragment layouts (v_mfma_f32_16x16x32 f16 / bf16: A lane l = row l & 15,
// k = 8 * (l >> 4) + e; B the same with column l & 15; C lane l = column
// l & 15, rows 4 * (l >> 4) + r). Both products are computed transposed, so
// that the query row is the lane's COLUMN in every accumulator and m, l,
// alpha are lane-local (no broadcast to rescale O):
//   S^T[key][q] = K Q^T.  A = K: lane l needs 16 B of key row l & 15 — a plain
//     global load straight into registers, no LDS. B = Q^T is the same load
//     from qkv, done once and kept for the whole chunk (D / 8 VGPRs), rows
//     >= n as zeros. Two 16-key MFMA tiles per 32-key wave tile.
//   O^T[d][q] += V^T P^T.  B = P^T needs, per lane, 8 keys of its own column:
//     exactly the 4 + 4 accumulator registers of the two S^T tiles, if the k
//     index 8 * g + e of the product is read as key 4 * g + e of tile 0
//     (e < 4) and key 4 * g + e - 4 of tile 1: P goes from C layout to
//     operand with four cvt_pk and no lane exchange. A = V^T in that key
//     order is what ds_read_b64_tr_b16 returns when the 16 lanes of group g
//     address rows 4 g .. 4 g + 3 (+ 16 for tile 1) of a row-major V tile:
//     two transpose reads per 16 output columns. So only V goes through LDS,
//     global -> registers -> ds_write_b128 -> transpose read, in a 32-row
//     tile private to the wave (row stride 2 D + 32 B: consecutive rows start
//     8 banks apart). One wave's DS operations execute in order, so neither
//     the write -> read nor the read -> next write needs a barrier.
//   The next tile's K and V loads are issued before the current tile's
//   products (register double buffer); rows past st + n - 1 are clamped to
//   that live row, whose keys the causal mask gives p = 0.
// Tiles with kt + 31 <= st lie below every row's diagonal and skip the mask.
// After the loop the four waves put (m, l, O^T) into their own (now idle) V
// tiles, one barrier, and 16 threads per query row merge them into the
// partial.
//
// -Rpass-analysis=kernel-resource-usage: no spill and no scratch in any of the
// 16 instantiations; registers and LDS are in the table at
// verify_split_kernel.
// Built without packed fp32 VALU ops (ops/build.py SOURCE_FLAGS). No atomics:
// the result is deterministic and does not depend on the paging.

#include "attn_kv.h"

#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <type_traits>

namespace {

constexpr int VNW = 4;      // waves per workgroup
constexpr int VT = 32;      // keys per wave tile
constexpr int VSPLITS = 8;  // workgroups per (b, h), as the decode ops

// Where a cache row lives: element offset of row j (< cap()) of head h of
// sequence b. Rows of one VT-aligned tile are contiguous from row(.., kt).
struct ContigAddr {
  int S_alloc;
  ZTA_DEV int cap() const { return S_alloc; }
  ZTA_DEV long row(int b, int h, int H, int D, int j) const {
    return (((long)b * H + h) * S_alloc + j) * D;
  }
};
struct PagedAddr {
  const int* bt;
  Pool pl;
  ZTA_DEV int cap() const { return pl.M * pl.R; }
  ZTA_DEV long row(int b, int h, int H, int D, int j) const {
    const int pi = j / pl.R;  // < M because j < M * R
    return (((long)page_of(bt, b, pi, pl) * H + h) * pl.R + (j - pi * pl.R)) * D;
  }
};

// One item = 8 elements (16 B) of the K or V columns of one qkv row.
template <class Addr>
__global__ __launch_bounds__(256) void verify_append_kernel(
    const uint16_t* __restrict__ qkv, uint16_t* __restrict__ kc,
    uint16_t* __restrict__ vc, const int* __restrict__ lens,
    const int* __restrict__ start, int B, int H, int T, int C, int D, Addr addr) {
  const int c8n = C / 8;
  const long total = (long)B * T * 2 * c8n;
  for (long it = (long)blockIdx.x * blockDim.x + threadIdx.x; it < total;
       it += (long)gridDim.x * blockDim.x) {
    const int c8 = (int)(it % c8n);
    const int kv = (int)((it / c8n) & 1);
    const long row = it / (2 * c8n);
    const int i = (int)(row % T), b = (int)(row / T);
    const auto [st, n] = seq_range(lens, start, b, T, addr.cap());
    if (i >= n) continue;
    const int col = c8 * 8, h = col / D, d = col % D;
    const s16x8 x = *reinterpret_cast<const s16x8*>(&qkv[row * 3 * C + (1 + kv) * C + col]);
    uint16_t* dst = kv ? vc : kc;
    *reinterpret_cast<s16x8*>(&dst[addr.row(b, h, H, D, st + i) + d]) = x;  // st + i < cap
  }
}

template <bool F16>
ZTA_DEV f32x4 mfma16x32(bf16x8 a, bf16x8 b, f32x4 c) {
  if constexpr (F16) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a),
                                                  __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  } else {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
}

// ds_read_b64_tr_b16 (semantics: attn_tiles.h): the lane receives, of the
// [4][16] tile its 16-lane group addresses, column lane & 15, rows 0..3.
ZTA_DEV s16x4 tr_read(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)p);
}

// Resources (fp16 and bf16 alike; contiguous / paged), no spills, no scratch:
//            VGPRs       AGPRs   LDS bytes   waves / SIMD
//   D 32     78 / 80       8      12288       5
//   D 64    112 / 120     16      20480       4 / 3
//   D 96    164 / 166     24      28672       2
//   D 128   180 / 182     32      36864       2
template <int D, bool F16, class Addr>
__global__ __launch_bounds__(VNW * 64) void verify_split_kernel(
    const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ kc,
    const uint16_t* __restrict__ vc, const float* __restrict__ slopes,
    float* __restrict__ part,  // (B * T * H, splits, 2 + 64 * DPL)
    const int* __restrict__ lens, const int* __restrict__ start, int H, int T, int C,
    Addr addr, float scale) {
  constexpr int KS = D / 32;   // k-steps of a score tile
  constexpr int DB = D / 16;   // 16-column blocks of O^T; also V chunks per lane
  constexpr int C8 = D / 8;    // 16 B chunks per row
  constexpr int DPL = (D + 63) / 64;
  constexpr int PW = 2 + 64 * DPL;
  constexpr int VROW = 2 * D + 32;  // bytes per staged V row
  constexpr int WBYTES = VT * VROW;
  constexpr int OS = 17;            // q stride of the merge image, in floats
  static_assert(D * OS * 4 + 128 <= WBYTES, "merge image must fit the V tile");
  __shared__ __attribute__((aligned(16))) char smem[VNW * WBYTES];

  const int bh = blockIdx.x;
  const int b = bh / H, h = bh % H;
  const int split = blockIdx.y, splits = gridDim.y;
  const auto [st, n] = seq_range(lens, start, b, T, addr.cap());
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int L = lane & 15;  // this lane's query row
  const int g = lane >> 4;
  const int s_end = st + n;  // keys [0, s_end) are live; <= cap
  const int ntiles = (s_end + VT - 1) / VT;
  const int tps = (ntiles + splits - 1) / splits;
  const int t_lo = split * tps;
  const int t_hi = n > 0 ? min(ntiles, t_lo + tps) : 0;  // no live row: no tile

  constexpr float LOG2E = 1.4426950408889634f;
  constexpr float LN2 = 0.6931471805599453f;
  const float scale2 = scale * LOG2E;
  const float slope2 = slopes[h] * LOG2E;
  const bool ok = L < n;  // n <= T
  const int pi = st + L;  // position of this lane's row

  bf16x8 qf[KS];
  {
    const long qrow = ((long)b * T + L) * 3 * C + (long)h * D;
#pragma unroll
    for (int s = 0; s < KS; ++s)
      qf[s] = ok ? *reinterpret_cast<const bf16x8*>(&qkv[qrow + s * 32 + 8 * g]) : bf16x8{};
  }

  float m_run = NEG_INF, l_run = 0.f;
  f32x4 o_acc[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d) o_acc[d] = f32x4{};

  char* vl = smem + wave * WBYTES;  // this wave's V tile, later its merge image
  bf16x8 kn[2][KS];
  s16x8 vn[DB];
  // tile t -> registers; rows past the last live key read that key's row
  auto load_tile = [&](int t) {
    const int kt = t * VT;
    const long base = addr.row(b, h, H, D, kt);  // kt < s_end <= cap
    const int last = s_end - 1 - kt;             // >= 0
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const long r = min(sub * 16 + L, last);
#pragma unroll
      for (int s = 0; s < KS; ++s)
        kn[sub][s] = *reinterpret_cast<const bf16x8*>(&kc[base + r * D + s * 32 + 8 * g]);
    }
#pragma unroll
    for (int it = 0; it < DB; ++it) {
      const int c = it * 64 + lane;
      const long r = min(c / C8, last);
      vn[it] = *reinterpret_cast<const s16x8*>(&vc[base + r * D + (c % C8) * 8]);
    }
  };

  int t = t_lo + wave;
  if (t < t_hi) load_tile(t);
  for (; t < t_hi; t += VNW) {
    // V tile -> LDS (after the previous tile's transpose reads: DS order)
#pragma unroll
    for (int it = 0; it < DB; ++it) {
      const int c = it * 64 + lane;
      *reinterpret_cast<s16x8*>(vl + (c / C8) * VROW + (c % C8) * 16) = vn[it];
    }
    bf16x8 kf[2][KS];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int s = 0; s < KS; ++s) kf[sub][s] = kn[sub][s];
    if (t + VNW < t_hi) load_tile(t + VNW);
    const int kt = t * VT;

    // ---- S^T tiles: C[i = key][j = q] = mfma(A = K, B = Q^T) ----
    f32x4 s_acc[2];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      s_acc[sub] = f32x4{};
#pragma unroll
      for (int s = 0; s < KS; ++s) s_acc[sub] = mfma16x32<F16>(kf[sub][s], qf[s], s_acc[sub]);
    }

    // ---- online softmax of row L, log2 domain; register e holds key
    // kt + 16 * (e >> 2) + 4 g + (e & 3). Wave-uniform mask test. ----
    float sv[8];
    float tile_max = NEG_INF;
    if (kt + VT - 1 <= st) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int kj = kt + 16 * (e >> 2) + 4 * g + (e & 3);
        sv[e] = s_acc[e >> 2][e & 3] * scale2 + slope2 * (float)(kj - pi);
        tile_max = fmaxf(tile_max, sv[e]);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int kj = kt + 16 * (e >> 2) + 4 * g + (e & 3);
        float x = s_acc[e >> 2][e & 3] * scale2 + slope2 * (float)(kj - pi);
        if (kj > pi || !ok) x = NEG_INF;
        sv[e] = x;
        tile_max = fmaxf(tile_max, x);
      }
    }
    tile_max = fmaxf(tile_max, __shfl_xor(tile_max, 16, 64));
    tile_max = fmaxf(tile_max, __shfl_xor(tile_max, 32, 64));
    const float m_new = fmaxf(m_run, tile_max);
    // m_run == NEG_INF: nothing accumulated yet, alpha is irrelevant but finite
    const float alpha = exp2f(m_run - m_new);
    m_run = m_new;
    float p[8];
    float row_sum = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      p[e] = sv[e] > 0.5f * NEG_INF ? exp2f(sv[e] - m_new) : 0.f;
      row_sum += p[e];
    }
    row_sum += __shfl_xor(row_sum, 16, 64);
    row_sum += __shfl_xor(row_sum, 32, 64);
    l_run = l_run * alpha + row_sum;
#pragma unroll
    for (int d = 0; d < DB; ++d) o_acc[d] *= alpha;

    // ---- P^T operand: the lane's own eight values, rounded ----
    union {
      unsigned u[4];
      bf16x8 v8;
    } pb;
#pragma unroll
    for (int j = 0; j < 4; ++j) pb.u[j] = pack2<F16>(p[2 * j], p[2 * j + 1]);

    // ---- O^T += V^T P^T: A = V^T by transpose reads ----
    const char* vrd = vl + (4 * g + (L >> 2)) * VROW + (4 * (L & 3)) * 2;
#pragma unroll
    for (int d = 0; d < DB; ++d) {
      union {
        s16x4 h[2];
        bf16x8 v8;
      } va;
      va.h[0] = tr_read(vrd + d * 32);
      va.h[1] = tr_read(vrd + 16 * VROW + d * 32);
      o_acc[d] = mfma16x32<F16>(va.v8, pb.v8, o_acc[d]);
    }
  }

  // ---- merge the four waves: image [d][OS] of O^T, then m[16], l[16] ----
  float* wo = (float*)vl;
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int r = 0; r < 4; ++r) wo[(d * 16 + 4 * g + r) * OS + L] = o_acc[d][r];
  if (g == 0) {
    wo[D * OS + L] = m_run;
    wo[D * OS + 16 + L] = l_run;
  }
  __syncthreads();
  const int q = threadIdx.x >> 4, dg = threadIdx.x & 15;
  if (q >= T) return;
  const bool live = q < n;
  float mw[VNW], mg = NEG_INF;
#pragma unroll
  for (int w = 0; w < VNW; ++w) {
    mw[w] = ((const float*)(smem + w * WBYTES))[D * OS + q];
    mg = fmaxf(mg, mw[w]);
  }
  float f[VNW], lg = 0.f;
#pragma unroll
  for (int w = 0; w < VNW; ++w) {
    f[w] = mw[w] > 0.5f * NEG_INF ? exp2f(mw[w] - mg) : 0.f;
    lg += ((const float*)(smem + w * WBYTES))[D * OS + 16 + q] * f[w];
  }
  float* pr = &part[((((long)b * T + q) * H + h) * splits + split) * PW];
  if (dg == 0) {
    pr[0] = live && mg > 0.5f * NEG_INF ? mg * LN2 : NEG_INF;
    pr[1] = live ? lg : 0.f;
  }
#pragma unroll
  for (int k = 0; k < 4 * DPL; ++k) {
    const int d = dg + 16 * k;
    float o = 0.f;
    if (d < D && live) {
#pragma unroll
      for (int w = 0; w < VNW; ++w)
        o += ((const float*)(smem + w * WBYTES))[d * OS + q] * f[w];
    }
    pr[2 + d] = o;
  }
}

// Checks shared by both ops; the cache / pool checks follow in each.
void check_common(const char* op, const at::Tensor& qkv, const at::Tensor& kc,
                  const at::Tensor& vc, const at::Tensor& slopes,
                  std::initializer_list<const at::Tensor*> per_seq) {
  TORCH_CHECK(qkv.is_cuda() && qkv.is_contiguous() && qkv.dim() == 3 &&
                  qkv.size(2) % 3 == 0,
              op, ": qkv must be (B, T, 3C) contiguous");
  TORCH_CHECK(qkv.scalar_type() == at::kHalf || qkv.scalar_type() == at::kBFloat16, op,
              ": fp16 or bf16 only");
  TORCH_CHECK(qkv.size(1) <= 16, op, ": at most 16 rows per sequence, got ", qkv.size(1));
  const long B = qkv.size(0), C = qkv.size(2) / 3;
  TORCH_CHECK(kc.is_cuda() && vc.is_cuda() && kc.dim() == 4 && kc.is_contiguous() &&
                  vc.is_contiguous() && kc.sizes() == vc.sizes() &&
                  kc.scalar_type() == qkv.scalar_type() &&
                  vc.scalar_type() == qkv.scalar_type() &&
                  kc.size(1) * kc.size(3) == C && kc.size(0) >= 1,
              op, ": the caches must be 4-d contiguous, alike, of qkv's dtype, with "
              "H*D == C");
  TORCH_CHECK(kc.size(2) < (1L << 31) / 2, op, ": too many rows");
  TORCH_CHECK(slopes.numel() == kc.size(1), op, ": slopes must have one entry per head");
  for (const at::Tensor* t : per_seq)
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kInt && t->dim() == 1 &&
                    t->numel() == B && t->is_contiguous(),
                op, ": lens / start must be (B,) contiguous int32 device tensors");
}

template <class Addr>
at::Tensor run_verify(const char* op, const at::Tensor& qkv, at::Tensor& kc, at::Tensor& vc,
                      const at::Tensor& slopes, const at::Tensor& lens,
                      const at::Tensor& start, int H, int D, Addr addr) {
  const bool f16 = qkv.scalar_type() == at::kHalf;
  const int B = qkv.size(0), T = qkv.size(1), C = qkv.size(2) / 3;
  auto o = at::empty({B, T, C}, qkv.options());
  if (B == 0 || T == 0) return o;
  auto sl = slopes.to(at::kFloat).contiguous();
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const int* lp = lens.data_ptr<int>();
  const int* sp = start.data_ptr<int>();
  const bool ok = attn::with_head_dim(D, [&](auto d) {
    constexpr int DD = decltype(d)::value;
    constexpr int DPL = (DD + 63) / 64;
    auto part = at::empty({(long)B * T * H, VSPLITS, 2 + 64 * DPL},
                          qkv.options().dtype(at::kFloat));
    hipLaunchKernelGGL((verify_append_kernel<Addr>),
                       dim3(capped_grid((long)B * T * 2 * (C / 8), 256)), dim3(256), 0,
                       stream, (const uint16_t*)qkv.data_ptr(), (uint16_t*)kc.data_ptr(),
                       (uint16_t*)vc.data_ptr(), lp, sp, B, H, T, C, D, addr);
    auto launch = [&](auto f16c) {
      constexpr bool F = decltype(f16c)::value;
      hipLaunchKernelGGL((verify_split_kernel<DD, F, Addr>), dim3(B * H, VSPLITS),
                         dim3(VNW * 64), 0, stream, (const uint16_t*)qkv.data_ptr(),
                         (const uint16_t*)kc.data_ptr(), (const uint16_t*)vc.data_ptr(),
                         sl.data_ptr<float>(), part.data_ptr<float>(), lp, sp, H, T, C, addr,
                         1.0f / sqrtf((float)DD));
      hipLaunchKernelGGL((attn_decode_merge_kernel<DPL, F>), dim3(B * T * H), dim3(64), 0,
                         stream, part.data_ptr<float>(), (uint16_t*)o.data_ptr(), DD,
                         VSPLITS);
    };
    if (f16)
      launch(std::true_type{});
    else
      launch(std::false_type{});
  });
  TORCH_CHECK(ok, op, ": head_dim must be one of 32/64/96/128, got ", D);
  return o;
}

}  // namespace

at::Tensor attn_verify_append(at::Tensor qkv, at::Tensor k_cache, at::Tensor v_cache,
                              at::Tensor slopes, at::Tensor lens, at::Tensor start) {
  const char* op = "attn_verify_append";
  check_common(op, qkv, k_cache, v_cache, slopes, {&lens, &start});
  TORCH_CHECK(k_cache.size(0) == qkv.size(0), op,
              ": k_cache/v_cache must be (B, H, S_alloc, D)");
  return run_verify(op, qkv, k_cache, v_cache, slopes, lens, start, (int)k_cache.size(1),
                    (int)k_cache.size(3), ContigAddr{(int)k_cache.size(2)});
}

at::Tensor attn_verify_paged(at::Tensor qkv, at::Tensor k_pool, at::Tensor v_pool,
                             at::Tensor slopes, at::Tensor block_table, at::Tensor lens,
                             at::Tensor start) {
  const char* op = "attn_verify_paged";
  check_common(op, qkv, k_pool, v_pool, slopes, {&lens, &start});
  TORCH_CHECK(k_pool.size(2) % TB == 0 && k_pool.size(2) > 0, op,
              ": rows per page must be a positive multiple of ", TB);
  TORCH_CHECK(block_table.is_cuda() && block_table.scalar_type() == at::kInt &&
                  block_table.dim() == 2 && block_table.size(0) == qkv.size(0) &&
                  block_table.size(1) >= 1 && block_table.is_contiguous(),
              op, ": block_table must be a (B, M) contiguous int32 device tensor, M >= 1");
  TORCH_CHECK(block_table.size(1) * k_pool.size(2) < (1L << 31), op,
              ": M * R must fit in int32");
  const Pool pl{(int)k_pool.size(0), (int)k_pool.size(2), (int)block_table.size(1)};
  return run_verify(op, qkv, k_pool, v_pool, slopes, lens, start, (int)k_pool.size(1),
                    (int)k_pool.size(3), PagedAddr{block_table.data_ptr<int>(), pl});
}
