// Speculative-decoding verify attention on the int8 paged KV cache for gfx950:
// T <= 16 new query rows per sequence against the code pools, split over the
// keys. The cache format and the quantizer are those of attn_kv8.hip, the
// semantics (st, n, clamps, bias, zeros in rows i >= n) and the work split
// those of attn_verify.hip.
//
//   attn_verify_paged_q8(qkv (B, T, 3C), k_pool / v_pool (P, H, R, D) uint8,
//                        k_scale / v_scale (P, H, R) fp32, slopes (H),
//                        block_table (B, M), lens (B), start (B)) -> o (B, T, C)
//
// Three launches on one stream:
//   kv8_quantize_paged (attn_kv8.hip)  quantizes the K / V columns of the live
//     rows into the pools (and replaces them in qkv by what the pools hold), so
//     that the split kernel reads every key from the pools.
//   kv8_verify_split_kernel<D, F16>  grid (B*H, 8), four waves; tiles of 32
//     keys aligned to 32 (inside one page: R % 64 == 0), 8 contiguous chunks of
//     tiles, wave w takes tiles w, w + 4, ... of its chunk. No workgroup
//     barrier, no LDS-DMA and no atomics in the key loop; the epilogue is that
//     of verify_split_kernel.
//   attn_decode_merge_kernel (attn_kv.h)  unchanged.
// The tiling is a function of st + n alone: the result is deterministic and
// depends neither on R nor on the block table.
//
// Both products are computed transposed (fragment layouts: attn_verify.hip),
// so the query row is the lane's accumulator column and m, l, alpha are
// lane-local. What is new here is how the operands are made from codes.
//
//   S^T[key][q] = K Q^T, A = the EXACT codes u - 128 (integers in [-127, 127],
//     exact in fp16 and in bf16), not codes * scale. The row's scale meets the
//     fp32 accumulator: s = acc * (k_scale[j] D^-1/2 log2 e) + slope2 (j - pos).
//     So K is not rounded to 16 bits at all (the staged route rounds it once).
//     In the C layout a lane holds keys 4 g + r of a 16-key tile: its four K
//     scales are one aligned 16 B load per 16-key tile.
//   K loads: a lane needs 8 codes per 32-wide contraction step. The
//     contraction index may be permuted as long as Q's operand uses the same
//     permutation, so a lane takes 16 contiguous codes (columns 64 pr + 16 g +
//     [0, 16)) with ONE 16 B load and feeds k-steps 2 pr and 2 pr + 1 from its
//     two halves; Q^T is loaded once in the same order (32 contiguous bytes
//     per lane and pair) and kept for the chunk. D 64: one pair, D 128: two,
//     D 96: one pair and one 8 B load (columns 64 + 8 g), D 32: one 8 B load.
//     The paired form is the only one built: it halves the K load
//     instructions (8 -> 4 per tile and lane at D 128) and costs no register
//     or instruction elsewhere. The 8 B form was not timed against it
//     (profiles/PERF.md "Int8 verify").
//   O^T[d][q] += V^T P^T, A = round16((u - 128) * v_scale[j]): one fp32 product
//     rounded once, which is what kv8_load_paged puts into the staging cache,
//     so the rounding point of V is that of the staged route. It is converted
//     in registers on the way global (16 codes per 16 B load) -> registers ->
//     2 x ds_write_b128 -> ds_read_b64_tr_b16, into the wave-private 32-row
//     tile of attn_verify.hip. v_scale is NOT folded into P, for either type:
//     p * v_scale falls into fp16's subnormal range at ordinary V magnitudes,
//     and one rounding rule for both types keeps one bound in the tests.
//   Conversion, VALU ops per element as the source asks for them:
//     K fp16   1     v_perm_b32 builds two halves 0x6400 | u (= 1024 + u), one
//                    v_pk_add_f16 subtracts 1152 from both
//     K bf16   2.5   v_cvt_f32_ubyteN, v_sub_f32 128, and half a v_perm_b32 /
//                    v_and_or that keeps the upper halves (exact: 7 bits);
//                    gfx950 has no packed bf16 subtract
//     V        3.5   v_cvt_f32_ubyteN, v_subrev 128, v_mul_f32 by the scale,
//                    half a v_cvt_pk_{f16,bf16}_f32 (the product is kept an
//                    fp32 multiply of its own: fused into the fp16 convert it
//                    would round once instead of twice and lose a zero's sign)
//   Register double buffer: K codes, V codes and both scales of the wave's
//   next tile are loaded before the current tile's arithmetic, and its pool
//   row (one table lookup per tile, in memory, so a table row may have any
//   number of entries) one tile earlier still. The loads are straight-line
//   code: past the chunk's last tile they read row 0 of page 0 and the result
//   is dropped. Rows of a live tile past key st + n - 1 lie inside the page;
//   their scores are replaced by the causal mask (a select, so a NaN scale
//   does not spread) and their V scale by 0.
// Tiles with kt + 31 <= st lie below every row's diagonal and skip the mask.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; no
// spill and no scratch in any of the 8 instantiations) are in the table at
// kv8_verify_split_kernel. Built without packed fp32 VALU ops (ops/build.py
// SOURCE_FLAGS).

#include "attn_kv8.h"

#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <type_traits>

void kv8_quantize_paged(at::Tensor qkv, at::Tensor k_pool, at::Tensor v_pool,
                        at::Tensor k_scale, at::Tensor v_scale, at::Tensor block_table,
                        at::Tensor lens, at::Tensor start);  // attn_kv8.hip

namespace {

constexpr int VNW = 4;      // waves per workgroup
constexpr int VT = 32;      // keys per wave tile
constexpr int VSPLITS = 8;  // workgroups per (b, h), as the decode ops

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

// Eight codes (two dwords, first code in the low byte) as the exact values
// u - 128 of an MFMA operand.
template <bool F16>
ZTA_DEV bf16x8 code_frag(unsigned lo, unsigned hi) {
  union {
    unsigned u[4];
    bf16x8 v8;
  } out;
  const unsigned w[2] = {lo, hi};
  if constexpr (F16) {
    // 0x6400 | u is the fp16 1024 + u, and (1024 + u) - 1152 = u - 128 exactly
    const f16x2 bias = {(_Float16)1152.0f, (_Float16)1152.0f};
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const unsigned p0 = __builtin_amdgcn_perm(0x64646464u, w[d], 0x04010400u);
      const unsigned p1 = __builtin_amdgcn_perm(0x64646464u, w[d], 0x04030402u);
      out.u[2 * d] = __builtin_bit_cast(unsigned, __builtin_bit_cast(f16x2, p0) - bias);
      out.u[2 * d + 1] = __builtin_bit_cast(unsigned, __builtin_bit_cast(f16x2, p1) - bias);
    }
  } else {
    // |u - 128| <= 127 has 7 significant bits: the upper half of its fp32 is exact
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float a = (float)((w[j >> 1] >> (16 * (j & 1))) & 0xffu) - 128.f;
      const float b = (float)((w[j >> 1] >> (16 * (j & 1) + 8)) & 0xffu) - 128.f;
      out.u[j] = (__builtin_bit_cast(unsigned, a) >> 16) |
                 (__builtin_bit_cast(unsigned, b) & 0xffff0000u);
    }
  }
  return out.v8;
}

// Codes 2 i and 2 i + 1 of dword w (i = 0, 1) times sc, each one fp32 product
// rounded once to the element type: the bits of kv8_load_kernel.
template <bool F16>
ZTA_DEV unsigned value_pair(unsigned w, int i, float sc) {
  float a = ((float)((w >> (16 * i)) & 0xffu) - 128.f) * sc;
  float b = ((float)((w >> (16 * i + 8)) & 0xffu) - 128.f) * sc;
  asm("" : "+v"(a), "+v"(b));  // keep the fp32 products (file header)
  return pack2<F16>(a, b);
}

// Resources (fp16 / bf16), no spills, no scratch:
//            VGPRs       AGPRs   LDS bytes   waves / SIMD
//   D 32      87 / 88      8      12288       5
//   D 64     112 / 113    16      20480       4 / 3
//   D 96     156 / 154    24      28672       2
//   D 128    185 / 183    32      36864       2
template <int D, bool F16>
__global__ __launch_bounds__(VNW * 64) void kv8_verify_split_kernel(
    const uint16_t* __restrict__ qkv, const uint8_t* __restrict__ kp,
    const uint8_t* __restrict__ vp, const float* __restrict__ ksc,
    const float* __restrict__ vsc, const float* __restrict__ slopes,
    float* __restrict__ part,  // (B * T * H, splits, 2 + 64 * DPL)
    const int* __restrict__ bt, const int* __restrict__ lens,
    const int* __restrict__ start, int H, int T, int C, Pool pl,
    int r_shift,     // log2(R) if R is a power of two, else -1
    float scale2) {  // D^-1/2 * log2(e)
  constexpr int KS = D / 32;   // k-steps of a score tile
  constexpr int KP = KS / 2;   // of them in pairs fed by one 16 B load
  constexpr int DB = D / 16;   // 16-column blocks of O^T
  constexpr int VC = D / 32;   // 16-code chunks of the V tile per lane
  constexpr int C16 = D / 16;  // 16-code chunks per row
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
  const auto [st, n] = seq_range(lens, start, b, T, pl.M * pl.R);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int L = lane & 15;  // this lane's query row
  const int g = lane >> 4;
  const int s_end = st + n;  // keys [0, s_end) are live; <= M * R
  const int ntiles = (s_end + VT - 1) / VT;
  const int tps = (ntiles + splits - 1) / splits;
  const int t_lo = split * tps;
  const int t_hi = n > 0 ? min(ntiles, t_lo + tps) : 0;  // no live row: no tile

  constexpr float LOG2E = 1.4426950408889634f;
  constexpr float LN2 = 0.6931471805599453f;
  const float slope2 = slopes[h] * LOG2E;
  const bool ok = L < n;  // n <= T
  const int pi = st + L;  // position of this lane's row

  // column of k-step s, element 0, for this lane: K's and Q's alike
  auto kcol = [&](int s) {
    return s < 2 * KP ? (s >> 1) * 64 + 16 * g + 8 * (s & 1) : s * 32 + 8 * g;
  };
  bf16x8 qf[KS];
  {
    const long qrow = ((long)b * T + L) * 3 * C + (long)h * D;
#pragma unroll
    for (int s = 0; s < KS; ++s)
      qf[s] = ok ? *reinterpret_cast<const bf16x8*>(&qkv[qrow + kcol(s)]) : bf16x8{};
  }

  float m_run = NEG_INF, l_run = 0.f;
  f32x4 o_acc[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d) o_acc[d] = f32x4{};

  // What a lane holds of one tile: per 16-key half its key row's codes (dwords
  // 2 s, 2 s + 1 feed k-step s) and the scales of keys 4 g + r; 16-code chunks
  // it * 64 + lane of the V tile with their rows' scales.
  struct TileRegs {
    unsigned k[2][2 * KS];
    f32x4 ks[2];
    uint4 v[VC];
    float vs[VC];
  };

  // First pool row (of head h) of tile t; row 0 of page 0 past the chunk.
  auto tile_row = [&](int t) -> long {
    const bool live = t < t_hi;
    const int kt = (live ? t : 0) * VT;  // < s_end <= M * R for a live tile
    const int pidx = min(r_shift >= 0 ? kt >> r_shift : kt / pl.R, pl.M - 1);
    const int page = page_of(bt, b, pidx, pl);
    return live ? ((long)page * H + h) * pl.R + (kt - pidx * pl.R) : 0;
  };
  // Rows prow + [0, 32) -> registers: inside one page, hence inside the pools.
  auto issue = [&](long prow, int t) {
    TileRegs r;
    const uint8_t* kb = kp + prow * D;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const uint8_t* kr = kb + (sub * 16 + L) * D;
#pragma unroll
      for (int pr = 0; pr < KP; ++pr) {
        const uint4 x = *reinterpret_cast<const uint4*>(kr + pr * 64 + 16 * g);
        r.k[sub][4 * pr] = x.x;
        r.k[sub][4 * pr + 1] = x.y;
        r.k[sub][4 * pr + 2] = x.z;
        r.k[sub][4 * pr + 3] = x.w;
      }
      if constexpr (KS & 1) {
        const uint2 x = *reinterpret_cast<const uint2*>(kr + (KS - 1) * 32 + 8 * g);
        r.k[sub][2 * KS - 2] = x.x;
        r.k[sub][2 * KS - 1] = x.y;
      }
      r.ks[sub] = *reinterpret_cast<const f32x4*>(ksc + prow + sub * 16 + 4 * g);
    }
    const int last = s_end - 1 - t * VT;  // last live row of the tile
#pragma unroll
    for (int it = 0; it < VC; ++it) {
      const int c = it * 64 + lane;
      r.v[it] = *reinterpret_cast<const uint4*>(vp + prow * D + c * 16);
      const float s = vsc[prow + c / C16];
      r.vs[it] = c / C16 <= last ? s : 0.f;
    }
    return r;
  };

  char* vl = smem + wave * WBYTES;  // this wave's V tile, later its merge image
  int t = t_lo + wave;
  TileRegs cur = issue(tile_row(t), t);
  long row_nxt = tile_row(t + VNW);
  for (; t < t_hi; t += VNW) {
    const TileRegs nxt = issue(row_nxt, t + VNW);
    row_nxt = tile_row(t + 2 * VNW);
    const int kt = t * VT;

    // V tile -> LDS as 16-bit values (after the previous tile's transpose
    // reads: DS order)
#pragma unroll
    for (int it = 0; it < VC; ++it) {
      const int c = it * 64 + lane;
      const unsigned w[4] = {cur.v[it].x, cur.v[it].y, cur.v[it].z, cur.v[it].w};
      unsigned o[8];
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        o[2 * d] = value_pair<F16>(w[d], 0, cur.vs[it]);
        o[2 * d + 1] = value_pair<F16>(w[d], 1, cur.vs[it]);
      }
      uint4* dst = reinterpret_cast<uint4*>(vl + (c / C16) * VROW + (c % C16) * 32);
      dst[0] = uint4{o[0], o[1], o[2], o[3]};
      dst[1] = uint4{o[4], o[5], o[6], o[7]};
    }

    // ---- S^T tiles: C[i = key][j = q] = mfma(A = codes of K, B = Q^T) ----
    f32x4 s_acc[2];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      s_acc[sub] = f32x4{};
#pragma unroll
      for (int s = 0; s < KS; ++s)
        s_acc[sub] = mfma16x32<F16>(code_frag<F16>(cur.k[sub][2 * s], cur.k[sub][2 * s + 1]),
                                    qf[s], s_acc[sub]);
    }

    // ---- online softmax of row L, log2 domain; register e holds key
    // kt + 16 * (e >> 2) + 4 g + (e & 3). Wave-uniform mask test. ----
    float sv[8];
    float tile_max = NEG_INF;
    if (kt + VT - 1 <= st) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int kj = kt + 16 * (e >> 2) + 4 * g + (e & 3);
        sv[e] = s_acc[e >> 2][e & 3] * (cur.ks[e >> 2][e & 3] * scale2) +
                slope2 * (float)(kj - pi);
        tile_max = fmaxf(tile_max, sv[e]);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int kj = kt + 16 * (e >> 2) + 4 * g + (e & 3);
        float x = s_acc[e >> 2][e & 3] * (cur.ks[e >> 2][e & 3] * scale2) +
                  slope2 * (float)(kj - pi);
        if (kj > pi || !ok) x = NEG_INF;  // also every key >= s_end
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
    cur = nxt;
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

}  // namespace

at::Tensor attn_verify_paged_q8(at::Tensor qkv, at::Tensor k_pool, at::Tensor v_pool,
                                at::Tensor k_scale, at::Tensor v_scale, at::Tensor slopes,
                                at::Tensor block_table, at::Tensor lens, at::Tensor start) {
  const char* op = "attn_verify_paged_q8";
  const Pool pl = check_kv8(op, k_pool, v_pool, k_scale, v_scale, block_table, {&lens, &start});
  check_qkv(op, qkv, k_pool, block_table);
  TORCH_CHECK(qkv.size(1) <= 16, op, ": at most 16 rows per sequence, got ", qkv.size(1));
  TORCH_CHECK(slopes.numel() == k_pool.size(1), op, ": slopes must have one entry per head");
  // the kernel's 16 B loads: a tile starts at a multiple of 32 rows
  for (const at::Tensor* t : {&qkv, &k_pool, &v_pool, &k_scale})
    TORCH_CHECK((uintptr_t)t->data_ptr() % 16 == 0, op, ": tensors must be 16-byte aligned");
  const bool f16 = qkv.scalar_type() == at::kHalf;
  const int B = qkv.size(0), T = qkv.size(1), C = qkv.size(2) / 3;
  const int H = k_pool.size(1), D = k_pool.size(3);
  auto o = at::empty({B, T, C}, qkv.options());
  if (B == 0 || T == 0) return o;
  auto sl = slopes.to(at::kFloat).contiguous();
  kv8_quantize_paged(qkv, k_pool, v_pool, k_scale, v_scale, block_table, lens, start);
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const int r_shift = (pl.R & (pl.R - 1)) == 0 ? __builtin_ctz(pl.R) : -1;
  attn::with_head_dim(D, [&](auto d) {  // check_kv8 admits only its four sizes
    constexpr int DD = decltype(d)::value;
    constexpr int DPL = (DD + 63) / 64;
    auto part = at::empty({(long)B * T * H, VSPLITS, 2 + 64 * DPL},
                          qkv.options().dtype(at::kFloat));
    auto launch = [&](auto f16c) {
      constexpr bool F = decltype(f16c)::value;
      hipLaunchKernelGGL((kv8_verify_split_kernel<DD, F>), dim3(B * H, VSPLITS),
                         dim3(VNW * 64), 0, stream, (const uint16_t*)qkv.data_ptr(),
                         k_pool.data_ptr<uint8_t>(), v_pool.data_ptr<uint8_t>(),
                         k_scale.data_ptr<float>(), v_scale.data_ptr<float>(),
                         sl.data_ptr<float>(), part.data_ptr<float>(),
                         block_table.data_ptr<int>(), lens.data_ptr<int>(),
                         start.data_ptr<int>(), H, T, C, pl, r_shift,
                         1.4426950408889634f / sqrtf((float)DD));
      hipLaunchKernelGGL((attn_decode_merge_kernel<DPL, F>), dim3(B * T * H), dim3(64), 0,
                         stream, part.data_ptr<float>(), (uint16_t*)o.data_ptr(), DD,
                         VSPLITS);
    };
    if (f16)
      launch(std::true_type{});
    else
      launch(std::false_type{});
  });
  return o;
}
