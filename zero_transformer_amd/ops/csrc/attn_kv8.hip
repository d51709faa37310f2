// Int8 paged KV cache for gfx950: a quantizing append, a dequantizing load
// into a 16-bit staging cache, and a native int8 decode attention.
//
//   k_pool / v_pool    (P, H, R, D) uint8: code u = q + 128, q in [-127, 127]
//   k_scale / v_scale  (P, H, R) fp32: one scale per cached row and head
//   value of a code    (u - 128) * scale
//   quantizer (fp32)   scale = max_d |x| / 127, q = rint(x / scale) clamped to
//                      +-127; a zero row has scale 0 and every code 128
//                      (reference.quantize_kv_rows; the division is a true
//                      fp32 division, so the bits match)
//   block_table, lens, start: as in attn_paged.hip, clamped in the same way.
//
//   kv8_quantize_paged(qkv (B,T,3C), k_pool, v_pool, k_scale, v_scale,
//                      block_table, lens, start)
//     rows i < n of sequence b: the K and V columns are quantized per head
//     into logical row st + i, and overwritten in qkv by (u - 128) * scale
//     rounded once to qkv's type, so that the 16-bit prefill / verify kernels
//     attend over what the cache holds.
//   kv8_load_paged(k_pool, v_pool, k_scale, v_scale, block_table, rows (B),
//                  k_dst, v_dst (B,H,S,D) 16-bit)
//     rows [0, min(rows[b], S, M R)) of the destinations <- (u - 128) * scale.
//   attn_decode_paged_q8(qkv (B,1,3C), pools, scales, slopes, block_table,
//                        lens) -> (B,1,C)
//     attn_decode_paged with the new row quantized before it is stored.
//
// kv8_quantize_kernel: one item = the D elements of one (row, head, K | V).
// A 16-lane row of a wave takes an item, lane r < D / 8 holding 16 B of it
// (D <= 128); the amax is a 4-step butterfly inside the 16 lanes, the codes
// leave as 8 B per lane, the scale from lane 0. Four items per wave, all
// shuffles in wave-uniform control flow. <DECODE> takes (st, n) = (S - 1, 1)
// from lens alone and leaves qkv as it is.
//
// kv8_load_kernel: one item = 16 codes (a 16 B load), two 16 B stores.
//
// kv8_decode_split_kernel<D, F16, REGTAB>: grid (B H, 8), four waves; the
// block's key range [lo, hi) is that of paged_decode_split_kernel (chunk =
// ceil(S / 8)).
// A 16 B load covers 16 codes of a key row, so LPK = D / 16 lanes share a key
// and a wave scores G = 64 / LPK keys per load instruction (8 at D 128, 10 at
// D 96 with four idle lanes, 16 at D 64, 32 at D 32). Iteration t of a wave
// takes keys lo + t G + [0, G), t = wave, wave + 4, ...: a function of S
// alone, so the result depends neither on R nor on the table. Each lane looks
// its key's page up itself (the table row sits in a register, lane i holding
// entry i, read with one cross-lane move; rows of more than 64 entries look
// up in memory). Per key: 16 products on the VALU against q held as fp32, a
// sum over the LPK lanes, one multiply by k_scale[j] D^-1/2 log2 e, the ALiBi
// term, and the online softmax in the log2 domain, one (m, l) per key slot.
// The running max moves only when a score exceeds it by more than 11.5 bits
// (wave-uniform test), so the accumulators are rarely rescaled. For V each
// lane accumulates sum_j w_j (u_j - 128) for its 16 columns, w_j = p_j
// v_scale[j]. Codes and scales of the next iteration are loaded before the
// arithmetic of the current one (register double buffer). The 4 G key slots
// of the block are merged through LDS into the partial {m ln 2, l, acc[D]}
// that attn_decode_merge_kernel (attn_kv.h) expects. No atomics.
//
// The -128 offset is subtracted per element after the conversion ((float)u -
// 128 is exact), not folded out as dot(q, u) - 128 sum q: the folded form
// cancels and would put 2^-24 * 128 * scale_j * sum_d |q_d| on every score.
// With the subtraction the only error against the exact dequantized cache is
// that of fp32 accumulation, and the tests' bound has no extra term.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; no
// spills, no scratch anywhere in this file):
//   kernel (REGTAB / table in memory)    VGPRs    LDS B   waves/SIMD
//   kv8_decode_split_kernel<32,  *>      75 / 73  17408   6
//   kv8_decode_split_kernel<64,  *>      76 / 74  16896   6
//   kv8_decode_split_kernel<96,  *>      80 / 78  15680   6
//   kv8_decode_split_kernel<128, *>      77 / 75  16640   6
//   kv8_quantize_kernel<*, *>            36 - 43  0       8
//   kv8_load_kernel<*>                   26       0       8
// The compiler converts a code as a byte-selecting integer add of -128 and
// one v_cvt_f32_i32: two VALU ops per element, as many as a byte-to-float
// conversion and a subtraction.

#include "attn_kv8.h"

#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <type_traits>

namespace {

constexpr int NW = 4;      // waves per decode block
constexpr int SPLITS = 8;  // decode blocks per (b, h), as attn_paged.hip

template <bool F16>
ZTA_DEV float cvt16(uint16_t u) {
  if constexpr (F16) {
    return (float)__builtin_bit_cast(_Float16, u);
  } else {
    return bf16_to_f32(u);
  }
}

// Byte i of w as a float, minus the code offset: exact.
ZTA_DEV float code(unsigned w, int i) { return (float)((w >> (8 * i)) & 0xffu) - 128.f; }

// v_exp_f32 as it is: the arguments here are differences to a running max
// (<= 11.5), and a result below the normal range may flush to zero.
ZTA_DEV float ex2(float x) { return __builtin_amdgcn_exp2f(x); }

// Row index (page, h, j % R) of logical row j of sequence b in a (P, H, R)
// plane set; j < M * R.
ZTA_DEV long pool_row(const int* __restrict__ bt, int b, int h, int H, int j, Pool pl) {
  const int page = page_of(bt, b, j / pl.R, pl);
  return ((long)page * H + h) * pl.R + j % pl.R;
}

template <bool F16, bool DECODE>
__global__ __launch_bounds__(256) void kv8_quantize_kernel(
    uint16_t* __restrict__ qkv, uint8_t* __restrict__ kp, uint8_t* __restrict__ vp,
    float* __restrict__ ksc, float* __restrict__ vsc, const int* __restrict__ bt,
    const int* __restrict__ lens, const int* __restrict__ start, int B, int H, int T,
    int C, int D, Pool pl) {
  const int r = threadIdx.x & 15;
  const bool act = r < D / 8;
  const long items = (long)B * T * H * 2;
  // the trip count is the same for every lane of the block: the shuffles
  // below run in uniform control flow
  for (long base = (long)blockIdx.x * 16; base < items; base += (long)gridDim.x * 16) {
    const long it = base + (threadIdx.x >> 4);
    bool live = it < items;
    int kv = 0, h = 0, i = 0, b = 0, st = 0;
    if (live) {
      kv = (int)(it & 1);
      h = (int)((it >> 1) % H);
      const long row = it / (2 * H);
      i = (int)(row % T);
      b = (int)(row / T);
      int n;
      if constexpr (DECODE) {
        const int S = min(max(lens[b], 0), pl.M * pl.R);
        st = S - 1;
        n = S > 0 ? 1 : 0;
      } else {
        const auto sr = seq_range(lens, start, b, T, pl.M * pl.R);
        st = sr.st;
        n = sr.n;
      }
      live = i < n;
    }
    uint16_t* src = qkv + ((long)b * T + i) * 3 * C + (long)(1 + kv) * C + h * D + r * 8;
    s16x8 x{};
    if (live && act) x = *reinterpret_cast<const s16x8*>(src);
    float f[8];
    float amax = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      f[e] = cvt16<F16>((uint16_t)x[e]);
      amax = fmaxf(amax, fabsf(f[e]));
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off, WAVE));
    if (!live) continue;
    const float scale = amax / 127.f;  // true division: bit-equal to the reference
    const float safe = scale > 0.f ? scale : 1.f;
    unsigned w[2] = {0u, 0u};
    float dq[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float q = fminf(fmaxf(rintf(f[e] / safe), -127.f), 127.f);
      w[e >> 2] |= (unsigned)((int)q + 128) << (8 * (e & 3));
      dq[e] = (float)(int)q * scale;  // from the code: a rounded -0 is stored as +0
    }
    const long prow = pool_row(bt, b, h, H, st + i, pl);  // st + i < M * R
    if (act) {
      *reinterpret_cast<uint2*>((kv ? vp : kp) + prow * D + r * 8) = uint2{w[0], w[1]};
      if constexpr (!DECODE) {
        *reinterpret_cast<uint4*>(src) =
            uint4{pack2<F16>(dq[0], dq[1]), pack2<F16>(dq[2], dq[3]),
                  pack2<F16>(dq[4], dq[5]), pack2<F16>(dq[6], dq[7])};
      }
    }
    if (r == 0) (kv ? vsc : ksc)[prow] = scale;
  }
}

template <bool F16>
__global__ __launch_bounds__(256) void kv8_load_kernel(
    const uint8_t* __restrict__ kp, const uint8_t* __restrict__ vp,
    const float* __restrict__ ksc, const float* __restrict__ vsc,
    const int* __restrict__ bt, const int* __restrict__ rows, uint16_t* __restrict__ kd,
    uint16_t* __restrict__ vd, int B, int H, int S, int D, Pool pl) {
  const int cpr = D / 16;
  const long total = (long)B * H * S * 2 * cpr;
  for (long it = (long)blockIdx.x * blockDim.x + threadIdx.x; it < total;
       it += (long)gridDim.x * blockDim.x) {
    const int c = (int)(it % cpr);
    const int kv = (int)((it / cpr) & 1);
    const long row = it / (2 * cpr);  // (b, h, j)
    const int j = (int)(row % S);
    const int h = (int)((row / S) % H);
    const int b = (int)(row / ((long)S * H));
    if (j >= min(min(max(rows[b], 0), S), pl.M * pl.R)) continue;
    const long prow = pool_row(bt, b, h, H, j, pl);
    const uint4 u = *reinterpret_cast<const uint4*>((kv ? vp : kp) + prow * D + c * 16);
    const float sc = (kv ? vsc : ksc)[prow];
    const unsigned uw[4] = {u.x, u.y, u.z, u.w};
    unsigned o[8];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      o[2 * d] = pack2<F16>(code(uw[d], 0) * sc, code(uw[d], 1) * sc);
      o[2 * d + 1] = pack2<F16>(code(uw[d], 2) * sc, code(uw[d], 3) * sc);
    }
    uint4* dst = reinterpret_cast<uint4*>((kv ? vd : kd) + row * D + c * 16);
    dst[0] = uint4{o[0], o[1], o[2], o[3]};
    dst[1] = uint4{o[4], o[5], o[6], o[7]};
  }
}

// What a lane holds of one key: 16 codes of K and of V, the row's two scales.
struct KeyRegs {
  uint4 k, v;
  float ks, vs;
  int j;
  bool ok;
};

// REGTAB: the table row fits the wave's registers (M <= 64).
template <int D, bool F16, bool REGTAB>
__global__ __launch_bounds__(NW * 64) void kv8_decode_split_kernel(
    const uint16_t* __restrict__ qkv,  // (B, 3C): only q is read here
    const uint8_t* __restrict__ kp, const uint8_t* __restrict__ vp,
    const float* __restrict__ ksc, const float* __restrict__ vsc,
    const float* __restrict__ slopes,
    float* __restrict__ part,  // (BH, SPLITS, 2 + 64 * DPL)
    const int* __restrict__ bt, const int* __restrict__ lens, int H, int C, Pool pl,
    int r_shift,     // log2(R) if R is a power of two, else -1
    float scale2) {  // D^-1/2 * log2(e)
  constexpr int LPK = D / 16;   // lanes per key
  constexpr int G = 64 / LPK;   // keys per wave and load
  constexpr int NSLOT = NW * G;  // key slots of the block
  constexpr int DPL = (D + 63) / 64;
  constexpr float LOG2E = 1.4426950408889634f;
  constexpr float LN2 = 0.6931471805599453f;
  constexpr float DEFER_THR = 11.5f;  // ~8 nats, as the flash kernels
  __shared__ __attribute__((aligned(16))) float red_acc[NSLOT * D];
  __shared__ float red_ml[NSLOT * 2];

  const int bh = blockIdx.x;
  const int b = bh / H, h = bh % H;
  const int S = min(max(lens[b], 0), pl.M * pl.R);
  const int split = blockIdx.y;
  const int chunk = (S + SPLITS - 1) / SPLITS;
  const int lo = split * chunk;
  const int hi = min(S, lo + chunk);
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int ks = lane / LPK;   // key slot within the wave; == G on idle lanes
  const int sub = lane % LPK;  // which 16 columns
  const bool kvalid = ks < G;
  // independent of S: issued together with the length and the q loads
  const int my_entry = bt[(long)b * pl.M + min(lane, pl.M - 1)];
  const float slope2 = slopes[h] * LOG2E;

  float q[16];
  {
    const uint16_t* qr = qkv + (long)b * 3 * C + (long)h * D + sub * 16;
    const s16x8 q0 = *reinterpret_cast<const s16x8*>(qr);
    const s16x8 q1 = *reinterpret_cast<const s16x8*>(qr + 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      q[e] = cvt16<F16>((uint16_t)q0[e]);
      q[8 + e] = cvt16<F16>((uint16_t)q1[e]);
    }
  }

  // Loads of iteration t: this lane's key is lo + t * G + ks. Straight-line
  // code, so that the compiler's wait counts stay exact and the loads stay in
  // flight over the arithmetic: a lane without a key reads row 0 of page 0
  // (always inside the pool) and drops what it gets.
  auto issue = [&](int t) {
    KeyRegs g;
    g.j = lo + t * G + ks;
    g.ok = kvalid && g.j < hi;
    // j < hi <= S <= M * R for a live key: the clamp only meets dead ones
    const int pidx = min(r_shift >= 0 ? g.j >> r_shift : g.j / pl.R, pl.M - 1);
    const int entry =
        REGTAB ? __shfl(my_entry, pidx, WAVE) : bt[(long)b * pl.M + pidx];
    const int page = min(max(entry, 0), pl.P - 1);
    const long prow = g.ok ? ((long)page * H + h) * pl.R + (g.j - pidx * pl.R) : 0;
    g.k = *reinterpret_cast<const uint4*>(kp + prow * D + sub * 16);
    g.v = *reinterpret_cast<const uint4*>(vp + prow * D + sub * 16);
    g.ks = ksc[prow];
    g.vs = vsc[prow];
    return g;
  };

  float m = NEG_INF, l = 0.f;
  float acc[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) acc[c] = 0.f;

  KeyRegs cur = issue(wave);
  for (int t = wave; lo + t * G < hi; t += NW) {  // wave-uniform
    const KeyRegs nxt = issue(t + NW);
    const unsigned kw[4] = {cur.k.x, cur.k.y, cur.k.z, cur.k.w};
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int i = 0; i < 4; ++i) s += q[4 * d + i] * code(kw[d], i);
    if constexpr ((LPK & (LPK - 1)) == 0) {
#pragma unroll
      for (int off = LPK / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, WAVE);
    } else {  // D 96: the same order in every lane of the group
      float tot = 0.f;
#pragma unroll
      for (int k = 0; k < LPK; ++k) tot += __shfl(s, min(ks * LPK + k, 63), WAVE);
      s = tot;
    }
    s = s * (cur.ks * scale2) + slope2 * (float)(cur.j - (S - 1));
    const float vs = cur.ok ? cur.vs : 0.f;  // a dead lane's loads may hold anything

    const bool need = cur.ok && s > m + DEFER_THR;
    if (__any(need)) {
      const float mn = need ? s : m;
      const float alpha = need ? ex2(m - mn) : 1.f;  // first key: exp2(-huge) = 0
      m = mn;
      l *= alpha;
#pragma unroll
      for (int c = 0; c < 16; ++c) acc[c] *= alpha;
    }
    const float p = cur.ok ? ex2(s - m) : 0.f;
    l += p;
    const float w = p * vs;
    const unsigned vw[4] = {cur.v.x, cur.v.y, cur.v.z, cur.v.w};
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[4 * d + i] += w * code(vw[d], i);
    cur = nxt;
  }

  // merge the block's key slots; slot s holds keys lo + s, lo + s + NSLOT, ...
  // and is empty iff s >= hi - lo
  if (kvalid) {
    const int slot = wave * G + ks;
    if (sub == 0) {
      red_ml[2 * slot] = m;
      red_ml[2 * slot + 1] = l;
    }
    f32x4* dst = reinterpret_cast<f32x4*>(&red_acc[slot * D + sub * 16]);
#pragma unroll
    for (int c = 0; c < 4; ++c)
      dst[c] = f32x4{acc[4 * c], acc[4 * c + 1], acc[4 * c + 2], acc[4 * c + 3]};
  }
  __syncthreads();
  const int tid = threadIdx.x;
  if (tid < 64 * DPL) {
    const int nsl = min(NSLOT, max(hi - lo, 0));
    float mg = NEG_INF;
    for (int s = 0; s < nsl; ++s) mg = fmaxf(mg, red_ml[2 * s]);
    float lg = 0.f, og = 0.f;
    for (int s = 0; s < nsl; ++s) {
      const float f = ex2(red_ml[2 * s] - mg);  // a live slot's m is finite
      lg += red_ml[2 * s + 1] * f;
      if (tid < D) og += red_acc[s * D + tid] * f;
    }
    float* pr = &part[((long)bh * SPLITS + split) * (2 + 64 * DPL)];
    if (tid == 0) {
      pr[0] = nsl > 0 ? mg * LN2 : NEG_INF;  // the merge kernel works in nats
      pr[1] = lg;
    }
    pr[2 + tid] = og;
  }
}

template <bool DECODE>
void launch_quantize(at::Tensor& qkv, at::Tensor& kp, at::Tensor& vp, at::Tensor& ksc,
                     at::Tensor& vsc, const at::Tensor& bt, const int* lens,
                     const int* start, Pool pl, hipStream_t stream) {
  const int B = qkv.size(0), T = qkv.size(1), C = qkv.size(2) / 3;
  const int H = kp.size(1), D = kp.size(3);
  const long items = (long)B * T * H * 2;
  auto launch = [&](auto f16c) {
    hipLaunchKernelGGL((kv8_quantize_kernel<decltype(f16c)::value, DECODE>),
                       dim3(capped_grid(items * 16, 256, 8192)), dim3(256), 0, stream,
                       (uint16_t*)qkv.data_ptr(), kp.data_ptr<uint8_t>(),
                       vp.data_ptr<uint8_t>(), ksc.data_ptr<float>(), vsc.data_ptr<float>(),
                       bt.data_ptr<int>(), lens, start, B, H, T, C, D, pl);
  };
  if (qkv.scalar_type() == at::kHalf)
    launch(std::true_type{});
  else
    launch(std::false_type{});
}

}  // namespace

void kv8_quantize_paged(at::Tensor qkv, at::Tensor k_pool, at::Tensor v_pool,
                        at::Tensor k_scale, at::Tensor v_scale, at::Tensor block_table,
                        at::Tensor lens, at::Tensor start) {
  const Pool pl = check_kv8("kv8_quantize_paged", k_pool, v_pool, k_scale, v_scale,
                            block_table, {&lens, &start});
  check_qkv("kv8_quantize_paged", qkv, k_pool, block_table);
  if (qkv.size(0) == 0 || qkv.size(1) == 0) return;
  launch_quantize<false>(qkv, k_pool, v_pool, k_scale, v_scale, block_table,
                         lens.data_ptr<int>(), start.data_ptr<int>(), pl,
                         at::hip::getCurrentHIPStreamMasqueradingAsCUDA());
}

void kv8_load_paged(at::Tensor k_pool, at::Tensor v_pool, at::Tensor k_scale,
                    at::Tensor v_scale, at::Tensor block_table, at::Tensor rows,
                    at::Tensor k_dst, at::Tensor v_dst) {
  const Pool pl = check_kv8("kv8_load_paged", k_pool, v_pool, k_scale, v_scale,
                            block_table, {&rows});
  const long B = block_table.size(0), H = k_pool.size(1), D = k_pool.size(3);
  TORCH_CHECK(k_dst.is_cuda() && v_dst.is_cuda() && k_dst.dim() == 4 &&
                  k_dst.is_contiguous() && v_dst.is_contiguous() &&
                  k_dst.sizes() == v_dst.sizes() &&
                  k_dst.scalar_type() == v_dst.scalar_type() &&
                  (k_dst.scalar_type() == at::kHalf || k_dst.scalar_type() == at::kBFloat16) &&
                  k_dst.size(0) == B && k_dst.size(1) == H && k_dst.size(3) == D,
              "kv8_load_paged: k_dst/v_dst must be (B, H, S, D) contiguous fp16 or bf16");
  const long S = k_dst.size(2);
  TORCH_CHECK(S < (1L << 31), "kv8_load_paged: S must fit in int32");
  if (B == 0 || S == 0) return;
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  auto launch = [&](auto f16c) {
    hipLaunchKernelGGL((kv8_load_kernel<decltype(f16c)::value>),
                       dim3(capped_grid(B * H * S * 2 * (D / 16), 256, 8192)), dim3(256), 0,
                       stream, k_pool.data_ptr<uint8_t>(), v_pool.data_ptr<uint8_t>(),
                       k_scale.data_ptr<float>(), v_scale.data_ptr<float>(),
                       block_table.data_ptr<int>(), rows.data_ptr<int>(),
                       (uint16_t*)k_dst.data_ptr(), (uint16_t*)v_dst.data_ptr(), (int)B,
                       (int)H, (int)S, (int)D, pl);
  };
  if (k_dst.scalar_type() == at::kHalf)
    launch(std::true_type{});
  else
    launch(std::false_type{});
}

at::Tensor attn_decode_paged_q8(at::Tensor qkv, at::Tensor k_pool, at::Tensor v_pool,
                                at::Tensor k_scale, at::Tensor v_scale, at::Tensor slopes,
                                at::Tensor block_table, at::Tensor lens) {
  const Pool pl = check_kv8("attn_decode_paged_q8", k_pool, v_pool, k_scale, v_scale,
                            block_table, {&lens});
  check_qkv("attn_decode_paged_q8", qkv, k_pool, block_table);
  TORCH_CHECK(qkv.size(1) == 1, "attn_decode_paged_q8: qkv must be (B, 1, 3C)");
  TORCH_CHECK(slopes.numel() == k_pool.size(1),
              "attn_decode_paged_q8: slopes must have one entry per head");
  const bool f16 = qkv.scalar_type() == at::kHalf;
  const long B = qkv.size(0), C = qkv.size(2) / 3;
  const int H = k_pool.size(1), D = k_pool.size(3);
  auto out = at::empty({B, 1, C}, qkv.options());
  if (B == 0) return out;
  auto sl = slopes.to(at::kFloat).contiguous();
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  launch_quantize<true>(qkv, k_pool, v_pool, k_scale, v_scale, block_table,
                        lens.data_ptr<int>(), nullptr, pl, stream);
  const int dpl = (D + 63) / 64;
  const int r_shift = (pl.R & (pl.R - 1)) == 0 ? __builtin_ctz(pl.R) : -1;
  auto part = at::empty({B * H, SPLITS, 2 + 64 * (long)dpl}, qkv.options().dtype(at::kFloat));
  attn::with_head_dim(D, [&](auto d) {
    constexpr int DD = decltype(d)::value;
    constexpr int DPL = (DD + 63) / 64;
    auto launch = [&](auto f16c, auto regc) {
      constexpr bool F = decltype(f16c)::value;
      hipLaunchKernelGGL((kv8_decode_split_kernel<DD, F, decltype(regc)::value>),
                         dim3(B * H, SPLITS),
                         dim3(NW * 64), 0, stream, (const uint16_t*)qkv.data_ptr(),
                         k_pool.data_ptr<uint8_t>(), v_pool.data_ptr<uint8_t>(),
                         k_scale.data_ptr<float>(), v_scale.data_ptr<float>(),
                         sl.data_ptr<float>(), part.data_ptr<float>(),
                         block_table.data_ptr<int>(), lens.data_ptr<int>(), H, (int)C, pl,
                         r_shift, 1.4426950408889634f / sqrtf((float)DD));
      hipLaunchKernelGGL((attn_decode_merge_kernel<DPL, F>), dim3(B * H), dim3(64), 0,
                         stream, part.data_ptr<float>(), (uint16_t*)out.data_ptr(), DD,
                         SPLITS);
    };
    auto by_table = [&](auto f16c) {
      if (pl.M <= 64)
        launch(f16c, std::true_type{});
      else
        launch(f16c, std::false_type{});
    };
    if (f16)
      by_table(std::true_type{});
    else
      by_table(std::false_type{});
  });
  return out;
}
