// Weight-only int4 ("W4A16") decode projections for gfx950, group-scaled.
//
//   y (B, N) = x (B, K) @ W^T,   W[n][k] = (u[n][k] - 8) * scale[n][k / 128]
//
// x, y: bf16 or fp16; packed: uint8 (N, K/2), two 4-bit codes u = q + 8 per
// byte; scale: fp32 (N, K/128), one per row and group of 128 consecutive k
// (the GPTQ / AWQ storage shape, symmetric). Every kernel accumulates the
// integer-weight products of a group in fp32, multiplies that partial sum by
// the group's scale once, adds it to an fp32 accumulator and rounds once to
// the output type, so the result is defined by (packed, scale, x) alone.
// The weight stream is a quarter of ops/csrc/gemv.hip's bytes.
//
// 1 <= B <= 16, K % 512 == 0, any N >= 1. Nothing is read on the host, no
// float atomics (same bits on every call), any workspace comes from torch's
// allocator at a size fixed by the shapes: every launch is graph-capturable.
//
// Nibble order (ops.reference.quantize_rows_w4 / unpack_rows_w4 define it).
// A row is a sequence of little-endian dwords of 8 codes each; dword d holds
// k = 8 d .. 8 d + 7, and its nibble j (bits 4 j .. 4 j + 3) holds
//
//     k = 8 d + [0, 2, 4, 6, 1, 3, 5, 7][j]
//
// so (dword >> 4 s) & 0x000F000F is the pair (k = 2 s, k = 2 s + 1) in the
// low and high half of a dword: OR-ing 0x6400 into both halves gives the two
// fp16 numbers 1024 + u, one packed subtract of 1032 gives (q, q') exactly,
// and s = 0..3 walks the dword in k order. A 16-byte load (32 codes, four
// dwords) therefore turns into four 8-k MFMA fragments, or 16 packed pairs
// lined up with x's own packing, at 3 VALU ops per pair and with no permute.
// bf16 has no packed subtract here: the codes go through fp32 (byte -> float
// convert of the masked dword, minus 8, upper half: |q| <= 8 is exact).
//
// Two bodies:
//
// * w4_gemv_kernel (B <= 4): one wave per output row, four rows per
//   256-thread workgroup. A lane's 16-byte load is 32 weights of ONE group
//   (128 % 32 == 0), so the lane needs one scale per step, multiplies its own
//   32-term partial sum by it and only then joins the 64-lane butterfly. A
//   wave step covers 2048 k; K % 2048 != 0 ends on a step with 16, 32 or 48
//   live lanes. fp16 multiplies the exact fp16 codes with x's halves straight
//   into fp32 (mixed-precision FMA: no convert of either operand); bf16
//   converts both to fp32.
//
// * w4_gemm_kernel (any B, meant for the rows the streaming body loses):
//   v_mfma_f32_16x16x32_{f16,bf16} with x as the A operand (row b = lane &
//   15; rows b >= B are zero fragments, never loaded) and a 16-row tile of W
//   as the B operand (column n = lane & 15). Lane (r, g = lane >> 4) takes
//   ONE 16-byte load of row n0 + r: the 32 codes k0 + 32 g .. + 32 of one
//   128-k group, i.e. the four lane groups cover exactly the group. Dword j
//   of the load feeds MFMA j; the x fragment of lane (b, g) for MFMA j is x[b]
//   [k0 + 32 g + 8 j .. + 8) (the k order inside an MFMA is free as long as
//   both operands agree). The four MFMAs run into a fresh partial tile whose
//   lane holds (b = 4 g + i, n = r): ONE scale per lane, tile and step,
//   acc += scale[n][group] * partial.
//
//   Work split. W4 rows are short (K = 2048 is 1 KB), so a matrix is a few
//   MB and the kernel lives on launch, staging and drain, not on bandwidth:
//   the split wants enough workgroups to cover the 256 CUs and as little
//   serial work in front of the first MFMA as possible. A workgroup (4 waves)
//   owns 64 rows (4 tiles) x one K chunk of `per` 512-wide units; fewer rows
//   per workgroup would raise the x bytes staged per weight byte, which at
//   B = 16 and 64 rows already equal the weight bytes (4 B / rows). The four
//   waves split the chunk's 128-k steps round robin (a unit is one step of
//   each wave: the workgroup reads 256 contiguous bytes of each row per
//   round) and each wave keeps all four tiles' accumulators, issuing the four
//   tiles' weight and scale loads together; the loads of the first step are
//   issued BEFORE x is staged to LDS, and those of step s + 1 before the
//   MFMAs of step s. The x chunk (B x chunk, <= 33 KB, so that four
//   workgroups share a CU's LDS) is staged once with coalesced 16-byte
//   loads, rows padded by 16 bytes against bank conflicts.
//   The waves' partial tiles are summed through LDS in wave order. Across
//   workgroups K is split `ksplit` ways (grid.y) when N / 64 row groups alone
//   leave CUs idle: each workgroup then writes its (already scaled) fp32
//   partial to a (ksplit, B, N) workspace and w4_reduce_kernel sums the
//   splits in index order and casts. ksplit depends on (N, K) only: see
//   pick_ksplit.
//
// w4_dequant_kernel: (packed, scale) -> 16-bit (N, K), 16 bytes in and 64
// bytes out per lane, bits equal to ops.reference.dequantize_rows_w4 (one
// fp32 product, one rounding). The many-row (prefill) path feeds it to the
// GEMM library (ops.linear_w4).

#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) _Float16 h16x2;
typedef __attribute__((ext_vector_type(8))) _Float16 h16x8;
typedef __attribute__((ext_vector_type(8))) __bf16 b16x8;

constexpr int GROUP = 128;  // k per scale

// DT 0 = bf16, 1 = fp16
template <int DT>
ZTA_DEV float act_to_f32(uint16_t bits) {
  if (DT == 0) return bf16_to_f32(bits);
  return float(__builtin_bit_cast(_Float16, bits));
}

template <int DT>
ZTA_DEV uint16_t f32_to_act(float v) {
  if (DT == 0) return f32_to_bf16(v);
  return __builtin_bit_cast(uint16_t, _Float16(v));  // RNE
}

// q of k = 8 d + i (i = 0..7) of dword `dw` as fp32: even nibbles (k 0, 4,
// 1, 5) are the bytes of dw & 0x0F0F0F0F, odd nibbles (k 2, 6, 3, 7) those of
// (dw >> 4) & 0x0F0F0F0F. Compiles to a bit-field extract, an integer add
// and a convert per code.
ZTA_DEV float code_to_f32(uint32_t dw, int i) {
  const uint32_t m = ((i & 2) ? (dw >> 4) : dw) & 0x0F0F0F0Fu;
  const int byte = 2 * (i & 1) + (i >> 2);
  return float((m >> (8 * byte)) & 0xFFu) - 8.0f;
}

// the pair (k = 8 d + 2 s, + 1) of dword `dw` as two exact fp16 q
ZTA_DEV h16x2 codes_to_f16x2(uint32_t dw, int s) {
  const h16x2 bias = {_Float16(1032.0f), _Float16(1032.0f)};
  const uint32_t h = ((dw >> (4 * s)) & 0x000F000Fu) | 0x64006400u;
  return __builtin_bit_cast(h16x2, h) - bias;
}

// ---------------------------------------------------------------------------
// Streaming body
// ---------------------------------------------------------------------------

// sum over the lane's 32 k of q * x for each of the B rows
template <int DT, int B>
ZTA_DEV void dot32(const u32x4 w, const s16x8* __restrict__ x, size_t xrow8, float* s) {
  if (DT == 1) {
    h16x2 qh[16];
#pragma unroll
    for (int p = 0; p < 16; ++p) qh[p] = codes_to_f16x2(w[p >> 2], p & 3);
#pragma unroll
    for (int b = 0; b < B; ++b) {
      float t = 0.0f;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const h16x8 xv = __builtin_bit_cast(h16x8, x[b * xrow8 + d]);
#pragma unroll
        for (int i = 0; i < 8; ++i)
          t = __builtin_fmaf(float(qh[4 * d + (i >> 1)][i & 1]), float(xv[i]), t);
      }
      s[b] = t;
    }
  } else {
    float wf[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) wf[i] = code_to_f32(w[i >> 3], i & 7);
#pragma unroll
    for (int b = 0; b < B; ++b) {
      float t = 0.0f;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const s16x8 xv = x[b * xrow8 + d];
#pragma unroll
        for (int i = 0; i < 8; ++i)
          t = __builtin_fmaf(wf[8 * d + i], bf16_to_f32(uint16_t(xv[i])), t);
      }
      s[b] = t;
    }
  }
}

template <int DT, int B>
__global__ __launch_bounds__(256) void w4_gemv_kernel(
    const s16x8* __restrict__ x,       // (B, K/8)
    const u32x4* __restrict__ packed,  // (N, K/32)
    const float* __restrict__ scale,   // (N, K/128)
    uint16_t* __restrict__ y,          // (B, N)
    int N, int K32) {
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + wave;
  if (n >= N) return;

  float acc[B];
#pragma unroll
  for (int b = 0; b < B; ++b) acc[b] = 0.0f;

  const u32x4* wr = packed + (size_t)n * K32;
  const float* sr = scale + (size_t)n * (K32 >> 2);
  const size_t xrow8 = (size_t)K32 * 4;
  // K32 % 64 is 0, 16, 32 or 48: in the last step of the latter three the
  // lanes from there on fail this test and idle
  for (int k32 = lane; k32 < K32; k32 += 64) {
    const u32x4 w = wr[k32];
    const float sc = sr[k32 >> 2];
    float s[B];
    dot32<DT, B>(w, x + (size_t)k32 * 4, xrow8, s);
#pragma unroll
    for (int b = 0; b < B; ++b) acc[b] = __builtin_fmaf(s[b], sc, acc[b]);
  }
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const float r = wave_reduce_sum(acc[b]);
    if (lane == 0) y[(size_t)b * N + n] = f32_to_act<DT>(r);
  }
}

// ---------------------------------------------------------------------------
// Matrix body
// ---------------------------------------------------------------------------

constexpr int TG = 4;            // 16-row tiles per workgroup (and per wave)
constexpr int GROUP_ROWS = 16 * TG;
constexpr int UNIT = 512;        // K granule of the split: one step per wave
constexpr int MAX_UNITS = 2;     // per workgroup: x chunk <= 16 x 1024 x 2 B
constexpr int XPAD = 8;          // 16-bit elements of padding per LDS x row
constexpr int RSTRIDE = GROUP_ROWS + 4;  // floats per b row of a partial tile

// the 8 codes of one dword -> MFMA fragment in k order
ZTA_DEV h16x8 codes_to_f16x8(uint32_t dw) {
  h16x8 out;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const h16x2 p = codes_to_f16x2(dw, s);
    out[2 * s] = p[0];
    out[2 * s + 1] = p[1];
  }
  return out;
}

ZTA_DEV b16x8 codes_to_bf16x8(uint32_t dw) {
  // |q| <= 8 has 4 significant bits: the upper half of its fp32 is exact
  s16x8 out;
#pragma unroll
  for (int i = 0; i < 8; ++i)
    out[i] = short(__builtin_bit_cast(uint32_t, code_to_f32(dw, i)) >> 16);
  return __builtin_bit_cast(b16x8, out);
}

template <int DT>
ZTA_DEV f32x4 mfma_w4(s16x8 xf, uint32_t dw, f32x4 c) {
  if (DT == 1) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(
        __builtin_bit_cast(h16x8, xf), codes_to_f16x8(dw), c, 0, 0, 0);
  } else {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(
        __builtin_bit_cast(b16x8, xf), codes_to_bf16x8(dw), c, 0, 0, 0);
  }
}

// grid (ceil(N / 64), ksplit); dynamic LDS = max(B * (per*512 + XPAD) * 2,
// 4 * 16 * RSTRIDE * 4) bytes. SPLIT: write fp32 partials to `part`
// (ksplit, B, N) instead of y.
template <int DT, bool SPLIT>
__global__ __launch_bounds__(256) void w4_gemm_kernel(
    const s16x8* __restrict__ x,         // (B, K/8)
    const uint8_t* __restrict__ packed,  // (N, K/2)
    const float* __restrict__ scale,     // (N, K/128)
    uint16_t* __restrict__ y,            // (B, N)
    float* __restrict__ part,            // (ksplit, B, N)
    int B, int N, int K, int per) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int r = lane & 15;  // W row of the tile / x row b
  const int g = lane >> 4;  // 32-k quarter of the group
  const int n0 = blockIdx.x * GROUP_ROWS;
  const int k0 = blockIdx.y * per * UNIT;
  const int klen = min(per * UNIT, K - k0);  // a multiple of 512, > 0
  const int steps = klen / UNIT;             // per wave
  const int xstride = klen + XPAD;           // 16-bit elements

  // this wave's step s is k0 + s * 512 + wave * 128 .. + 128
  const uint8_t* wrow[TG];
  const float* srow[TG];
#pragma unroll
  for (int t = 0; t < TG; ++t) {
    // rows past N re-read row N - 1; their results are never stored
    const int n = min(n0 + 16 * t + r, N - 1);
    wrow[t] = packed + ((size_t)n * K + k0 + wave * GROUP + 32 * g) / 2;
    srow[t] = scale + (size_t)n * (K / GROUP) + k0 / GROUP + wave;
  }
  u32x4 w[TG];
  float sc[TG];
#pragma unroll
  for (int t = 0; t < TG; ++t) {
    w[t] = *reinterpret_cast<const u32x4*>(wrow[t]);
    sc[t] = srow[t][0];
  }

  // stage x[:, k0 : k0 + klen) (coalesced 16-byte vectors)
  {
    const int vec_per_row = klen >> 3;
    const int total = B * vec_per_row;
    const int K8 = K >> 3;
    for (int v = tid; v < total; v += 256) {
      const int b = v / vec_per_row, c = v - b * vec_per_row;
      *reinterpret_cast<s16x8*>(smem + ((size_t)b * xstride + 8 * c) * 2) =
          x[(size_t)b * K8 + (k0 >> 3) + c];
    }
  }
  __syncthreads();

  f32x4 acc[TG];
#pragma unroll
  for (int t = 0; t < TG; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  const char* xrow = smem + ((size_t)r * xstride + wave * GROUP + 32 * g) * 2;
  const bool live = r < B;

  for (int s = 0; s < steps; ++s) {
    u32x4 wn[TG];
    float scn[TG];
    if (s + 1 < steps) {
#pragma unroll
      for (int t = 0; t < TG; ++t) {
        wn[t] = *reinterpret_cast<const u32x4*>(wrow[t] + (s + 1) * (UNIT / 2));
        scn[t] = srow[t][(s + 1) * (UNIT / GROUP)];
      }
    }
    s16x8 xf[4] = {s16x8{}, s16x8{}, s16x8{}, s16x8{}};
    if (live) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        xf[j] = *reinterpret_cast<const s16x8*>(xrow + 2 * s * UNIT + 16 * j);
    }
#pragma unroll
    for (int t = 0; t < TG; ++t) {
      f32x4 p = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int j = 0; j < 4; ++j) p = mfma_w4<DT>(xf[j], w[t][j], p);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[t][i] = __builtin_fmaf(p[i], sc[t], acc[t][i]);
    }
    if (s + 1 < steps) {
#pragma unroll
      for (int t = 0; t < TG; ++t) {
        w[t] = wn[t];
        sc[t] = scn[t];
      }
    }
  }
  __syncthreads();  // everyone is done with the x chunk: reuse the LDS

  // red[wave][b][n_local]; lane holds C[b = 4 g + i][n_local = 16 t + r]
  float* red = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int t = 0; t < TG; ++t) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      red[((size_t)wave * 16 + 4 * g + i) * RSTRIDE + 16 * t + r] = acc[t][i];
  }
  __syncthreads();

  for (int o = tid; o < B * GROUP_ROWS; o += 256) {
    const int b = o >> 6, nl = o & (GROUP_ROWS - 1);
    const int n = n0 + nl;
    if (n >= N) continue;
    float s = red[(size_t)b * RSTRIDE + nl];
#pragma unroll
    for (int wv = 1; wv < 4; ++wv) s += red[((size_t)wv * 16 + b) * RSTRIDE + nl];
    if (SPLIT) {
      part[((size_t)blockIdx.y * B + b) * N + n] = s;
    } else {
      y[(size_t)b * N + n] = f32_to_act<DT>(s);
    }
  }
}

// y[b][n] = cast(sum_s part[s][b][n]), s in index order
template <int DT>
__global__ __launch_bounds__(256) void w4_reduce_kernel(
    const float* __restrict__ part, uint16_t* __restrict__ y, int ksplit, long total) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total;
       i += (long)gridDim.x * 256) {
    float s = part[i];
    for (int k = 1; k < ksplit; ++k) s += part[(long)k * total + i];
    y[i] = f32_to_act<DT>(s);
  }
}

// ---------------------------------------------------------------------------
// Dequant
// ---------------------------------------------------------------------------

template <int DT>
__global__ __launch_bounds__(256) void w4_dequant_kernel(
    const u32x4* __restrict__ packed, const float* __restrict__ scale,
    s16x8* __restrict__ w, long total32) {
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < total32;
       v += (long)gridDim.x * 256) {
    // 32-k block v of the row-major (N, K/32) grid lies in group v / 4 of
    // the row-major (N, K/128) scales
    const float sc = scale[v >> 2];
    const u32x4 in = packed[v];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      s16x8 out;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float p = code_to_f32(in[d], i) * sc;
        // keep the product an fp32 multiply of its own: fused into the fp16
        // convert (v_fma_mixlo_f16, + 0) it loses the sign of a zero
        asm volatile("" : "+v"(p));
        out[i] = short(f32_to_act<DT>(p));
      }
      w[4 * v + d] = out;
    }
  }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

struct W4Args {
  int B, N, K;
  bool bf16;
};

// packed (N, K/2) uint8 and scale (N, K/128) fp32 on one GPU -> (N, K)
void check_w4_weight(const char* op, const at::Tensor& packed, const at::Tensor& scale,
                     int64_t kmult) {
  TORCH_CHECK(packed.is_cuda(), op, ": packed must be on the GPU");
  TORCH_CHECK(scale.device() == packed.device(), op, ": scale must be on packed's device");
  TORCH_CHECK(packed.scalar_type() == at::kByte, op, ": packed must be uint8");
  TORCH_CHECK(scale.scalar_type() == at::kFloat, op, ": scale must be float32");
  TORCH_CHECK(packed.dim() == 2 && packed.size(0) >= 1, op,
              ": packed must be (N, K / 2) with N >= 1");
  const int64_t N = packed.size(0), K = 2 * packed.size(1);
  TORCH_CHECK(K >= kmult && K % kmult == 0, op, ": need K % ", kmult, " == 0, got K = ", K);
  TORCH_CHECK(N < (1 << 30) && N * K / 32 < (int64_t(1) << 31), op, ": packed too large");
  TORCH_CHECK(scale.dim() == 2 && scale.size(0) == N && scale.size(1) == K / GROUP, op,
              ": scale must be (N, K / 128)");
  TORCH_CHECK(packed.is_contiguous() && scale.is_contiguous(), op,
              ": packed and scale must be contiguous");
  TORCH_CHECK((uintptr_t)packed.data_ptr() % 16 == 0, op, ": packed must be 16-byte aligned");
}

W4Args check_w4(const char* op, const at::Tensor& x, const at::Tensor& packed,
                const at::Tensor& scale) {
  TORCH_CHECK(x.is_cuda(), op, ": x must be on the GPU");
  TORCH_CHECK(packed.device() == x.device(), op, ": packed and scale must be on x's device");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kHalf, op,
              ": x must be bf16 or fp16");
  check_w4_weight(op, packed, scale, 512);
  const int64_t N = packed.size(0), K = 2 * packed.size(1);
  TORCH_CHECK(x.dim() == 2 && x.size(1) == K, op, ": x must be (B, K = ", K, ")");
  const int64_t B = x.size(0);
  TORCH_CHECK(B >= 1 && B <= 16, op, ": need 1 <= B <= 16, got ", B);
  TORCH_CHECK(x.is_contiguous(), op, ": x must be contiguous");
  TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0, op, ": x must be 16-byte aligned");
  return {int(B), int(N), int(K), x.scalar_type() == at::kBFloat16};
}

// Workgroup K split of the matrix body, from (N, K) alone: enough workgroups
// for TARGET_WGS as long as a workgroup keeps one 512-wide unit, at most
// MAX_KSPLIT ways (the partial buffer and its reduce grow with the split),
// never more than MAX_UNITS units per workgroup (the LDS x chunk), which
// wins over the cap for a very long K. TARGET_WGS is half a workgroup per
// CU, not W8's two: measured at K = 2048, fp16, rows 1..16 (profiles/PERF.md
// "W4A16 decode"), N = 6144 / 8192 (96 / 128 row groups) run 0.3-0.8 us
// faster unsplit or split 2 ways than split 4 ways, since the partial buffer
// and the reduce launch cost more than the idle CUs, and N = 2048 (32 row
// groups) runs 0.4-1.2 us faster split 4 ways than 1 or 2.
constexpr int TARGET_WGS = 128;
constexpr int MAX_KSPLIT = 8;

int pick_ksplit(int N, int K) {
  const int units = K / UNIT;
  const int groups = (N + GROUP_ROWS - 1) / GROUP_ROWS;
  int want = (TARGET_WGS + groups - 1) / groups;
  if (want > MAX_KSPLIT) want = MAX_KSPLIT;
  const int floor_split = (units + MAX_UNITS - 1) / MAX_UNITS;
  if (want < floor_split) want = floor_split;
  if (want > units) want = units;
  return want;
}

template <int DT, int B>
void launch_gemv(const at::Tensor& x, const at::Tensor& packed, const at::Tensor& scale,
                 at::Tensor& y, int N, int K, hipStream_t stream) {
  hipLaunchKernelGGL((w4_gemv_kernel<DT, B>), dim3((N + 3) / 4), dim3(256), 0, stream,
                     (const s16x8*)x.data_ptr(), (const u32x4*)packed.data_ptr(),
                     scale.data_ptr<float>(), (uint16_t*)y.data_ptr(), N, K / 32);
}

template <int DT>
void launch_gemv_b(int B, const at::Tensor& x, const at::Tensor& packed,
                   const at::Tensor& scale, at::Tensor& y, int N, int K,
                   hipStream_t stream) {
  switch (B) {
    case 1: launch_gemv<DT, 1>(x, packed, scale, y, N, K, stream); break;
    case 2: launch_gemv<DT, 2>(x, packed, scale, y, N, K, stream); break;
    case 3: launch_gemv<DT, 3>(x, packed, scale, y, N, K, stream); break;
    default: launch_gemv<DT, 4>(x, packed, scale, y, N, K, stream); break;
  }
}

template <int DT>
void launch_gemm(const W4Args& a, int ksplit, const at::Tensor& x, const at::Tensor& packed,
                 const at::Tensor& scale, at::Tensor& y, hipStream_t stream) {
  const int units = a.K / UNIT;
  const int per = (units + ksplit - 1) / ksplit;
  ksplit = (units + per - 1) / per;  // no empty workgroups
  const size_t xbytes = (size_t)a.B * (per * UNIT + XPAD) * 2;
  const size_t rbytes = (size_t)4 * 16 * RSTRIDE * sizeof(float);
  const size_t lds = xbytes > rbytes ? xbytes : rbytes;
  dim3 grid((a.N + GROUP_ROWS - 1) / GROUP_ROWS, ksplit), block(256);
  const s16x8* xp = (const s16x8*)x.data_ptr();
  const uint8_t* wp = (const uint8_t*)packed.data_ptr();
  const float* sp = scale.data_ptr<float>();
  uint16_t* yp = (uint16_t*)y.data_ptr();
  if (ksplit == 1) {
    hipLaunchKernelGGL((w4_gemm_kernel<DT, false>), grid, block, lds, stream, xp, wp, sp,
                       yp, (float*)nullptr, a.B, a.N, a.K, per);
    return;
  }
  at::Tensor part = at::empty({ksplit, a.B, a.N}, x.options().dtype(at::kFloat));
  hipLaunchKernelGGL((w4_gemm_kernel<DT, true>), grid, block, lds, stream, xp, wp, sp, yp,
                     part.data_ptr<float>(), a.B, a.N, a.K, per);
  const long total = (long)a.B * a.N;
  hipLaunchKernelGGL((w4_reduce_kernel<DT>), dim3(capped_grid(total, 256)), block, 0,
                     stream, part.data_ptr<float>(), yp, ksplit, total);
}

}  // namespace

// Streaming body: 1 <= B <= 4.
at::Tensor w4_gemv(at::Tensor x, at::Tensor packed, at::Tensor scale) {
  const W4Args a = check_w4("w4_gemv", x, packed, scale);
  TORCH_CHECK(a.B <= 4, "w4_gemv: the streaming body takes B <= 4, got ", a.B);
  at::Tensor y = at::empty({a.B, a.N}, x.options());
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  if (a.bf16)
    launch_gemv_b<0>(a.B, x, packed, scale, y, a.N, a.K, stream);
  else
    launch_gemv_b<1>(a.B, x, packed, scale, y, a.N, a.K, stream);
  TORCH_CHECK(hipGetLastError() == hipSuccess, "w4_gemv: kernel launch failed");
  return y;
}

// Matrix body: 1 <= B <= 16. ksplit 0 picks the workgroup K split from
// (N, K); a positive value (benchmarks, tests) is clamped to what the LDS x
// chunk and K / 512 allow.
at::Tensor w4_gemm(at::Tensor x, at::Tensor packed, at::Tensor scale, int64_t ksplit) {
  const W4Args a = check_w4("w4_gemm", x, packed, scale);
  const int units = a.K / UNIT;
  TORCH_CHECK(ksplit >= 0 && ksplit <= units, "w4_gemm: ksplit must be in [0, K / 512]");
  int ks = ksplit == 0 ? pick_ksplit(a.N, a.K) : int(ksplit);
  const int floor_split = (units + MAX_UNITS - 1) / MAX_UNITS;
  if (ks < floor_split) ks = floor_split;
  at::Tensor y = at::empty({a.B, a.N}, x.options());
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  if (a.bf16)
    launch_gemm<0>(a, ks, x, packed, scale, y, stream);
  else
    launch_gemm<1>(a, ks, x, packed, scale, y, stream);
  TORCH_CHECK(hipGetLastError() == hipSuccess, "w4_gemm: kernel launch failed");
  return y;
}

// (packed, scale) -> (N, K) bf16 (`bf16`) or fp16; K % 128 == 0.
at::Tensor dequant_w4(at::Tensor packed, at::Tensor scale, bool bf16) {
  check_w4_weight("dequant_w4", packed, scale, GROUP);
  const int64_t N = packed.size(0), K = 2 * packed.size(1);
  at::Tensor w = at::empty({N, K}, packed.options().dtype(bf16 ? at::kBFloat16 : at::kHalf));
  const long total32 = N * K / 32;
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  dim3 grid(capped_grid(total32, 256, 4096)), block(256);
  if (bf16)
    hipLaunchKernelGGL((w4_dequant_kernel<0>), grid, block, 0, stream,
                       (const u32x4*)packed.data_ptr(), scale.data_ptr<float>(),
                       (s16x8*)w.data_ptr(), total32);
  else
    hipLaunchKernelGGL((w4_dequant_kernel<1>), grid, block, 0, stream,
                       (const u32x4*)packed.data_ptr(), scale.data_ptr<float>(),
                       (s16x8*)w.data_ptr(), total32);
  TORCH_CHECK(hipGetLastError() == hipSuccess, "dequant_w4: kernel launch failed");
  return w;
}
