// Weight-only int8 ("W8A16") decode projections for gfx950.
//
//   y (B, N) = x (B, K) @ (q (N, K) * scale (N,)[:, None])^T
//
// x, y: bf16 or fp16; q: int8 row-major (plain signed, -127..127); scale:
// fp32 per output row. Every kernel accumulates the integer-weight products
// in fp32, multiplies the finished sum by scale[n] once and rounds once to
// the output type, so the result is defined by (q, scale, x) alone. The
// weight stream is half the bytes of ops/csrc/gemv.hip's.
//
// 1 <= B <= 16, K % 512 == 0, any N >= 1. Nothing is read on the host, no
// float atomics (same bits on every call), any workspace comes from torch's
// allocator at a size fixed by the shapes: every launch is graph-capturable.
//
// Two bodies, because the two regimes have different limits:
//
// * w8_gemv_kernel (B <= 4): gemv.hip's mapping, one wave per output row,
//   four rows per 256-thread workgroup. A lane's 16-byte load holds 16
//   weights, a wave step covers 1024 k; with K % 1024 == 512 the last step
//   runs with the upper half-wave inactive. Bytes go to fp32 in registers
//   (one sign-extending convert each), multiply the rows' x fragments in
//   fp32, 64-lane butterfly, scale, cast, store.
//
// * w8_gemm_kernel (any B, meant for 3..16): v_mfma_f32_16x16x32_{f16,bf16}.
//   A 16-row tile of W is the A operand (row = lane & 15), x^T the B operand
//   (column b = lane & 15; b >= B are zero fragments, never loaded), the
//   16x16 fp32 result is (n, b). The k order inside an MFMA is free as long
//   as both operands agree: lane (row r, group g = lane >> 4) takes ONE
//   16-byte load of q[r][k0 + 16 g .. + 16) and feeds two MFMAs from it
//   (bytes 0..7, then 8..15); the x fragments of lane (b, g) are the same 16
//   k of row b, in the same two halves. int8 -> fp16 / bf16 is exact.
//
//   Work split. A workgroup (4 waves) owns 64 rows (4 tiles) x one K chunk
//   of `per` 512-wide units. Its x chunk (B x chunk, <= 33 KB) is staged to
//   LDS once with coalesced 16-byte loads and shared by the four tiles. The
//   four waves split the chunk's 64-k steps round robin (wave w takes steps
//   w, w + 4, ...: K is split across waves from the smallest K, 512, on), so
//   the workgroup reads 256 contiguous bytes of each row per round; a wave
//   keeps all four tiles' accumulators (16 VGPRs) and issues the four tiles'
//   loads together, which is the memory-level parallelism of the kernel.
//   The waves' partial tiles are summed through LDS in wave order. Across
//   workgroups K is split `ksplit` ways (grid.y, from K = 1024 on) when
//   N / 64 row groups alone would leave CUs idle: then each workgroup writes
//   its fp32 partial to a (ksplit, B, N) workspace and w8_reduce_kernel sums
//   the splits in index order, scales and casts. ksplit depends on (N, K)
//   only: see pick_ksplit.
//
// w8_dequant_kernel: (q, scale) -> 16-bit (N, K) in one pass, 16 bytes in and
// 32 bytes out per lane, bits equal to ops.reference.dequantize_rows_w8
// (one fp32 product, one rounding). The many-row (prefill) path calls it
// with the power-of-two part of each scale, which keeps q * 2^e exact, feeds
// that to the GEMM library and applies the remaining factor in [1, 2) to the
// result's columns in fp32 (ops.linear_w8): rounding q * scale to 16 bits
// would cost the product 3x (fp16) to 25x (bf16) the parity bound.

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

ZTA_DEV float byte_to_f32(uint32_t word, int i) {
  return float(int(int8_t(word >> (8 * i))));
}

// ---------------------------------------------------------------------------
// Streaming body
// ---------------------------------------------------------------------------

template <int DT, int B>
__global__ __launch_bounds__(256) void w8_gemv_kernel(
    const s16x8* __restrict__ x,    // (B, K/8)
    const u32x4* __restrict__ q,    // (N, K/16)
    const float* __restrict__ scale,
    uint16_t* __restrict__ y,       // (B, N)
    int N, int K16) {
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + wave;
  if (n >= N) return;

  float acc[B];
#pragma unroll
  for (int b = 0; b < B; ++b) acc[b] = 0.0f;

  const u32x4* qr = q + (size_t)n * K16;
  // K16 % 64 is 0 or 32: in the last step of the latter the upper half-wave
  // fails this test and idles
  for (int k16 = lane; k16 < K16; k16 += 64) {
    const u32x4 w = qr[k16];
    float wf[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) wf[i] = byte_to_f32(w[i >> 2], i & 3);
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const s16x8* xb = x + (size_t)b * (2 * K16) + 2 * k16;
      const s16x8 x0 = xb[0], x1 = xb[1];
      float s = 0.0f;
#pragma unroll
      for (int i = 0; i < 8; ++i) s += wf[i] * act_to_f32<DT>(uint16_t(x0[i]));
#pragma unroll
      for (int i = 0; i < 8; ++i) s += wf[8 + i] * act_to_f32<DT>(uint16_t(x1[i]));
      acc[b] += s;
    }
  }
  const float sc = scale[n];
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const float r = wave_reduce_sum(acc[b]);
    if (lane == 0) y[(size_t)b * N + n] = f32_to_act<DT>(r * sc);
  }
}

// ---------------------------------------------------------------------------
// Matrix body
// ---------------------------------------------------------------------------

constexpr int TG = 4;            // 16-row tiles per workgroup (and per wave)
constexpr int GROUP_ROWS = 16 * TG;
constexpr int UNIT = 512;        // K granule of the split across workgroups
constexpr int MAX_UNITS = 2;     // per workgroup: x chunk <= 16 x 1024 x 2 B
constexpr int XPAD = 8;          // 16-bit elements of padding per LDS x row
constexpr int RSTRIDE = GROUP_ROWS + 4;  // floats per b row of a partial tile

// 8 int8 (two dwords' worth: `lo` bytes 0..3, `hi` bytes 0..3) -> fragment
ZTA_DEV h16x8 bytes_to_f16x8(uint32_t lo, uint32_t hi) {
  // u = q + 128 as an unsigned byte; 0x6400 | u is the fp16 1024 + u, and
  // (1024 + u) - 1152 = q exactly. v_perm_b32 builds two such halves a time.
  const h16x2 bias = {_Float16(1152.0f), _Float16(1152.0f)};
  h16x8 out;
  const uint32_t w[2] = {lo ^ 0x80808080u, hi ^ 0x80808080u};
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const uint32_t p0 = __builtin_amdgcn_perm(0x64646464u, w[d], 0x04010400u);
    const uint32_t p1 = __builtin_amdgcn_perm(0x64646464u, w[d], 0x04030402u);
    const h16x2 a = __builtin_bit_cast(h16x2, p0) - bias;
    const h16x2 b = __builtin_bit_cast(h16x2, p1) - bias;
    out[4 * d + 0] = a[0];
    out[4 * d + 1] = a[1];
    out[4 * d + 2] = b[0];
    out[4 * d + 3] = b[1];
  }
  return out;
}

ZTA_DEV b16x8 bytes_to_bf16x8(uint32_t lo, uint32_t hi) {
  // |q| <= 127 has 7 significant bits: the upper half of its fp32 is exact
  s16x8 out;
  const uint32_t w[2] = {lo, hi};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float f = byte_to_f32(w[i >> 2], i & 3);
    out[i] = short(__builtin_bit_cast(uint32_t, f) >> 16);
  }
  return __builtin_bit_cast(b16x8, out);
}

template <int DT>
ZTA_DEV f32x4 mfma_w8(uint32_t lo, uint32_t hi, s16x8 xf, f32x4 c) {
  if (DT == 1) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(
        bytes_to_f16x8(lo, hi), __builtin_bit_cast(h16x8, xf), c, 0, 0, 0);
  } else {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(
        bytes_to_bf16x8(lo, hi), __builtin_bit_cast(b16x8, xf), c, 0, 0, 0);
  }
}

// grid (ceil(N / 64), ksplit); dynamic LDS = max(B * (per*512 + XPAD) * 2,
// 4 * 16 * RSTRIDE * 4) bytes. SPLIT: write fp32 partials to `part`
// (ksplit, B, N) instead of y.
template <int DT, bool SPLIT>
__global__ __launch_bounds__(256) void w8_gemm_kernel(
    const s16x8* __restrict__ x,    // (B, K/8)
    const int8_t* __restrict__ q,   // (N, K)
    const float* __restrict__ scale,
    uint16_t* __restrict__ y,       // (B, N)
    float* __restrict__ part,       // (ksplit, B, N)
    int B, int N, int K, int per) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int r = lane & 15;  // W row of the tile / x row b
  const int g = lane >> 4;  // k group
  const int n0 = blockIdx.x * GROUP_ROWS;
  const int k0 = blockIdx.y * per * UNIT;
  const int klen = min(per * UNIT, K - k0);  // a multiple of 512, > 0
  const int xstride = klen + XPAD;           // 16-bit elements

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
  const int8_t* qrow[TG];
#pragma unroll
  for (int t = 0; t < TG; ++t) {
    acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    // rows past N re-read row N - 1; their results are never stored
    const int n = min(n0 + 16 * t + r, N - 1);
    qrow[t] = q + (size_t)n * K + k0 + 16 * g;
  }
  const char* xrow = smem + ((size_t)r * xstride + 16 * g) * 2;
  const bool live = r < B;

  // klen / 64 steps is a multiple of 8: every wave gets the same even count
  for (int kk = wave * 64; kk < klen; kk += 256) {
    u32x4 w[TG];
#pragma unroll
    for (int t = 0; t < TG; ++t) w[t] = *reinterpret_cast<const u32x4*>(qrow[t] + kk);
    s16x8 xa = s16x8{}, xb = s16x8{};
    if (live) {
      xa = *reinterpret_cast<const s16x8*>(xrow + 2 * kk);
      xb = *reinterpret_cast<const s16x8*>(xrow + 2 * kk + 16);
    }
#pragma unroll
    for (int t = 0; t < TG; ++t) {
      acc[t] = mfma_w8<DT>(w[t][0], w[t][1], xa, acc[t]);
      acc[t] = mfma_w8<DT>(w[t][2], w[t][3], xb, acc[t]);
    }
  }
  __syncthreads();  // everyone is done with the x chunk: reuse the LDS

  // red[wave][b][n_local]; lane holds C[n_local = 16 t + 4 g + i][b = r]
  float* red = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int t = 0; t < TG; ++t) {
    *reinterpret_cast<f32x4*>(red + ((size_t)wave * 16 + r) * RSTRIDE + 16 * t + 4 * g) =
        acc[t];
  }
  __syncthreads();

  for (int o = tid; o < B * GROUP_ROWS; o += 256) {
    const int b = o >> 6, nl = o & (GROUP_ROWS - 1);
    const int n = n0 + nl;
    if (n >= N) continue;
    float s = red[(size_t)b * RSTRIDE + nl];
#pragma unroll
    for (int w = 1; w < 4; ++w) s += red[((size_t)w * 16 + b) * RSTRIDE + nl];
    if (SPLIT) {
      part[((size_t)blockIdx.y * B + b) * N + n] = s;
    } else {
      y[(size_t)b * N + n] = f32_to_act<DT>(s * scale[n]);
    }
  }
}

// y[b][n] = cast(scale[n] * sum_s part[s][b][n]), s in index order
template <int DT>
__global__ __launch_bounds__(256) void w8_reduce_kernel(
    const float* __restrict__ part, const float* __restrict__ scale,
    uint16_t* __restrict__ y, int ksplit, int B, int N) {
  const long total = (long)B * N;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total;
       i += (long)gridDim.x * 256) {
    float s = part[i];
    for (int k = 1; k < ksplit; ++k) s += part[(long)k * total + i];
    y[i] = f32_to_act<DT>(s * scale[i % N]);
  }
}

// ---------------------------------------------------------------------------
// Dequant
// ---------------------------------------------------------------------------

template <int DT>
__global__ __launch_bounds__(256) void w8_dequant_kernel(
    const u32x4* __restrict__ q, const float* __restrict__ scale,
    s16x8* __restrict__ w, long total16, int K16) {
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < total16;
       v += (long)gridDim.x * 256) {
    const float sc = scale[v / K16];
    const u32x4 in = q[v];
    s16x8 out[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float p = byte_to_f32(in[i >> 2], i & 3) * sc;
      // keep the product an fp32 multiply of its own: fused into the fp16
      // convert (v_fma_mixlo_f16, + 0) it loses the sign of a zero
      asm volatile("" : "+v"(p));
      out[i >> 3][i & 7] = short(f32_to_act<DT>(p));
    }
    w[2 * v] = out[0];
    w[2 * v + 1] = out[1];
  }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

struct W8Args {
  int B, N, K;
  bool bf16;
};

W8Args check_w8(const char* op, const at::Tensor& x, const at::Tensor& q,
                const at::Tensor& scale) {
  TORCH_CHECK(x.is_cuda(), op, ": x must be on the GPU");
  TORCH_CHECK(q.device() == x.device() && scale.device() == x.device(), op,
              ": q and scale must be on x's device");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kHalf, op,
              ": x must be bf16 or fp16");
  TORCH_CHECK(q.scalar_type() == at::kChar, op, ": q must be int8");
  TORCH_CHECK(scale.scalar_type() == at::kFloat, op, ": scale must be float32");
  TORCH_CHECK(q.dim() == 2 && q.size(0) >= 1, op, ": q must be (N, K) with N >= 1");
  const int64_t N = q.size(0), K = q.size(1);
  TORCH_CHECK(K >= 512 && K % 512 == 0, op, ": need K % 512 == 0, got K = ", K);
  TORCH_CHECK(N < (1 << 30) && N * K / 16 < (int64_t(1) << 31), op, ": q too large");
  TORCH_CHECK(scale.dim() == 1 && scale.size(0) == N, op, ": scale must be (N,)");
  TORCH_CHECK(x.dim() == 2 && x.size(1) == K, op, ": x must be (B, K = ", K, ")");
  const int64_t B = x.size(0);
  TORCH_CHECK(B >= 1 && B <= 16, op, ": need 1 <= B <= 16, got ", B);
  TORCH_CHECK(x.is_contiguous() && q.is_contiguous() && scale.is_contiguous(), op,
              ": x, q and scale must be contiguous");
  TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0 && (uintptr_t)q.data_ptr() % 16 == 0,
              op, ": x and q must be 16-byte aligned");
  return {int(B), int(N), int(K), x.scalar_type() == at::kBFloat16};
}

// Workgroup K split of the matrix body, from (N, K) alone. Aim for >= 512
// workgroups (two per CU) as long as a workgroup keeps one 512-wide unit,
// but split at most MAX_KSPLIT ways: the partial buffer and its reduce grow
// with the split (measured at N = 2048, K = 8192: 16 ways 10.3-12.2 us, 8 ways
// 8.5-10.5 us; profiles/PERF.md). Never more than MAX_UNITS units per
// workgroup (the LDS x chunk), which wins over the cap for a very long K.
constexpr int MAX_KSPLIT = 8;

int pick_ksplit(int N, int K) {
  const int units = K / UNIT;
  const int groups = (N + GROUP_ROWS - 1) / GROUP_ROWS;
  int want = (512 + groups - 1) / groups;
  if (want > MAX_KSPLIT) want = MAX_KSPLIT;
  const int floor_split = (units + MAX_UNITS - 1) / MAX_UNITS;
  if (want < floor_split) want = floor_split;
  if (want > units) want = units;
  return want;
}

template <int DT, int B>
void launch_gemv(const at::Tensor& x, const at::Tensor& q, const at::Tensor& scale,
                 at::Tensor& y, int N, int K, hipStream_t stream) {
  hipLaunchKernelGGL((w8_gemv_kernel<DT, B>), dim3((N + 3) / 4), dim3(256), 0, stream,
                     (const s16x8*)x.data_ptr(), (const u32x4*)q.data_ptr(),
                     scale.data_ptr<float>(), (uint16_t*)y.data_ptr(), N, K / 16);
}

template <int DT>
void launch_gemv_b(int B, const at::Tensor& x, const at::Tensor& q,
                   const at::Tensor& scale, at::Tensor& y, int N, int K,
                   hipStream_t stream) {
  switch (B) {
    case 1: launch_gemv<DT, 1>(x, q, scale, y, N, K, stream); break;
    case 2: launch_gemv<DT, 2>(x, q, scale, y, N, K, stream); break;
    case 3: launch_gemv<DT, 3>(x, q, scale, y, N, K, stream); break;
    default: launch_gemv<DT, 4>(x, q, scale, y, N, K, stream); break;
  }
}

template <int DT>
void launch_gemm(const W8Args& a, int ksplit, const at::Tensor& x, const at::Tensor& q,
                 const at::Tensor& scale, at::Tensor& y, hipStream_t stream) {
  const int units = a.K / UNIT;
  const int per = (units + ksplit - 1) / ksplit;
  ksplit = (units + per - 1) / per;  // no empty workgroups
  const size_t xbytes = (size_t)a.B * (per * UNIT + XPAD) * 2;
  const size_t rbytes = (size_t)4 * 16 * RSTRIDE * sizeof(float);
  const size_t lds = xbytes > rbytes ? xbytes : rbytes;
  dim3 grid((a.N + GROUP_ROWS - 1) / GROUP_ROWS, ksplit), block(256);
  const s16x8* xp = (const s16x8*)x.data_ptr();
  const int8_t* qp = (const int8_t*)q.data_ptr();
  const float* sp = scale.data_ptr<float>();
  uint16_t* yp = (uint16_t*)y.data_ptr();
  if (ksplit == 1) {
    hipLaunchKernelGGL((w8_gemm_kernel<DT, false>), grid, block, lds, stream, xp, qp, sp,
                       yp, (float*)nullptr, a.B, a.N, a.K, per);
    return;
  }
  at::Tensor part = at::empty({ksplit, a.B, a.N}, x.options().dtype(at::kFloat));
  hipLaunchKernelGGL((w8_gemm_kernel<DT, true>), grid, block, lds, stream, xp, qp, sp, yp,
                     part.data_ptr<float>(), a.B, a.N, a.K, per);
  hipLaunchKernelGGL((w8_reduce_kernel<DT>),
                     dim3(capped_grid((long)a.B * a.N, 256)), block, 0, stream,
                     part.data_ptr<float>(), sp, yp, ksplit, a.B, a.N);
}

}  // namespace

// Streaming body: 1 <= B <= 4.
at::Tensor w8_gemv(at::Tensor x, at::Tensor q, at::Tensor scale) {
  const W8Args a = check_w8("w8_gemv", x, q, scale);
  TORCH_CHECK(a.B <= 4, "w8_gemv: the streaming body takes B <= 4, got ", a.B);
  at::Tensor y = at::empty({a.B, a.N}, x.options());
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  if (a.bf16)
    launch_gemv_b<0>(a.B, x, q, scale, y, a.N, a.K, stream);
  else
    launch_gemv_b<1>(a.B, x, q, scale, y, a.N, a.K, stream);
  TORCH_CHECK(hipGetLastError() == hipSuccess, "w8_gemv: kernel launch failed");
  return y;
}

// Matrix body: 1 <= B <= 16. ksplit 0 picks the workgroup K split from
// (N, K); a positive value (benchmarks, tests) is clamped to what the LDS x
// chunk and K / 512 allow.
at::Tensor w8_gemm(at::Tensor x, at::Tensor q, at::Tensor scale, int64_t ksplit) {
  const W8Args a = check_w8("w8_gemm", x, q, scale);
  const int units = a.K / UNIT;
  TORCH_CHECK(ksplit >= 0 && ksplit <= units, "w8_gemm: ksplit must be in [0, K / 512]");
  int ks = ksplit == 0 ? pick_ksplit(a.N, a.K) : int(ksplit);
  const int floor_split = (units + MAX_UNITS - 1) / MAX_UNITS;
  if (ks < floor_split) ks = floor_split;
  at::Tensor y = at::empty({a.B, a.N}, x.options());
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  if (a.bf16)
    launch_gemm<0>(a, ks, x, q, scale, y, stream);
  else
    launch_gemm<1>(a, ks, x, q, scale, y, stream);
  TORCH_CHECK(hipGetLastError() == hipSuccess, "w8_gemm: kernel launch failed");
  return y;
}

// (q, scale) -> (N, K) bf16 (`bf16`) or fp16; K % 16 == 0.
at::Tensor dequant_w8(at::Tensor q, at::Tensor scale, bool bf16) {
  const at::ScalarType dtype = bf16 ? at::kBFloat16 : at::kHalf;
  TORCH_CHECK(q.is_cuda() && scale.device() == q.device(),
              "dequant_w8: q and scale must be on the same GPU");
  TORCH_CHECK(q.scalar_type() == at::kChar && scale.scalar_type() == at::kFloat,
              "dequant_w8: q must be int8 and scale float32");
  TORCH_CHECK(q.dim() == 2 && q.size(0) >= 1 && q.size(1) >= 16 && q.size(1) % 16 == 0,
              "dequant_w8: q must be (N, K) with K % 16 == 0");
  TORCH_CHECK(scale.dim() == 1 && scale.size(0) == q.size(0), "dequant_w8: scale must be (N,)");
  TORCH_CHECK(q.is_contiguous() && scale.is_contiguous(), "dequant_w8: q and scale must be contiguous");
  TORCH_CHECK((uintptr_t)q.data_ptr() % 16 == 0, "dequant_w8: q must be 16-byte aligned");
  const int64_t N = q.size(0), K = q.size(1);
  TORCH_CHECK(K / 16 < (int64_t(1) << 31), "dequant_w8: K too large");
  at::Tensor w = at::empty({N, K}, q.options().dtype(dtype));
  const long total16 = N * K / 16;
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  dim3 grid(capped_grid(total16, 256, 4096)), block(256);
  if (bf16)
    hipLaunchKernelGGL((w8_dequant_kernel<0>), grid, block, 0, stream,
                       (const u32x4*)q.data_ptr(), scale.data_ptr<float>(),
                       (s16x8*)w.data_ptr(), total16, int(K / 16));
  else
    hipLaunchKernelGGL((w8_dequant_kernel<1>), grid, block, 0, stream,
                       (const u32x4*)q.data_ptr(), scale.data_ptr<float>(),
                       (s16x8*)w.data_ptr(), total16, int(K / 16));
  TORCH_CHECK(hipGetLastError() == hipSuccess, "dequant_w8: kernel launch failed");
  return w;
}
