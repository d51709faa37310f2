// Fused-dequant skinny GEMM for quantized weights and 17..64 activation rows
// (gfx950): the rows between decode and prefill, where ops/csrc/gemv_w8.hip
// and gemv_w4.hip (<= 16 rows) stop and dequantizing the whole weight for the
// GEMM library costs four to eight times the bytes the weight holds.
//
//   FMT 8:  y (B, N) = scale[n] * (x (B, K) @ q (N, K)^T)        (gemv_w8.hip)
//   FMT 4:  y (B, N) = x (B, K) @ W^T,
//           W[n][k] = round_to_x_dtype((u[n][k] - 8) * scale[n][k / 128])
//
// x, y: bf16 or fp16. 1 <= B <= 64, K % 512 == 0, any N >= 1. fp32
// accumulation, one rounding to the output type, no float atomics (same bits
// on every call), nothing read on the host, the only workspace comes from
// torch's allocator at a size fixed by the shapes: graph-capturable.
//
// Numerics. W8: the int8 codes are exact in fp16 / bf16 and go to the MFMA as
// they are; the row scale multiplies the finished fp32 sum, as in the <= 16
// row bodies. W4: ops.linear_w4 defines the many-row result as the GEMM over
// the weight rounded ONCE to x's dtype (reference.dequantize_rows_w4), so the
// fragment is made exactly as w4_dequant_kernel makes it (code -> fp32, times
// the group's fp32 scale as a multiply of its own, one convert) and only the
// summation order differs from the library route.
//
// One kernel, wq_rows_kernel<FMT, DT, RT>, RT = ceil(B / 16) row tiles:
//
// * MFMA orientation: v_mfma_f32_16x16x32_{f16,bf16}, x the A operand (row b
//   = 16 rt + (lane & 15)), a 16-row tile of W the B operand (column n = lane
//   & 15); the lane holds C[b = 16 rt + 4 g + i][n], g = lane >> 4. Rows b >=
//   B of the last tile are zero fragments that are never loaded or stored.
//   A step is 128 k = four MFMA k slices. W4: lane (r, g) takes ONE 16-byte
//   load, the 32 codes k + 32 g .. + 32 of ONE scale group; dword j feeds
//   slice j, whose x fragment is x[b][k + 32 g + 8 j .. + 8). W8: two 16-byte
//   loads L = 0, 1 of q[r][k + 64 L + 16 g .. + 16); bytes 8 h .. 8 h + 8 feed
//   slice 2 L + h, x fragment x[b][k + 64 L + 16 g + 8 h .. + 8).
// * Every weight fragment is decoded once per step and reused by all RT row
//   tiles: the conversion that limits the <= 16-row W4 body is spread over
//   up to four MFMAs.
// * Work split: a workgroup (4 waves) owns 128 rows of W x one K chunk of
//   `per` 512-wide units; a wave owns two 16-row tiles (32 rows) over the
//   whole chunk, so no partial tiles are summed across waves and a wave's x
//   fragment from LDS feeds two MFMAs. 128 rows rather than 64 halve the x
//   bytes staged per weight byte (at 64 rows x is 128 B per k against 64 /
//   128 B of W4 / W8 weights).
// * x is staged to LDS in pieces of 256 k (coalesced 16-byte loads, rows
//   padded by 16 bytes), not the whole 512-unit: 64 rows x 264 x 2 B = 33 KB,
//   so that four workgroups share a CU's 160 KB where a 512-k piece (66 KB)
//   would leave two; the registers allow 2-4 waves per SIMD (profiles/PERF.md
//   "Quantized rows 17-64" has the table). The piece is restaged between two
//   barriers, and that wait is exposed: the grids of the 1.3B shapes are a
//   workgroup per CU or less, so no other workgroup covers it (open, same
//   section).
// * The weight and scale loads of step s + 1 are issued before the decode
//   and the MFMAs of step s, those of step 0 before the first piece is
//   staged. Three steps in flight (a ring of four in registers) measured no
//   faster.
// * Split-K across workgroups (grid.y) where N / 128 row groups leave CUs
//   idle: fp32 partials go to a (ksplit, B, N) workspace and
//   wq_rows_reduce_kernel sums the splits in index order (W8: times scale[n])
//   and rounds. ksplit depends on (N, K) only: see pick_ksplit.

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
typedef __attribute__((ext_vector_type(2))) __bf16 b16x2;

constexpr int GROUP = 128;     // k per W4 scale, and per step of either format
constexpr int TPW = 2;         // 16-row W tiles per wave
constexpr int WG_ROWS = 4 * 16 * TPW;  // W rows per workgroup
constexpr int UNIT = 512;      // K granule of the split across workgroups
constexpr int PIECE = 256;     // k of x staged to LDS at a time
constexpr int XPAD = 8;        // 16-bit elements of padding per LDS x row
constexpr int XSTRIDE = PIECE + XPAD;
constexpr int MAX_ROWS = 64;

// DT 0 = bf16, 1 = fp16
template <int DT>
ZTA_DEV uint16_t f32_to_act(float v) {
  if (DT == 0) return f32_to_bf16(v);
  return __builtin_bit_cast(uint16_t, _Float16(v));  // RNE
}

// ---------------------------------------------------------------------------
// Weight fragments: 8 consecutive k of one W row as an MFMA B operand
// ---------------------------------------------------------------------------

// W8 (as ops/csrc/gemv_w8.hip): u = q + 128 as an unsigned byte; 0x6400 | u
// is the fp16 1024 + u, and (1024 + u) - 1152 = q exactly
ZTA_DEV s16x8 w8_frag_f16(uint32_t lo, uint32_t hi) {
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
  return __builtin_bit_cast(s16x8, out);
}

// |q| <= 127 has 7 significant bits: the upper half of its fp32 is exact
ZTA_DEV s16x8 w8_frag_bf16(uint32_t lo, uint32_t hi) {
  s16x8 out;
  const uint32_t w[2] = {lo, hi};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float f = float(int(int8_t(w[i >> 2] >> (8 * (i & 3)))));
    out[i] = short(__builtin_bit_cast(uint32_t, f) >> 16);
  }
  return out;
}

// W4: the 8 codes of dword `dw` (nibble order of reference.quantize_rows_w4:
// nibble j holds k = [0, 2, 4, 6, 1, 3, 5, 7][j]) times `sc`, in k order, with
// the bits of w4_dequant_kernel
template <int DT>
ZTA_DEV s16x8 w4_frag(uint32_t dw, float sc) {
  float p[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t m = ((i & 2) ? (dw >> 4) : dw) & 0x0F0F0F0Fu;
    const int byte = 2 * (i & 1) + (i >> 2);
    p[i] = (float((m >> (8 * byte)) & 0xFFu) - 8.0f) * sc;
    // keep the product an fp32 multiply of its own: fused into the fp16
    // convert (v_fma_mixlo_f16, + 0) it loses the sign of a zero
    asm volatile("" : "+v"(p[i]));
  }
  if (DT == 0) {
    // v_cvt_pk_bf16_f32: round to nearest even like f32_to_bf16, two per op
    // where the integer version costs six ops each (a NaN, which only a
    // non-finite scale makes, comes out as the canonical quiet NaN)
    u32x4 out;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      out[i] = __builtin_bit_cast(
          uint32_t, __builtin_convertvector(f32x2{p[2 * i], p[2 * i + 1]}, b16x2));
    return __builtin_bit_cast(s16x8, out);
  }
  s16x8 out;
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = short(f32_to_act<1>(p[i]));
  return out;
}

template <int DT>
ZTA_DEV f32x4 mfma(s16x8 xf, s16x8 wf, f32x4 c) {
  if (DT == 1) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(
        __builtin_bit_cast(h16x8, xf), __builtin_bit_cast(h16x8, wf), c, 0, 0, 0);
  } else {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(
        __builtin_bit_cast(b16x8, xf), __builtin_bit_cast(b16x8, wf), c, 0, 0, 0);
  }
}

// ---------------------------------------------------------------------------
// The kernel
// ---------------------------------------------------------------------------

// grid (ceil(N / 128), ksplit); dynamic LDS = B * XSTRIDE * 2 bytes. `part`
// not null: write fp32 partials to part (ksplit, B, N) instead of y.
template <int FMT, int DT, int RT>
__global__ __launch_bounds__(256) void wq_rows_kernel(
    const s16x8* __restrict__ x,     // (B, K/8)
    const uint8_t* __restrict__ wq,  // W8: int8 (N, K); W4: packed (N, K/2)
    const float* __restrict__ scale, // W8: (N,); W4: (N, K/128)
    uint16_t* __restrict__ y,        // (B, N)
    float* __restrict__ part,        // (ksplit, B, N) or null
    int B, int N, int K, int per) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NLD = FMT == 8 ? 2 : 1;           // 16-byte loads per tile and step
  constexpr int STEP_BYTES = FMT == 8 ? GROUP : GROUP / 2;
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int r = lane & 15;  // W row of the tile / x row of the row tile
  const int g = lane >> 4;  // k group
  const int n0 = blockIdx.x * WG_ROWS + wave * (16 * TPW);
  const int k0 = blockIdx.y * per * UNIT;
  const int klen = min(per * UNIT, K - k0);  // a multiple of 512, > 0
  const int steps = klen / GROUP;

  const uint8_t* wrow[TPW];
  const float* srow[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    // rows past N re-read row N - 1; their results are never stored
    const size_t n = min(n0 + 16 * t + r, N - 1);
    if (FMT == 8) {
      wrow[t] = wq + n * K + k0 + 16 * g;
      srow[t] = scale;
    } else {
      wrow[t] = wq + (n * K + k0 + 32 * g) / 2;
      srow[t] = scale + n * (K / GROUP) + k0 / GROUP;
    }
  }
  u32x4 w[TPW][NLD];
  float sc[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
#pragma unroll
    for (int l = 0; l < NLD; ++l)
      w[t][l] = *reinterpret_cast<const u32x4*>(wrow[t] + 64 * l);
    sc[t] = FMT == 4 ? srow[t][0] : 0.0f;
  }

  f32x4 acc[TPW][RT];
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[t][rt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  const int K8 = K >> 3;
  for (int p = 0; p < klen / PIECE; ++p) {
    if (p) __syncthreads();  // everyone is done with the previous piece
    // stage x[:, k0 + 256 p .. + 256): 32 vectors per row
    for (int v = tid; v < B * (PIECE / 8); v += 256) {
      const int b = v >> 5, c = v & 31;
      *reinterpret_cast<s16x8*>(smem + ((size_t)b * XSTRIDE + 8 * c) * 2) =
          x[(size_t)b * K8 + ((k0 + PIECE * p) >> 3) + c];
    }
    __syncthreads();

#pragma unroll
    for (int ss = 0; ss < PIECE / GROUP; ++ss) {
      const int s = p * (PIECE / GROUP) + ss;
      u32x4 wn[TPW][NLD];
      float scn[TPW];
      if (s + 1 < steps) {
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
#pragma unroll
          for (int l = 0; l < NLD; ++l)
            wn[t][l] = *reinterpret_cast<const u32x4*>(
                wrow[t] + (size_t)(s + 1) * STEP_BYTES + 64 * l);
          scn[t] = FMT == 4 ? srow[t][s + 1] : 0.0f;
        }
      }
      // decode once, for every row tile
      s16x8 wf[TPW][4];
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if constexpr (FMT == 4) {
            wf[t][j] = w4_frag<DT>(w[t][0][j], sc[t]);
          } else {
            const u32x4 q = w[t][j >> 1];
            wf[t][j] = DT == 1 ? w8_frag_f16(q[2 * (j & 1)], q[2 * (j & 1) + 1])
                               : w8_frag_bf16(q[2 * (j & 1)], q[2 * (j & 1) + 1]);
          }
        }
      }
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        s16x8 xf[4] = {s16x8{}, s16x8{}, s16x8{}, s16x8{}};
        if (16 * rt + r < B) {
          const char* xrow = smem + ((size_t)(16 * rt + r) * XSTRIDE + ss * GROUP) * 2;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int koff = FMT == 4 ? 32 * g + 8 * j : 64 * (j >> 1) + 16 * g + 8 * (j & 1);
            xf[j] = *reinterpret_cast<const s16x8*>(xrow + 2 * koff);
          }
        }
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[t][rt] = mfma<DT>(xf[j], wf[t][j], acc[t][rt]);
        }
      }
      if (s + 1 < steps) {
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
#pragma unroll
          for (int l = 0; l < NLD; ++l) w[t][l] = wn[t][l];
          sc[t] = scn[t];
        }
      }
    }
  }

  // lane holds C[b = 16 rt + 4 g + i][n = n0 + 16 t + r]
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int n = n0 + 16 * t + r;
    if (n >= N) continue;
    const float rs = (FMT == 8 && part == nullptr) ? scale[n] : 1.0f;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int b = 16 * rt + 4 * g + i;
        if (b >= B) continue;
        if (part != nullptr) {
          part[((size_t)blockIdx.y * B + b) * N + n] = acc[t][rt][i];
        } else {
          y[(size_t)b * N + n] =
              f32_to_act<DT>(FMT == 8 ? acc[t][rt][i] * rs : acc[t][rt][i]);
        }
      }
    }
  }
}

// y[b][n] = cast(sum_s part[s][b][n] (* scale[n])), s in index order
template <int FMT, int DT>
__global__ __launch_bounds__(256) void wq_rows_reduce_kernel(
    const float* __restrict__ part, const float* __restrict__ scale,
    uint16_t* __restrict__ y, int ksplit, int N, long total) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total;
       i += (long)gridDim.x * 256) {
    float s = part[i];
    for (int k = 1; k < ksplit; ++k) s += part[(long)k * total + i];
    y[i] = f32_to_act<DT>(FMT == 8 ? s * scale[i % N] : s);
  }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

struct RowsArgs {
  int B, N, K;
  bool bf16;
};

// wq: int8 (N, K) with scale (N,), or uint8 (N, K / 2) with scale (N, K / 128)
template <int FMT>
RowsArgs check_rows(const char* op, const at::Tensor& x, const at::Tensor& wq,
                    const at::Tensor& scale) {
  TORCH_CHECK(x.is_cuda(), op, ": x must be on the GPU");
  TORCH_CHECK(wq.device() == x.device() && scale.device() == x.device(), op,
              ": the weight and scale must be on x's device");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kHalf, op,
              ": x must be bf16 or fp16");
  TORCH_CHECK(wq.scalar_type() == (FMT == 8 ? at::kChar : at::kByte), op,
              FMT == 8 ? ": q must be int8" : ": packed must be uint8");
  TORCH_CHECK(scale.scalar_type() == at::kFloat, op, ": scale must be float32");
  TORCH_CHECK(wq.dim() == 2 && wq.size(0) >= 1, op, ": the weight must be 2-d with N >= 1");
  const int64_t N = wq.size(0), K = (FMT == 8 ? 1 : 2) * wq.size(1);
  TORCH_CHECK(K >= 512 && K % 512 == 0, op, ": need K % 512 == 0, got K = ", K);
  TORCH_CHECK(N < (1 << 30) && N * K / 16 < (int64_t(1) << 31), op, ": weight too large");
  if (FMT == 8) {
    TORCH_CHECK(scale.dim() == 1 && scale.size(0) == N, op, ": scale must be (N,)");
  } else {
    TORCH_CHECK(scale.dim() == 2 && scale.size(0) == N && scale.size(1) == K / GROUP, op,
                ": scale must be (N, K / 128)");
  }
  TORCH_CHECK(x.dim() == 2 && x.size(1) == K, op, ": x must be (B, K = ", K, ")");
  const int64_t B = x.size(0);
  TORCH_CHECK(B >= 1 && B <= MAX_ROWS, op, ": need 1 <= B <= 64, got ", B);
  TORCH_CHECK(x.is_contiguous() && wq.is_contiguous() && scale.is_contiguous(), op,
              ": x, the weight and scale must be contiguous");
  TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0 && (uintptr_t)wq.data_ptr() % 16 == 0, op,
              ": x and the weight must be 16-byte aligned");
  return {int(B), int(N), int(K), x.scalar_type() == at::kBFloat16};
}

// Workgroup K split, from (N, K) alone: enough workgroups for TARGET_WGS as
// long as a workgroup keeps one 512-wide unit, at most MAX_KSPLIT ways (the
// partial buffer, B x N fp32 per split, and its reduce grow with the split).
constexpr int TARGET_WGS = 256;
constexpr int MAX_KSPLIT = 8;

int pick_ksplit(int N, int K) {
  const int units = K / UNIT;
  const int groups = (N + WG_ROWS - 1) / WG_ROWS;
  int want = (TARGET_WGS + groups - 1) / groups;
  if (want > MAX_KSPLIT) want = MAX_KSPLIT;
  if (want > units) want = units;
  return want;
}

template <int FMT, int DT, int RT>
void launch_rt(const RowsArgs& a, int ksplit, const at::Tensor& x, const at::Tensor& wq,
               const at::Tensor& scale, at::Tensor& y, hipStream_t stream) {
  const int units = a.K / UNIT;
  const int per = (units + ksplit - 1) / ksplit;
  ksplit = (units + per - 1) / per;  // no empty workgroups
  const size_t lds = (size_t)a.B * XSTRIDE * 2;
  dim3 grid((a.N + WG_ROWS - 1) / WG_ROWS, ksplit), block(256);
  const s16x8* xp = (const s16x8*)x.data_ptr();
  const uint8_t* wp = (const uint8_t*)wq.data_ptr();
  const float* sp = scale.data_ptr<float>();
  uint16_t* yp = (uint16_t*)y.data_ptr();
  if (ksplit == 1) {
    hipLaunchKernelGGL((wq_rows_kernel<FMT, DT, RT>), grid, block, lds, stream, xp, wp, sp,
                       yp, (float*)nullptr, a.B, a.N, a.K, per);
    return;
  }
  at::Tensor part = at::empty({ksplit, a.B, a.N}, x.options().dtype(at::kFloat));
  hipLaunchKernelGGL((wq_rows_kernel<FMT, DT, RT>), grid, block, lds, stream, xp, wp, sp, yp,
                     part.data_ptr<float>(), a.B, a.N, a.K, per);
  const long total = (long)a.B * a.N;
  hipLaunchKernelGGL((wq_rows_reduce_kernel<FMT, DT>), dim3(capped_grid(total, 256)), block,
                     0, stream, part.data_ptr<float>(), sp, yp, ksplit, a.N, total);
}

template <int FMT, int DT>
void launch_dt(const RowsArgs& a, int ksplit, const at::Tensor& x, const at::Tensor& wq,
               const at::Tensor& scale, at::Tensor& y, hipStream_t stream) {
  switch ((a.B + 15) / 16) {
    case 1: launch_rt<FMT, DT, 1>(a, ksplit, x, wq, scale, y, stream); break;
    case 2: launch_rt<FMT, DT, 2>(a, ksplit, x, wq, scale, y, stream); break;
    case 3: launch_rt<FMT, DT, 3>(a, ksplit, x, wq, scale, y, stream); break;
    default: launch_rt<FMT, DT, 4>(a, ksplit, x, wq, scale, y, stream); break;
  }
}

template <int FMT>
at::Tensor gemm_rows(const char* op, const at::Tensor& x, const at::Tensor& wq,
                     const at::Tensor& scale, int64_t ksplit) {
  const RowsArgs a = check_rows<FMT>(op, x, wq, scale);
  TORCH_CHECK(ksplit >= 0 && ksplit <= a.K / UNIT, op, ": ksplit must be in [0, K / 512]");
  const int ks = ksplit == 0 ? pick_ksplit(a.N, a.K) : int(ksplit);
  at::Tensor y = at::empty({a.B, a.N}, x.options());
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  if (a.bf16)
    launch_dt<FMT, 0>(a, ks, x, wq, scale, y, stream);
  else
    launch_dt<FMT, 1>(a, ks, x, wq, scale, y, stream);
  TORCH_CHECK(hipGetLastError() == hipSuccess, op, ": kernel launch failed");
  return y;
}

}  // namespace

// 1 <= B <= 64 (meant for 17..64). ksplit 0 picks the workgroup K split from
// (N, K); a positive value (benchmarks, tests) is used as given, less the
// splits that would be empty.
at::Tensor w8_gemm_rows(at::Tensor x, at::Tensor q, at::Tensor scale, int64_t ksplit) {
  return gemm_rows<8>("w8_gemm_rows", x, q, scale, ksplit);
}

at::Tensor w4_gemm_rows(at::Tensor x, at::Tensor packed, at::Tensor scale, int64_t ksplit) {
  return gemm_rows<4>("w4_gemm_rows", x, packed, scale, ksplit);
}
