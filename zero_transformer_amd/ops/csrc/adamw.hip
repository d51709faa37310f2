// Fused AdamW on a flat fp32 master shard (the ZeRO-1 sharded update,
// reference xmap_train_functions.py:110-123 + optax chain main_zero.py:160-168):
// grad*scale -> element-wise clip(+-clip) -> Adam moments (b2=0.95, bias
// correction) -> decoupled weight decay -> param -= lr*update, emitting the
// bf16 working copy for the all-gather in the same pass.
// Memory-bound over 4 fp32 streams: vectorized f32x4 access.
//
// SUMSQ instances also return the sum of g^2 of the RAW gradient (as stored,
// before grad_scale and the clip) for the grad-norm metric, from the values
// the update loads anyway: fp32 per thread, block_reduce_sum, one partial per
// block, then sumsq_final adds the partials in a fixed order. No atomics, so
// the sum is bit-reproducible from call to call. The update is untouched.

#include "common.h"

#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

namespace {

template <typename GT, bool EMIT_BF16>
ZTA_DEV void adamw_elem(float& pi, uint16_t* pb, float& mi_io, float& vi_io,
                        GT gv, float lr, float beta1, float beta2, float eps,
                        float wd, float clip, float gscale, float inv_bc1,
                        float inv_bc2) {
  float gi = to_f32(gv) * gscale;
  // clip == 0 turns clipping off (as reference.adamw_update), it does not
  // clamp every gradient to 0
  if (clip != 0.f) gi = fminf(fmaxf(gi, -clip), clip);
  float mi = beta1 * mi_io + (1.f - beta1) * gi;
  float vi = beta2 * vi_io + (1.f - beta2) * gi * gi;
  mi_io = mi;
  vi_io = vi;
  float update = (mi * inv_bc1) / (sqrtf(vi * inv_bc2) + eps);
  if (wd != 0.f) update += wd * pi;
  pi -= lr * update;
  if (EMIT_BF16) *pb = f32_to_bf16(pi);
}

// one partial per block; every thread of the block must arrive
ZTA_DEV void sumsq_block(float sq, float* __restrict__ sq_part) {
  __shared__ float scratch[16];
  sq = block_reduce_sum(sq, scratch);
  if (threadIdx.x == 0) sq_part[blockIdx.x] = sq;
}

template <typename GT, bool EMIT_BF16, bool SUMSQ>
__global__ void adamw_kernel(float* __restrict__ p, uint16_t* __restrict__ p_bf16,
                             const GT* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ v, long n, float lr, float beta1,
                             float beta2, float eps, float wd, float clip,
                             float gscale, float inv_bc1, float inv_bc2,
                             float* __restrict__ sq_part) {
  float sq = 0.f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x) {
    float pi = p[i];
    uint16_t pb;
    const GT gi = g[i];
    if constexpr (SUMSQ) {
      const float gf = to_f32(gi);
      sq += gf * gf;
    }
    adamw_elem<GT, EMIT_BF16>(pi, &pb, m[i], v[i], gi, lr, beta1, beta2, eps,
                              wd, clip, gscale, inv_bc1, inv_bc2);
    p[i] = pi;
    if (EMIT_BF16) p_bf16[i] = pb;
  }
  if constexpr (SUMSQ) sumsq_block(sq, sq_part);
}

// 4 elements per lane with f32x4 / 64-bit packed access on every stream
// (the scalar form measured ~5.2 TB/s of its ~7 TB/s roof; shard sizes are
// 128-element aligned so n % 4 == 0 always holds on the training path).
typedef __attribute__((ext_vector_type(4))) short s16x4v;

template <typename GT>
struct VecOf;
template <>
struct VecOf<uint16_t> {
  using type = s16x4v;
};
template <>
struct VecOf<float> {
  using type = f32x4;
};

template <typename GT, bool EMIT_BF16, bool SUMSQ>
__global__ void adamw_kernel_v4(float* __restrict__ p, uint16_t* __restrict__ p_bf16,
                                const GT* __restrict__ g, float* __restrict__ m,
                                float* __restrict__ v, long n4, float lr,
                                float beta1, float beta2, float eps, float wd,
                                float clip, float gscale, float inv_bc1,
                                float inv_bc2, float* __restrict__ sq_part) {
  float sq = 0.f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4;
       i += (long)gridDim.x * blockDim.x) {
    // vector loads -> scalar arrays (ext_vector elements cannot bind to
    // references) -> vector stores
    union F4 {
      f32x4 v;
      float a[4];
    };
    F4 pv{reinterpret_cast<f32x4*>(p)[i]};
    F4 mv{reinterpret_cast<f32x4*>(m)[i]};
    F4 vv{reinterpret_cast<f32x4*>(v)[i]};
    GT gv[4];
    using GV = typename VecOf<GT>::type;
    *reinterpret_cast<GV*>(gv) = reinterpret_cast<const GV*>(g)[i];
    uint16_t pb[4];
    if constexpr (SUMSQ) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gf = to_f32(gv[e]);
        sq += gf * gf;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
      adamw_elem<GT, EMIT_BF16>(pv.a[e], &pb[e], mv.a[e], vv.a[e], gv[e], lr,
                                beta1, beta2, eps, wd, clip, gscale, inv_bc1,
                                inv_bc2);
    reinterpret_cast<f32x4*>(p)[i] = pv.v;
    reinterpret_cast<f32x4*>(m)[i] = mv.v;
    reinterpret_cast<f32x4*>(v)[i] = vv.v;
    if (EMIT_BF16)
      reinterpret_cast<s16x4v*>(p_bf16)[i] = *reinterpret_cast<s16x4v*>(pb);
  }
  if constexpr (SUMSQ) sumsq_block(sq, sq_part);
}

// one block: thread t adds partials t, t + 256, ... in order, then the block
// reduces
__global__ void sumsq_final(const float* __restrict__ sq_part, int npart,
                            float* __restrict__ out) {
  __shared__ float scratch[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < npart; i += blockDim.x) s += sq_part[i];
  s = block_reduce_sum(s, scratch);
  if (threadIdx.x == 0) out[0] = s;
}

}  // namespace

void adamw_step(at::Tensor p, at::Tensor p_bf16, at::Tensor g, at::Tensor m,
                at::Tensor v, long step, double lr, double beta1, double beta2,
                double eps, double wd, double clip, double grad_scale,
                c10::optional<at::Tensor> sumsq_out) {
  TORCH_CHECK(p.is_cuda() && p.is_contiguous() && p.scalar_type() == at::kFloat);
  TORCH_CHECK(m.scalar_type() == at::kFloat && v.scalar_type() == at::kFloat);
  const long n = p.numel();
  const bool emit = p_bf16.numel() == n;
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const int block = 256;
  const float inv_bc1 = 1.f / (1.f - powf((float)beta1, (float)step));
  const float inv_bc2 = 1.f / (1.f - powf((float)beta2, (float)step));
  const bool v4 = n % 4 == 0;
  const long nwork = v4 ? n / 4 : n;
  const int grid = capped_grid(nwork, block, 4096);
  const bool sumsq = sumsq_out.has_value() && sumsq_out->defined();
  at::Tensor sq_part;
  float* sq_part_ptr = nullptr;
  if (sumsq) {
    TORCH_CHECK(sumsq_out->is_cuda() && sumsq_out->scalar_type() == at::kFloat &&
                    sumsq_out->numel() == 1,
                "adamw: sumsq_out must be one fp32 element on the device");
    sq_part = at::empty({grid}, p.options());
    sq_part_ptr = sq_part.data_ptr<float>();
  }

#define LAUNCH(K, GT, EMIT, SQ, NW)                                                    \
  hipLaunchKernelGGL((K<GT, EMIT, SQ>), dim3(grid), dim3(block), 0, stream,            \
                     p.data_ptr<float>(), (uint16_t*)p_bf16.data_ptr(),                \
                     (const GT*)g.data_ptr(), m.data_ptr<float>(),                     \
                     v.data_ptr<float>(), NW, (float)lr, (float)beta1, (float)beta2,   \
                     (float)eps, (float)wd, (float)clip, (float)grad_scale, inv_bc1,   \
                     inv_bc2, sq_part_ptr)
#define LAUNCH_SQ(K, GT, EMIT, NW)            \
  do {                                        \
    if (sumsq) LAUNCH(K, GT, EMIT, true, NW); \
    else LAUNCH(K, GT, EMIT, false, NW);      \
  } while (0)
#define DISPATCH(GT)                                          \
  do {                                                        \
    if (v4) {                                                 \
      if (emit) LAUNCH_SQ(adamw_kernel_v4, GT, true, nwork);  \
      else LAUNCH_SQ(adamw_kernel_v4, GT, false, nwork);      \
    } else {                                                  \
      if (emit) LAUNCH_SQ(adamw_kernel, GT, true, n);         \
      else LAUNCH_SQ(adamw_kernel, GT, false, n);             \
    }                                                         \
  } while (0)

  if (g.scalar_type() == at::kBFloat16) {
    DISPATCH(uint16_t);
  } else if (g.scalar_type() == at::kFloat) {
    DISPATCH(float);
  } else {
    TORCH_CHECK(false, "adamw: unsupported grad dtype");
  }
#undef DISPATCH
#undef LAUNCH_SQ
#undef LAUNCH
  if (sumsq)
    hipLaunchKernelGGL(sumsq_final, dim3(1), dim3(256), 0, stream, sq_part_ptr, grid,
                       sumsq_out->data_ptr<float>());
}
