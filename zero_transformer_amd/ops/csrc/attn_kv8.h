// Argument checks shared by the ops on the int8 paged KV cache (attn_kv8.hip,
// attn_verify_kv8.hip); the cache format is described in attn_kv8.hip.
#pragma once

#include "attn_kv.h"

#include <ATen/ATen.h>
#include <torch/extension.h>

namespace {

// Returns the pool geometry.
Pool check_kv8(const char* op, const at::Tensor& kp, const at::Tensor& vp,
               const at::Tensor& ksc, const at::Tensor& vsc, const at::Tensor& bt,
               std::initializer_list<const at::Tensor*> per_seq) {
  TORCH_CHECK(kp.is_cuda() && vp.is_cuda() && kp.dim() == 4 && kp.is_contiguous() &&
                  vp.is_contiguous() && kp.sizes() == vp.sizes() &&
                  kp.scalar_type() == at::kByte && vp.scalar_type() == at::kByte &&
                  kp.size(0) >= 1,
              op, ": k_pool/v_pool must be (P, H, R, D) contiguous uint8 with P >= 1");
  const long D = kp.size(3);
  TORCH_CHECK(D == 32 || D == 64 || D == 96 || D == 128, op,
              ": head_dim must be one of 32/64/96/128, got ", D);
  TORCH_CHECK(kp.size(2) % TB == 0 && kp.size(2) > 0, op,
              ": rows per page must be a positive multiple of ", TB);
  for (const at::Tensor* s : {&ksc, &vsc})
    TORCH_CHECK(s->is_cuda() && s->scalar_type() == at::kFloat && s->dim() == 3 &&
                    s->is_contiguous() && s->size(0) == kp.size(0) &&
                    s->size(1) == kp.size(1) && s->size(2) == kp.size(2),
                op, ": k_scale/v_scale must be (P, H, R) contiguous fp32");
  TORCH_CHECK(bt.is_cuda() && bt.scalar_type() == at::kInt && bt.dim() == 2 &&
                  bt.size(1) >= 1 && bt.is_contiguous(),
              op, ": block_table must be a (B, M) contiguous int32 device tensor, M >= 1");
  TORCH_CHECK(bt.size(1) * kp.size(2) < (1L << 31), op, ": M * R must fit in int32");
  for (const at::Tensor* t : per_seq)
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kInt && t->dim() == 1 &&
                    t->numel() == bt.size(0) && t->is_contiguous(),
                op, ": lens / start / rows must be (B,) contiguous int32 device tensors");
  return {(int)kp.size(0), (int)kp.size(2), (int)bt.size(1)};
}

void check_qkv(const char* op, const at::Tensor& qkv, const at::Tensor& kp,
               const at::Tensor& bt) {
  TORCH_CHECK(qkv.is_cuda() && qkv.is_contiguous() && qkv.dim() == 3 &&
                  qkv.size(2) == 3 * kp.size(1) * kp.size(3) && qkv.size(0) == bt.size(0),
              op, ": qkv must be (B, T, 3C) contiguous with C == H*D and B table rows");
  TORCH_CHECK(qkv.scalar_type() == at::kHalf || qkv.scalar_type() == at::kBFloat16, op,
              ": fp16 or bf16 only");
}

}  // namespace
