// Python bindings for the zero_transformer_amd gfx950 HIP kernels.

#include <torch/extension.h>

#include <vector>

std::vector<at::Tensor> layernorm_fwd(at::Tensor x, at::Tensor w, double eps);
std::vector<at::Tensor> add_ln_fwd(at::Tensor x, at::Tensor h, at::Tensor w,
                                   double eps);
std::vector<at::Tensor> layernorm_bwd(at::Tensor dy, at::Tensor x, at::Tensor w,
                                      at::Tensor rstd, at::Tensor mean);
at::Tensor gelu_fwd(at::Tensor x);
at::Tensor gelu_bwd(at::Tensor dy, at::Tensor x);
std::vector<at::Tensor> cross_entropy_fwd(at::Tensor logits, at::Tensor targets,
                                          int64_t divisor);
at::Tensor cross_entropy_bwd(at::Tensor logits, at::Tensor targets, at::Tensor lse,
                             at::Tensor dloss, int64_t divisor);
void adamw_step(at::Tensor p, at::Tensor p_bf16, at::Tensor g, at::Tensor m,
                at::Tensor v, long step, double lr, double beta1, double beta2,
                double eps, double wd, double clip, double grad_scale,
                c10::optional<at::Tensor> sumsq_out);
std::vector<at::Tensor> residual_ln_fwd(at::Tensor x, at::Tensor h, at::Tensor w,
                                        double p, int64_t seed, double eps);
std::vector<at::Tensor> residual_ln_bwd(at::Tensor dy, at::Tensor xp, at::Tensor w,
                                        at::Tensor rstd, at::Tensor mean,
                                        c10::optional<at::Tensor> dxp, double p,
                                        int64_t seed);
at::Tensor residual_dropout_fwd(at::Tensor x, at::Tensor h, double p, int64_t seed);
at::Tensor residual_dropout_bwd(at::Tensor dy, double p, int64_t seed);
at::Tensor attn_decode(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor slopes,
                       at::Tensor s_used);
at::Tensor attn_decode_append(at::Tensor qkv, at::Tensor k_cache,
                              at::Tensor v_cache, at::Tensor slopes,
                              at::Tensor lens);
at::Tensor attn_prefill_append(at::Tensor qkv, at::Tensor k_cache,
                               at::Tensor v_cache, at::Tensor slopes,
                               at::Tensor lens, at::Tensor start);
at::Tensor attn_prefill_paged(at::Tensor qkv, at::Tensor k_pool, at::Tensor v_pool,
                              at::Tensor slopes, at::Tensor block_table,
                              at::Tensor lens, at::Tensor start);
at::Tensor attn_decode_paged(at::Tensor qkv, at::Tensor k_pool, at::Tensor v_pool,
                             at::Tensor slopes, at::Tensor block_table,
                             at::Tensor lens);
std::vector<at::Tensor> attn_fwd(at::Tensor qkv, at::Tensor slopes, int64_t H,
                                 double p_drop, int64_t seed);
std::vector<at::Tensor> attn_bwd(at::Tensor dout, at::Tensor qkv, at::Tensor slopes,
                                 at::Tensor o, at::Tensor lse, int64_t H,
                                 double p_drop, int64_t seed, int64_t fused);
at::Tensor gemm_gelu(at::Tensor x, at::Tensor w);
at::Tensor gemv(at::Tensor x, at::Tensor w);
std::vector<at::Tensor> sample_rows(at::Tensor logits, c10::optional<at::Tensor> seen,
                                    at::Tensor temperature, at::Tensor top_k,
                                    at::Tensor top_p, at::Tensor penalty,
                                    at::Tensor seed, at::Tensor counter);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("layernorm_fwd", &layernorm_fwd, "bias-free LayerNorm fwd (gfx950)");
  m.def("add_ln_fwd", &add_ln_fwd,
        "fused residual-add + LayerNorm (decode path, no grads)");
  m.def("layernorm_bwd", &layernorm_bwd, "bias-free LayerNorm bwd (gfx950)");
  m.def("gelu_fwd", &gelu_fwd, "tanh GELU fwd (gfx950)");
  m.def("gelu_bwd", &gelu_bwd, "tanh GELU bwd (gfx950)");
  m.def("cross_entropy_fwd", &cross_entropy_fwd, "fused gather CE fwd (gfx950)");
  m.def("cross_entropy_bwd", &cross_entropy_bwd, "fused gather CE bwd (gfx950)");
  m.def("adamw_step", &adamw_step,
        "fused ZeRO-1 AdamW shard step, optionally returning sum(g^2) (gfx950)",
        pybind11::arg("p"), pybind11::arg("p_bf16"), pybind11::arg("g"),
        pybind11::arg("m"), pybind11::arg("v"), pybind11::arg("step"),
        pybind11::arg("lr"), pybind11::arg("beta1"), pybind11::arg("beta2"),
        pybind11::arg("eps"), pybind11::arg("wd"), pybind11::arg("clip"),
        pybind11::arg("grad_scale"), pybind11::arg("sumsq_out") = pybind11::none());
  m.def("residual_ln_fwd", &residual_ln_fwd,
        "fused x + dropout(h) and LayerNorm of it, fwd (gfx950)");
  m.def("residual_ln_bwd", &residual_ln_bwd,
        "fused LayerNorm bwd + residual grad sum + dropout bwd (gfx950)");
  m.def("residual_dropout_fwd", &residual_dropout_fwd, "fused x + dropout(h) fwd (gfx950)");
  m.def("residual_dropout_bwd", &residual_dropout_bwd, "fused x + dropout(h) bwd (gfx950)");
  m.def("attn_decode", &attn_decode, "single-token KV-cache ALiBi attention (gfx950)");
  m.def("attn_decode_append", &attn_decode_append,
        "decode attention on the fused qkv row with per-sequence lengths; "
        "appends the new K/V row to the caches in place (gfx950)");
  m.def("attn_prefill_append", &attn_prefill_append,
        "prefill attention on the fused qkv rows against the KV cache, with "
        "per-sequence new-row counts and cached-row offsets; fills the caches "
        "in place (gfx950 MFMA)");
  m.def("attn_prefill_paged", &attn_prefill_paged,
        "attn_prefill_append on a paged KV pool (P, H, R, D) addressed through a "
        "(B, M) block table (gfx950 MFMA)");
  m.def("attn_decode_paged", &attn_decode_paged,
        "attn_decode_append on a paged KV pool (P, H, R, D) addressed through a "
        "(B, M) block table (gfx950)");
  m.def("attn_fwd", &attn_fwd, "fused causal ALiBi flash attention fwd (gfx950 MFMA)");
  // fused: -1 = process default (ZTA_BWD_FUSED), 0 = two-kernel dq + dkdv,
  // 1 = single fused kernel (head_dim 128; other dims take the two-kernel path)
  m.def("attn_bwd", &attn_bwd, "fused causal ALiBi flash attention bwd (gfx950 MFMA)",
        py::arg("dout"), py::arg("qkv"), py::arg("slopes"), py::arg("o"),
        py::arg("lse"), py::arg("H"), py::arg("p_drop"), py::arg("seed"),
        py::arg("fused") = -1);
  m.def("gemm_gelu", &gemm_gelu,
        "hipBLASLt x@w^T with fused GELU epilogue (no-grad path)");
  m.def("gemv", &gemv, "weight-streaming decode GEMV x@w^T (gfx950)");
  m.def("sample_rows", &sample_rows,
        "fused sort-free sampler, one workgroup per row, per-row options and "
        "counter-based RNG -> {tokens, cut} (gfx950)");
}
