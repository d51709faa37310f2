"""GPT-2-style decoder-only transformer with ALiBi, built MI355X-first.

Same capabilities as the reference Flax model (src/models/GPT.py:53-113,
src/models/layers.py:47-191): bias-free q/k/v/out projections, 4x GELU MLP,
bias-free LayerNorm, weight-tied token embedding / LM head, ALiBi attention
bias, shifted fp32 cross-entropy loss, 0.02-normal init with 1/sqrt(2N)
scaling on residual-out projections.

Parameter names follow the torch_compatability .pth contract
(reference flax_to_pytorch.py:10-35,96-114):
    wte.weight, norm.weight, lm_head.weight,
    blocks.{i}.ln1.weight, blocks.{i}.ln2.weight,
    blocks.{i}.attn.{query,key,value,fc_resid}.weight,
    blocks.{i}.mlp.{fc1,fc_resid}.weight

The hot ops route through zero_transformer_amd.ops: fused HIP/CDNA4 kernels
on GPU, fp32 torch reference on CPU.
"""

from __future__ import annotations

import math
from typing import Optional, Tuple, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..utils.config import load_config


class LayerNorm(nn.Module):
    """Bias-free LayerNorm (flax nn.LayerNorm(use_bias=False), eps 1e-6)."""

    def __init__(self, dim: int, eps: float = 1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.eps = eps

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ops.layer_norm(x, self.weight, self.eps)


class CausalSelfAttention(nn.Module):
    """Causal multi-head attention with optional ALiBi position biasing.

    The q/k/v projections run as ONE fused GEMM (qkv_w, (3C, C)) — one pass
    over x and a bigger, better-shaped hipBLASLt GEMM than three (C, C)
    calls. The .pth contract (separate query/key/value weights,
    flax_to_pytorch.py:10-35) is preserved at every state_dict boundary by
    the _save/_load hooks below.
    """

    def __init__(self, cfg):
        super().__init__()
        dim, heads = cfg.embedding_dim, cfg.num_head
        assert dim % heads == 0
        self.dim = dim
        self.num_head = heads
        self.head_dim = dim // heads
        self.dropout_p = cfg.dropout
        self.qkv_w = nn.Parameter(torch.empty(3 * dim, dim))
        self.fc_resid = nn.Linear(dim, dim, bias=False)
        if cfg.alibi_attn:
            self.register_buffer("slopes", ops.alibi_slopes(heads), persistent=False)
        else:
            self.slopes = None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """Returns the PRE-dropout attention output; the residual dropout is
        fused into the Block's residual add (ops.residual_dropout_add)."""
        qkv = ops.linear(x, self.qkv_w)  # (B, T, 3C); explicit-GEMM backward
        o = ops.attention_qkv(
            qkv, self.num_head, self.slopes,
            dropout_p=self.dropout_p, training=self.training,
        )
        return ops.linear(o, self.fc_resid.weight)

    # .pth contract: expose query/key/value instead of the fused qkv_w
    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        w = destination.pop(prefix + "qkv_w")
        C = self.dim
        destination[prefix + "query.weight"] = w[:C]
        destination[prefix + "key.weight"] = w[C : 2 * C]
        destination[prefix + "value.weight"] = w[2 * C :]

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        C = self.dim
        names = [prefix + n + ".weight" for n in ("query", "key", "value")]
        if all(n in state_dict for n in names):
            state_dict[prefix + "qkv_w"] = torch.cat(
                [state_dict.pop(n) for n in names], dim=0
            )
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


class MLP(nn.Module):
    """4x expansion GELU MLP (reference layers.py:47-77). The trailing
    dropout is fused into the Block's residual add."""

    def __init__(self, cfg):
        super().__init__()
        dim = cfg.embedding_dim
        self.fc1 = nn.Linear(dim, 4 * dim, bias=False)
        self.fc_resid = nn.Linear(4 * dim, dim, bias=False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ops.mlp_gelu(x, self.fc1.weight, self.fc_resid.weight)


class Block(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.dropout_p = cfg.dropout
        self.ln1 = LayerNorm(cfg.embedding_dim)
        self.attn = CausalSelfAttention(cfg)
        self.ln2 = LayerNorm(cfg.embedding_dim)
        self.mlp = MLP(cfg)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        # residual adds with the reference's resid/MLP dropout fused in
        # (dropout(h) then add, layers.py:76,190 + GPT.py:43-49); the first
        # add also yields ln2 of its result from the same kernel
        x, ln_x = self._attn_half(x, self.ln1(x))
        return ops.residual_dropout_add(
            x, self.mlp(ln_x), self.dropout_p, self.training
        )

    def _attn_half(self, x: torch.Tensor, ln_x: torch.Tensor):
        """(x, ln1(x)) -> (x', ln2(x')), x' = x + dropout(attn(ln1(x)))."""
        return ops.residual_dropout_add_ln(
            x, self.attn(ln_x), self.dropout_p, self.training,
            self.ln2.weight, self.ln2.eps,
        )

    def forward_pair(self, x: torch.Tensor, ln_x: torch.Tensor, next_norm: LayerNorm):
        """The block on the carried pair (x, ln_x = ln1(x)) -> (x_out,
        next_norm(x_out)): each residual add is fused with the LayerNorm
        that reads its result (ln2; then the next block's ln1, or the
        model's final norm). The LayerNorm modules' weights are read
        directly: forward hooks on ln2 or on next_norm do not fire."""
        x, ln_x = self._attn_half(x, ln_x)
        return ops.residual_dropout_add_ln(
            x, self.mlp(ln_x), self.dropout_p, self.training,
            next_norm.weight, next_norm.eps,
        )


class GPT(nn.Module):
    """Decoder-only transformer with tied wte/lm_head."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.N = cfg.N
        self.vocab_size = cfg.vocab_size
        self.block_size = cfg.block_size
        self.wte = nn.Embedding(cfg.vocab_size, cfg.embedding_dim)
        self.blocks = nn.ModuleList([Block(cfg) for _ in range(cfg.N)])
        self.norm = LayerNorm(cfg.embedding_dim)
        self.lm_head = nn.Linear(cfg.embedding_dim, cfg.vocab_size, bias=False)
        self.lm_head.weight = self.wte.weight  # weight tying (GPT.py:100)
        self._init_weights()

    def _init_weights(self):
        scaled = 0.02 / math.sqrt(2 * self.N)
        for name, p in self.named_parameters():
            if p.dim() == 1:  # LayerNorm weights
                nn.init.ones_(p)
            elif "fc_resid" in name:  # residual-out projections (layers.py:72,184)
                nn.init.normal_(p, std=scaled)
            else:
                nn.init.normal_(p, std=0.02)

    def forward(
        self,
        idx: torch.Tensor,
        labels: Optional[torch.Tensor] = None,
    ) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
        x = self.wte(idx)
        # carry (x, LN(x)) from block to block, as the decode path of
        # models/inference.py does: only the first LayerNorm is a kernel of
        # its own. Blocks run through forward_pair, not Block.__call__, and
        # the later LayerNorms through their weights: module forward hooks on
        # blocks, ln2, later ln1 and the final norm do not fire here (attn
        # and mlp are still called as modules).
        norms = [b.ln1 for b in self.blocks] + [self.norm]
        ln_x = norms[0](x)
        for i, block in enumerate(self.blocks):
            x, ln_x = block.forward_pair(x, ln_x, norms[i + 1])
        x = ln_x
        logits = F.linear(x, self.lm_head.weight)
        if labels is None:
            return logits
        # Shifted CE (GPT.py:105-111): predict token t+1 from position t.
        # Full contiguous logits + an ignored (-1) target at each sequence
        # end: no [:, :-1] slice -> no 1.6 GB .contiguous() copy on the
        # forward and no pad-scatter on the backward.
        B, T = labels.shape
        tgt = torch.cat(
            [labels[..., 1:], labels.new_full((B, 1), -1)], dim=-1
        ).reshape(-1)
        loss = ops.cross_entropy(
            logits.reshape(-1, logits.shape[-1]), tgt, divisor=B * (T - 1)
        )
        return logits, loss

    def num_params(self, non_embedding: bool = False) -> int:
        n = sum(p.numel() for p in self.parameters())
        if non_embedding:
            n -= self.wte.weight.numel()
        return n


def model_getter(
    model_size: str,
    config_path: str = "conf/model_config.yaml",
    return_cfg: bool = False,
    dtype: torch.dtype = torch.float32,
):
    """Build a GPT from a named YAML section (reference GPT.py:116-137)."""
    configs = load_config(config_path)
    assert model_size in configs, "Invalid model name provided"
    assert dtype in (torch.float16, torch.bfloat16, torch.float32), "Invalid dtype provided"
    model = GPT(configs[model_size])
    if dtype != torch.float32:
        model = model.to(dtype)
    if return_cfg:
        return model, configs[model_size]
    return model
