"""Weight-only int8 ("W8A16") and int4 ("W4A16") storage for the inference model.

quantize_w8_(model) replaces the four projection weights of every block (the
fused (3C, C) qkv weight, attn.fc_resid, mlp.fc1, mlp.fc_resid) by int8 rows
with one fp32 scale per output row (ops.reference.quantize_rows_w8) and frees
the 16-bit parameters: half the bytes every decode step streams, half the
block weights' memory. quantize_w4_(model) does the same with 4-bit codes
and one fp32 scale per row and group of 128 k (ops.reference.quantize_rows_w4,
the GPTQ / AWQ storage shape): a quarter of the bytes plus 1/64 for the
scales. wte / lm_head (tied), the LayerNorm weights and the KV cache stay
16-bit. models/inference.py reaches a projection weight through one helper
(`_linear`), which sends a W8Weight to ops.linear_w8 and a W4Weight to
ops.linear_w4; nothing else in the model, the caches or the serving engine
knows about the formats. The attention's fused-qkv slot (`attn.qkv_w8`, named
when int8 was the only format) holds the fused weight of either format.
"""

from __future__ import annotations

import torch
import torch.nn as nn

from ..ops.reference import quantize_rows_w4, quantize_rows_w8


class W8Weight(nn.Module):
    """An (N, K) weight as buffers `q` (int8, (N, K)) and `scale` (fp32,
    (N,)). It stands where an nn.Linear stood, and `.weight` is the object
    itself, so `module.fc1.weight` keeps naming the thing a projection reads.
    state_dict() carries q and scale; loading them into a quantized model
    restores them."""

    def __init__(self, q: torch.Tensor, scale: torch.Tensor):
        super().__init__()
        self.register_buffer("q", q.contiguous())
        self.register_buffer("scale", scale.float().contiguous())

    @classmethod
    def from_float(cls, w: torch.Tensor) -> "W8Weight":
        return cls(*quantize_rows_w8(w))

    @property
    def weight(self) -> "W8Weight":
        return self

    @property
    def shape(self):
        return self.q.shape

    def rows(self, lo: int, hi: int) -> "W8Weight":
        """Output rows [lo, hi) as views (row slices stay contiguous)."""
        return W8Weight(self.q[lo:hi], self.scale[lo:hi])

    def _apply(self, fn, recurse=True):
        # model.half() / .to(dtype) casts floating buffers, which would round
        # the scales: keep the fp32 values and follow device moves only (q is
        # int8, so a dtype cast leaves it alone and it shows the device)
        scale = self.scale
        super()._apply(fn, recurse)
        self.scale = scale.to(self.q.device)
        return self


class W4Weight(nn.Module):
    """An (N, K) weight as buffers `packed` (uint8, (N, K/2): 4-bit codes in
    the nibble order of ops.reference.quantize_rows_w4) and `scale` (fp32,
    (N, K/128)). Stands where an nn.Linear stood, like W8Weight: `.weight` is
    the object itself, `.shape` the logical (N, K), state_dict() carries
    packed and scale."""

    def __init__(self, packed: torch.Tensor, scale: torch.Tensor):
        super().__init__()
        self.register_buffer("packed", packed.contiguous())
        self.register_buffer("scale", scale.float().contiguous())

    @classmethod
    def from_float(cls, w: torch.Tensor) -> "W4Weight":
        return cls(*quantize_rows_w4(w))

    @property
    def weight(self) -> "W4Weight":
        return self

    @property
    def shape(self):
        return torch.Size((self.packed.shape[0], 2 * self.packed.shape[1]))

    def rows(self, lo: int, hi: int) -> "W4Weight":
        """Output rows [lo, hi) as views (row slices of both stay contiguous)."""
        return W4Weight(self.packed[lo:hi], self.scale[lo:hi])

    def _apply(self, fn, recurse=True):
        # as W8Weight._apply: a dtype cast must not round the fp32 scales
        scale = self.scale
        super()._apply(fn, recurse)
        self.scale = scale.to(self.packed.device)
        return self


def _quantize_(model, cls):
    other = W4Weight if cls is W8Weight else W8Weight
    for block in model.blocks:
        attn, mlp = block.attn, block.mlp
        held = [attn.qkv_w8] + [getattr(m, n) for m, n in
                                ((attn, "fc_resid"), (mlp, "fc1"), (mlp, "fc_resid"))]
        assert not any(isinstance(h, other) for h in held), \
            f"the model already holds {other.__name__} projections"
        if attn.qkv_w8 is None:
            w = torch.cat([attn.query.weight, attn.key.weight, attn.value.weight], dim=0)
            attn.qkv_w8 = cls.from_float(w)
            attn.query = attn.key = attn.value = None
            attn._qkv_w = None
        for mod, name in ((attn, "fc_resid"), (mlp, "fc1"), (mlp, "fc_resid")):
            lin = getattr(mod, name)
            if not isinstance(lin, cls):
                setattr(mod, name, cls.from_float(lin.weight))
    return model


def quantize_w8_(model):
    """Quantize an inference GPT2 in place (after loading its 16-bit or fp32
    checkpoint) and return it. Idempotent."""
    return _quantize_(model, W8Weight)


def quantize_w4_(model):
    """quantize_w8_ with group-scaled 4-bit weights (every projection's K must
    be a multiple of 128). Idempotent."""
    return _quantize_(model, W4Weight)
