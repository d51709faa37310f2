"""Weight-only int8 ("W8A16") storage for the inference model.

quantize_w8_(model) replaces the four projection weights of every block (the
fused (3C, C) qkv weight, attn.fc_resid, mlp.fc1, mlp.fc_resid) by int8 rows
with one fp32 scale per output row (ops.reference.quantize_rows_w8) and frees
the 16-bit parameters: half the bytes every decode step streams, half the
block weights' memory. wte / lm_head (tied), the LayerNorm weights and the KV
cache stay 16-bit. models/inference.py reaches a projection weight through
one helper (`_linear`), which sends a W8Weight to ops.linear_w8; nothing else
in the model, the caches or the serving engine knows about the format.
"""

from __future__ import annotations

import torch
import torch.nn as nn

from ..ops.reference import quantize_rows_w8


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


def quantize_w8_(model):
    """Quantize an inference GPT2 in place (after loading its 16-bit or fp32
    checkpoint) and return it. Idempotent."""
    for block in model.blocks:
        attn, mlp = block.attn, block.mlp
        if attn.qkv_w8 is None:
            w = torch.cat([attn.query.weight, attn.key.weight, attn.value.weight], dim=0)
            attn.qkv_w8 = W8Weight.from_float(w)
            attn.query = attn.key = attn.value = None
            attn._qkv_w = None
        for mod, name in ((attn, "fc_resid"), (mlp, "fc1"), (mlp, "fc_resid")):
            lin = getattr(mod, name)
            if not isinstance(lin, W8Weight):
                setattr(mod, name, W8Weight.from_float(lin.weight))
    return model
