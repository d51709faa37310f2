"""Speculative decoding on the CPU: the verify ops are the prefill ops there,
and generate_speculative emits generate_fast's tokens whatever is drafted."""

from __future__ import annotations

import pytest
import torch

from zero_transformer_amd import ops
from zero_transformer_amd.models.inference import generate_fast, generate_speculative
from zero_transformer_amd.ops import reference

from . import _paged as PG
from . import _parity as P
from ._ragged import VOCAB, make_model, make_prompts


def test_verify_ops_are_the_prefill_ops_on_cpu():
    B, H, D, T, R, M = 2, 2, 32, 3, 64, 2
    qkv = P.randn((B, T, 3 * H * D), torch.float32, 1)
    k0 = P.randn((B, H, M * R, D), torch.float32, 2)
    v0 = P.randn((B, H, M * R, D), torch.float32, 3)
    sl = reference.alibi_slopes(H)
    lens = torch.tensor([3, 1], dtype=torch.int32)
    start = torch.tensor([62, 7], dtype=torch.int32)
    bt = PG.make_table(B, M, 5, 4)
    outs = []
    for name in ("prefill", "verify"):
        k, v = k0.clone(), v0.clone()
        kp = PG.scatter(torch.zeros(5, H, R, D), bt, k0)
        vp = PG.scatter(torch.zeros(5, H, R, D), bt, v0)
        o = getattr(ops, f"attention_{name}_append")(qkv, k, v, H, sl, lens, start)
        op = getattr(ops, f"attention_{name}_paged")(qkv, kp, vp, H, sl, bt, lens, start)
        outs.append((o, k, v, op, kp, vp))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("kind", ["oracle", "wrong", "lookup"])
def test_generate_speculative_equals_generate_fast_on_cpu(kind):
    """fp32, two prompts of 9 tokens in one batch, 11 new tokens, draft_len 4:
    the known continuation (3 = ceil(11 / 5) steps, the rest accepted), a wrong
    first draft token (11 steps, nothing accepted, every step rolled back) and
    the default prompt lookup."""
    model, n, K = make_model(), 11, 4
    idx = torch.tensor(make_prompts((9, 9)))
    want = generate_fast(model, idx, n, use_graph=False)
    ref = want.tolist()

    def fn(tokens):
        nxt = [ref[b][len(t):len(t) + K] for b, t in enumerate(tokens)]
        return nxt if kind == "oracle" else [[(x + 1) % VOCAB for x in r] for r in nxt]

    toks, steps, accepted = generate_speculative(
        model, idx, n, draft_len=K, draft_fn=None if kind == "lookup" else fn)
    assert torch.equal(toks, want)
    if kind == "oracle":
        assert (steps, accepted) == (3, 2 * (n - 3))
    if kind == "wrong":
        assert (steps, accepted) == (n, 0)
