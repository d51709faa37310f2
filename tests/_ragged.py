"""The small model and prompts shared by tests/test_ragged_decode.py (CPU)
and tests/test_gpu_ragged_decode.py."""

from __future__ import annotations

import torch

from zero_transformer_amd.models.inference import GPT2

SEED = 15  # see test_ragged_decode.greedy_ref: top-2 gaps >= 0.1, EOS case holds
LENS = (5, 12, 9)
VOCAB = 512


def make_model(num_ctx=64, lively=True):
    """GPT2(256, 512, 4 heads, N=2), seeded. Under the default init the tied
    N(0, 1) embedding dominates the residual stream and greedy decoding just
    echoes the last prompt token, whatever the attention does; `lively`
    shrinks the embedding and scales the two residual projections up so that
    the attention and MLP branches decide the next token (and a misplaced
    cache row changes it)."""
    torch.manual_seed(SEED)
    m = GPT2(embedding_dim=256, vocab_size=VOCAB, num_head=4, num_ctx=num_ctx, N=2)
    if lively:
        with torch.no_grad():
            torch.nn.init.normal_(m.wte.weight, std=0.1)
            for b in m.blocks:
                b.attn.fc_resid.weight.mul_(8.0)
                b.mlp.fc_resid.weight.mul_(8.0)
    return m.eval()


def make_prompts(lens=LENS):
    g = torch.Generator().manual_seed(SEED + 1)
    return [torch.randint(1, VOCAB, (n,), generator=g).tolist() for n in lens]
