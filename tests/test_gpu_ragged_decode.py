"""Ragged batched decode on the GPU: the decode-attention kernel with
per-sequence lengths and the fused cache append (ops/csrc/attn_decode.hip),
and generate_batch on top of it."""

from __future__ import annotations

import math

import pytest
import torch

from zero_transformer_amd.ops import reference

from . import _parity as P
from ._parity import BF16, FP16
from ._ragged import LENS, make_model, make_prompts

pytestmark = pytest.mark.gpu

S_ALLOC = 305
# (1, 8, 9): only the new key; S-1 in the last split; S-1 in split 4 of 8 with
# three empty splits. (7, 300, 64): empty splits, a ragged tail chunk, even chunks.
LEN_TRIPLES = ((1, 8, 9), (7, 300, 64))

# test_ragged_decode_step_logits: measured floor and the bound derived from it
LOGIT_FLOOR = 0.0
LOGIT_BOUND = 2 * LOGIT_FLOOR


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


def _append_case(dev, dtype, B, H, D, lens, slopes, seed, items):
    """Run ops.attention_decode_append on NaN-tailed caches; queue the output
    parity items and assert the caches bit for bit. `lens` in [1, S_ALLOC]."""
    from zero_transformer_amd import ops

    C = H * D
    qkv = P.randn((B, 1, 3 * C), dtype, seed)
    k0 = P.randn((B, H, S_ALLOC, D), dtype, seed + 1)
    v0 = P.randn((B, H, S_ALLOC, D), dtype, seed + 2)
    for b, n in enumerate(lens):  # dead tail, and the row about to be written
        k0[b, :, n - 1:] = math.nan
        v0[b, :, n - 1:] = math.nan
    q, kn, vn = (t.view(B, H, D) for t in qkv.split(C, dim=-1))
    k_want, v_want = k0.clone(), v0.clone()
    for b, n in enumerate(lens):
        k_want[b, :, n - 1] = kn[b]
        v_want[b, :, n - 1] = vn[b]
    kd, vd = k0.to(dev), v0.to(dev)
    got = ops.attention_decode_append(
        qkv.to(dev), kd, vd, H, None if slopes is None else slopes.to(dev),
        torch.tensor(lens, dtype=torch.int32, device=dev))
    assert got.shape == (B, 1, C) and got.dtype == dtype
    got = got.cpu().view(B, H, 1, D)
    for b, n in enumerate(lens):
        want, a = P.attn_decode_ref(q[b].view(1, H, 1, D), k_want[b:b + 1],
                                    v_want[b:b + 1], slopes, n)
        tag = (f"attention_decode_append D={D} S={n} {str(dtype)[6:]} "
               f"alibi={slopes is not None}")
        items.append((tag, got[b:b + 1], want, a, dtype))
    assert torch.equal(_bits(kd), _bits(k_want)), f"k cache differs, lens={lens}"
    assert torch.equal(_bits(vd), _bits(v_want)), f"v cache differs, lens={lens}"


def _check(items):
    bad = []
    for name, got, want, a, dt in items:
        r = P.worst_ratio(got, want, dt, a)
        print(f"[parity] {name}: worst error/bound = {r:.3f}")
        if not r <= 1.0:
            bad.append(f"{name}: error is {r:.3f} x the bound")
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("dtype", [BF16, FP16])
@pytest.mark.parametrize("D", [32, 64, 96, 128, 192, 256])
def test_decode_append_kernel_edges(dev, D, dtype):
    B, H = 3, 3
    slopes = reference.alibi_slopes(H)
    items = []
    for i, lens in enumerate(LEN_TRIPLES):
        for sl in (slopes, None):
            _append_case(dev, dtype, B, H, D, lens, sl, 700 + 10 * i, items)
    _check(items)


def test_decode_append_empty_and_clamped_lengths(dev):
    """S == 0 writes nothing and returns zeros; a length above the allocation
    is clamped to it in-kernel (sequence 0, so that even an unclamped write
    would land inside the cache tensor)."""
    from zero_transformer_amd import ops

    B, H, D = 3, 3, 128
    C = H * D
    qkv = P.randn((B, 1, 3 * C), BF16, 900)
    k0 = P.randn((B, H, S_ALLOC, D), BF16, 901)
    v0 = P.randn((B, H, S_ALLOC, D), BF16, 902)
    q, kn, vn = (t.view(B, H, D) for t in qkv.split(C, dim=-1))
    lens = (S_ALLOC + 2, 0, 3)
    eff = (S_ALLOC, 0, 3)
    k_want, v_want = k0.clone(), v0.clone()
    for b, n in enumerate(eff):
        if n:
            k_want[b, :, n - 1] = kn[b]
            v_want[b, :, n - 1] = vn[b]
    slopes = reference.alibi_slopes(H)
    kd, vd = k0.to(dev), v0.to(dev)
    got = ops.attention_decode_append(
        qkv.to(dev), kd, vd, H, slopes.to(dev),
        torch.tensor(lens, dtype=torch.int32, device=dev)).cpu().view(B, H, 1, D)
    assert torch.equal(_bits(kd), _bits(k_want)) and torch.equal(_bits(vd), _bits(v_want))
    assert torch.count_nonzero(got[1]) == 0
    items = []
    for b in (0, 2):
        want, a = P.attn_decode_ref(q[b].view(1, H, 1, D), k_want[b:b + 1],
                                    v_want[b:b + 1], slopes, eff[b])
        items.append((f"attention_decode_append clamp S={lens[b]}", got[b:b + 1], want, a, BF16))
    _check(items)


def test_attention_decode_s_used_forms(dev):
    """A B-element s_used of equal values is the 1-element form, bit for bit."""
    from zero_transformer_amd import ops

    B, H, D, S = 3, 3, 128, 77
    q = P.randn((B, H, 1, D), BF16, 910).to(dev)
    k = P.randn((B, H, S + 5, D), BF16, 911).to(dev)
    v = P.randn((B, H, S + 5, D), BF16, 912).to(dev)
    sl = reference.alibi_slopes(H).to(dev)
    one = ops.attention_decode(q, k, v, sl, torch.tensor([S], dtype=torch.int32, device=dev))
    per = ops.attention_decode(q, k, v, sl, torch.full((B,), S, dtype=torch.int32, device=dev))
    assert torch.equal(one, per)
    with pytest.raises(RuntimeError):
        ops.attention_decode(q, k, v, sl, torch.full((2,), S, dtype=torch.int32, device=dev))


@pytest.fixture(scope="module")
def lively(dev):
    return make_model().to(dev).to(torch.bfloat16)


def test_generate_batch_graph_matches_eager(dev, lively):
    from zero_transformer_amd.models.inference import generate_batch

    prompts = make_prompts(LENS)
    eager = generate_batch(lively, prompts, 8, use_graph=False)
    graph = generate_batch(lively, prompts, 8, use_graph=True)
    assert [len(r) for r in eager] == [8, 8, 8]
    assert graph == eager, "graph replay diverged from eager ragged decode"


def test_generate_batch_uniform_equals_generate_fast(dev, lively):
    from zero_transformer_amd.models.inference import generate_batch, generate_fast

    prompts = make_prompts((12, 12, 12))
    idx = torch.tensor(prompts, device=dev)
    want = generate_fast(lively, idx, 8)[:, 12:].tolist()
    assert generate_batch(lively, prompts, 8) == want


def test_one_token_prompt_equals_dynamic_cache_path(dev, lively):
    """A one-token prompt prefills through the decode step (cache length set
    first, K/V row 0 appended by the kernel): generate_fast and
    generate_stream, with and without the graph, and generate_batch must give
    the dynamic-cache path's greedy tokens."""
    from zero_transformer_amd.models.inference import generate_batch, generate_fast
    from zero_transformer_amd.models.sampling import generate_stream

    n = 8
    idx = torch.tensor([[17]], device=dev)
    with torch.no_grad():
        logits, past = lively(idx, use_cache=True)
        want = []
        for _ in range(n):
            nxt = logits[:, -1:].argmax(-1)
            want.append(int(nxt))
            logits, past = lively(nxt, use_cache=True, past_states=past)
    assert len(set(want)) > 1, "model only echoes"
    for g in (False, True):
        assert generate_fast(lively, idx, n, use_graph=g)[0, 1:].tolist() == want
        got = list(generate_stream(lively, idx, max_new_tokens=n, sample=False,
                                   repetition_penalty=1.0, use_graph=g))
        assert got == want
    assert generate_batch(lively, [[17]], n) == [want]


def test_ragged_decode_step_logits(dev):
    """One ragged static-cache decode step (B=3, lengths 5/12/9) against each
    sequence alone through the dynamic-cache path at B=1 (prefill, one step).

    The bound is 2x a floor measured on the MI355X at the parent commit (all
    parent code): max |static-cache B=3 uniform decode logits - dynamic-cache
    B=1 logits| over these prompts cut to length 5. That floor came out as
    exactly 0.0 (logit std 19.5): at C = 256 the projections are below the
    GEMV kernel's K % 512 gate, so B=1 and B=3 both run hipBLASLt, whose rows
    did not depend on the batch or on the padded prefill shape. LOGIT_FLOOR =
    0.0, LOGIT_BOUND = 0.0: the test asserts bit equality. The ragged step
    measured max diff 0.0 against it (logit std 19.1); a wrong length or a
    misplaced row moves the logits by their own magnitude.

    Reading a failure: bit equality between hipBLASLt runs at B=1 and B=3
    with different padded prefill shapes also breaks when a hipBLASLt
    heuristic or tuning change makes its rows depend on the GEMM shape. A
    diff of a bf16 ulp or two (~0.1-0.25 here) points there, and the floor
    wants re-measuring at the then parent; a diff of the logits' own
    magnitude points at the decode path.
    """
    from zero_transformer_amd.models.inference import StaticKVCache

    model = make_model(lively=False).to(dev).to(torch.bfloat16)
    prompts = make_prompts(LENS)
    B = len(prompts)
    attn = model.blocks[0].attn
    with torch.no_grad():
        alone, nxt = [], []
        for pr in prompts:
            lg, past = model(torch.tensor([pr], device=dev), use_cache=True)
            t = lg[:, -1:].argmax(-1)
            step, _ = model(t, use_cache=True, past_states=past)
            alone.append(step[0, 0].float())
            nxt.append(t[0])
        idx = torch.zeros(B, max(LENS), dtype=torch.long, device=dev)
        for b, pr in enumerate(prompts):
            idx[b, : len(pr)] = torch.tensor(pr, device=dev)
        cache = StaticKVCache(model.N, B, attn.num_head, attn.head_dim, 32, dev,
                              torch.bfloat16)
        model(idx, static_cache=cache)
        cache.set_len(list(LENS))
        cache.advance(1)
        ragged = model(torch.stack(nxt), static_cache=cache)[:, 0].float()
    alone = torch.stack(alone)
    diff = float((ragged - alone).abs().max())
    std = float(alone.std())
    print(f"[ragged] decode-step logits: max diff {diff:.4f}, bound {LOGIT_BOUND}, "
          f"logit std {std:.2f}")
    assert LOGIT_BOUND <= 0.1 * std, "bound too loose to show anything"
    assert diff <= LOGIT_BOUND
