"""Prefill on CPU: the fp32 reference op (ops.attention_prefill_append routes
CPU tensors to reference.attention_prefill_append), GPT2.prefill with
per-sequence lengths and chunking, and generate_batch's prefill_chunk.

The GPU runs the same Python with the HIP kernel pair in the reference op's
place (tests/test_gpu_prefill.py).
"""

from __future__ import annotations

import math

import pytest
import torch

from zero_transformer_amd import ops
from zero_transformer_amd.models.inference import StaticKVCache, generate_batch
from zero_transformer_amd.ops import reference

from . import _parity as P
from . import _prefill as PF
from ._ragged import LENS, make_model, make_prompts

REL_FP32 = 1e-5  # relative fp32 bound on reference-vs-reference comparisons


def _bits(t):
    return t.contiguous().view(torch.int32)


def _close(got, want, name):
    err = float((got - want).abs().max())
    lim = REL_FP32 * float(want.abs().max())
    print(f"[prefill] {name}: max err {err:.3e}, bound {lim:.3e}")
    assert err <= lim, f"{name}: {err} > {lim}"


def _inputs(B, H, D, T, S_alloc, seed):
    C = H * D
    qkv = P.randn((B, T, 3 * C), P.FP32, seed)
    k0 = P.randn((B, H, S_alloc, D), P.FP32, seed + 1)
    v0 = P.randn((B, H, S_alloc, D), P.FP32, seed + 2)
    return qkv, k0, v0


@pytest.mark.parametrize("alibi", [True, False])
def test_reference_prefill_full_equals_reference_attention(alibi):
    B, H, D, T, S_alloc = 2, 4, 16, 37, 40
    C = H * D
    sl = reference.alibi_slopes(H) if alibi else None
    qkv, k0, v0 = _inputs(B, H, D, T, S_alloc, 21)
    q, k, v = (t.view(B, T, H, D).transpose(1, 2) for t in qkv.split(C, dim=-1))
    want = reference.attention(q, k, v, sl).transpose(1, 2).reshape(B, T, C)
    kc, vc = k0.clone(), v0.clone()
    got = ops.attention_prefill_append(
        qkv, kc, vc, H, sl, torch.full((B,), T, dtype=torch.int32),
        torch.zeros(B, dtype=torch.int32))
    assert got.shape == (B, T, C) and got.dtype == P.FP32
    _close(got, want, f"full prefill vs attention alibi={alibi}")
    assert torch.equal(_bits(kc[:, :, :T]), _bits(k.contiguous()))
    assert torch.equal(_bits(vc[:, :, :T]), _bits(v.contiguous()))
    assert torch.equal(_bits(kc[:, :, T:]), _bits(k0[:, :, T:]))
    assert torch.equal(_bits(vc[:, :, T:]), _bits(v0[:, :, T:]))
    # None means the same thing
    kn, vn = k0.clone(), v0.clone()
    assert torch.equal(got, ops.attention_prefill_append(qkv, kn, vn, H, sl))
    assert torch.equal(_bits(kn), _bits(kc)) and torch.equal(_bits(vn), _bits(vc))


def test_reference_prefill_two_call_split_equals_one_call():
    B, H, D, T, S_alloc = 2, 4, 16, 29, 32
    sl = reference.alibi_slopes(H)
    qkv, k0, v0 = _inputs(B, H, D, T, S_alloc, 31)
    k1, v1 = k0.clone(), v0.clone()
    one = reference.attention_prefill_append(qkv, k1, v1, H, sl)
    for a in (1, 13, 28):
        k2, v2 = k0.clone(), v0.clone()
        i32 = lambda x: torch.full((B,), x, dtype=torch.int32)
        first = reference.attention_prefill_append(
            qkv[:, :a].contiguous(), k2, v2, H, sl, i32(a), i32(0))
        rest = reference.attention_prefill_append(
            qkv[:, a:].contiguous(), k2, v2, H, sl, i32(T - a), i32(a))
        _close(torch.cat([first, rest], dim=1), one, f"split at {a}")
        assert torch.equal(_bits(k2), _bits(k1)) and torch.equal(_bits(v2), _bits(v1))


def test_reference_prefill_clamps_and_untouched_rows():
    """lens > T clamps to T; start + lens > S_alloc clamps n to
    S_alloc - start; lens = 0 leaves the cache alone and returns zero rows.
    Pad rows of qkv and dead cache rows are NaN: they stay NaN in the caches
    and reach no live output row."""
    B, H, D, T, S_alloc = 4, 2, 16, 10, 24
    C = H * D
    sl = reference.alibi_slopes(H)
    qkv, k0, v0 = _inputs(B, H, D, T, S_alloc, 41)
    lens = (T + 5, 9, 0, 4)
    start = (0, S_alloc - 3, 7, S_alloc + 2)
    ranges = PF.clamp_range(lens, start, T, S_alloc)
    assert ranges == [(0, T), (S_alloc - 3, 3), (7, 0), (S_alloc, 0)]
    for b, (st, n) in enumerate(ranges):
        qkv[b, n:] = math.nan
        k0[b, :, st:] = math.nan
        v0[b, :, st:] = math.nan
    k_want, v_want = PF.expected_caches(qkv, k0, v0, H, ranges)
    kc, vc = k0.clone(), v0.clone()
    got = ops.attention_prefill_append(
        qkv, kc, vc, H, sl, torch.tensor(lens, dtype=torch.int32),
        torch.tensor(start, dtype=torch.int32))
    assert torch.equal(_bits(kc), _bits(k_want)) and torch.equal(_bits(vc), _bits(v_want))
    assert torch.isnan(kc[0, :, T:]).all() and torch.isnan(kc[2, :, 7:]).all()
    ref = PF.prefill_ref(qkv, k_want, v_want, H, sl, ranges, P.FP32)
    for b, (st, n) in enumerate(ranges):
        assert torch.count_nonzero(got[b, n:]) == 0, f"rows >= n of sequence {b}"
        assert torch.isfinite(got[b]).all()
        if n:
            P.assert_within(got[b, :n], ref[b][0], P.FP32, ref[b][1],
                            f"prefill_ref b={b} st={st} n={n}")


def _padded(prompts):
    idx = torch.zeros(len(prompts), max(len(p) for p in prompts), dtype=torch.long)
    for b, pr in enumerate(prompts):
        idx[b, : len(pr)] = torch.tensor(pr)
    return idx


@pytest.fixture(scope="module")
def model():
    return make_model()


@pytest.fixture(scope="module")
def alone_last(model):
    """Each prompt alone through the no-cache forward: its last-row logits."""
    with torch.no_grad():
        return torch.stack([model(torch.tensor([pr]))[0, -1] for pr in make_prompts(LENS)])


@pytest.mark.parametrize("chunk", [None, 4, 5])
def test_model_prefill_matches_each_sequence_alone(model, alone_last, chunk):
    """Bound 1e-4 * max|logit|: the ACC factor of tests/_parity.py over
    roughly ten chained fp32 ops. chunk=5 ends exactly on a prompt's end."""
    prompts = make_prompts(LENS)
    attn = model.blocks[0].attn
    cache = StaticKVCache(model.N, len(prompts), attn.num_head, attn.head_dim, 32,
                          "cpu", torch.float32)
    for k, v in zip(cache.k, cache.v):  # a pad row written anywhere would show
        k.fill_(math.nan)
        v.fill_(math.nan)
    got = model.prefill(_padded(prompts), cache, torch.tensor(LENS), chunk=chunk)
    assert got.shape == alone_last.shape
    err = float((got - alone_last).abs().max())
    lim = 1e-4 * float(alone_last.abs().max())
    print(f"[prefill] model.prefill chunk={chunk}: max err {err:.3e}, bound {lim:.3e}")
    assert err <= lim
    for b, n in enumerate(LENS):
        for t in cache.k + cache.v:
            assert torch.isfinite(t[b, :, :n]).all() and torch.isnan(t[b, :, n:]).all()
    assert cache.len_t.tolist() == [0, 0, 0]  # left to the caller


def test_generate_batch_prefill_chunk_gives_the_same_tokens(model):
    # the lively model's greedy top-2 gaps are >= 0.1 (tests/_ragged.py)
    prompts = make_prompts(LENS)
    want = generate_batch(model, prompts, 6)
    assert [len(r) for r in want] == [6, 6, 6]
    assert generate_batch(model, prompts, 6, prefill_chunk=4) == want
