"""Ragged batched decode on CPU: per-sequence KV lengths through the fp32
reference op, StaticKVCache, generate_batch and the batched sampler.

Everything here runs without a GPU: ops.attention_decode_append routes CPU
tensors to reference.attention_decode_append, so the static-cache decode path
is the same Python the GPU runs, with the reference op in the kernel's place.
The yardstick for the model-level tests is each sequence ALONE through the
no-cache forward (model(seq) / model.generate).
"""

from __future__ import annotations

import math

import pytest
import torch

from zero_transformer_amd import ops
from zero_transformer_amd.models import sampling
from zero_transformer_amd.models.inference import StaticKVCache, generate_batch
from zero_transformer_amd.ops import reference

from . import _parity as P
from ._ragged import LENS, SEED, VOCAB, make_model as _model, make_prompts as _prompts

N_NEW = 6
MIN_GAP = 1e-2  # reference top-2 logit gap that makes token equality meaningful


def _greedy_ref(model, prompts, n_new):
    """Per prompt: model.generate's greedy tokens (n_new: one count per
    prompt); asserts the top-2 logit gap of the no-cache forward at every
    one of those steps."""
    refs = []
    with torch.no_grad():
        for pr, n in zip(prompts, n_new):
            full = model.generate(torch.tensor([pr]), n)
            logits = model(full[:, :-1])[0, len(pr) - 1:]  # the n deciding rows
            top2 = logits.float().topk(2, dim=-1).values
            gap = float((top2[:, 0] - top2[:, 1]).min())
            print(f"[ragged] prompt len {len(pr)}: min top-2 gap {gap:.4f}")
            assert gap > MIN_GAP, f"seed gives a top-2 gap of {gap}: pick another"
            refs.append(full[0, len(pr):].tolist())
    return refs


@pytest.fixture(scope="module")
def model():
    return _model()


@pytest.fixture(scope="module")
def greedy_ref(model):
    return _greedy_ref(model, _prompts(LENS), (N_NEW,) * len(LENS))


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_reference_decode_append_matches_per_sequence_ref():
    B, H, D, S_alloc = 3, 4, 64, 16
    C = H * D
    slopes = reference.alibi_slopes(H)
    qkv = P.randn((B, 1, 3 * C), P.FP32, 11)
    k0 = P.randn((B, H, S_alloc, D), P.FP32, 12)
    v0 = P.randn((B, H, S_alloc, D), P.FP32, 13)
    for b, n in enumerate(LENS):  # dead tail, and the row about to be written
        k0[b, :, n - 1:] = math.nan
        v0[b, :, n - 1:] = math.nan
    lens = torch.tensor(LENS, dtype=torch.int32)
    for sl in (slopes, None):
        k, v = k0.clone(), v0.clone()
        got = reference.attention_decode_append(qkv, k, v, H, sl, lens)
        assert got.shape == (B, 1, C) and got.dtype == P.FP32
        k_want, v_want = k0.clone(), v0.clone()
        q, kn, vn = (t.view(B, H, D) for t in qkv.split(C, dim=-1))
        for b, n in enumerate(LENS):
            k_want[b, :, n - 1] = kn[b]
            v_want[b, :, n - 1] = vn[b]
            assert torch.equal(k[b, :, n - 1], kn[b]) and torch.equal(v[b, :, n - 1], vn[b])
            want, a = P.attn_decode_ref(q[b].view(1, H, 1, D), k_want[b:b + 1],
                                        v_want[b:b + 1], sl, n)
            P.assert_within(got[b].view(1, H, 1, D), want, P.FP32, a,
                            f"decode_append_ref b={b} S={n} alibi={sl is not None}")
        # every other row unchanged (NaN tails compared as bit patterns)
        assert torch.equal(_bits(k), _bits(k_want))
        assert torch.equal(_bits(v), _bits(v_want))
    # the ops layer routes CPU tensors here
    k, v = k0.clone(), v0.clone()
    again = ops.attention_decode_append(qkv, k, v, H, slopes, lens)
    k2, v2 = k0.clone(), v0.clone()
    assert torch.equal(again, reference.attention_decode_append(qkv, k2, v2, H, slopes, lens))


def test_teacher_forced_ragged_decode_matches_each_sequence_alone(model):
    prompts = _prompts(LENS)
    B, steps = len(prompts), 4
    g = torch.Generator().manual_seed(SEED + 2)
    forced = torch.randint(1, VOCAB, (B, steps), generator=g)
    idx = torch.zeros(B, max(LENS), dtype=torch.long)
    for b, pr in enumerate(prompts):
        idx[b, : len(pr)] = torch.tensor(pr)
    attn = model.blocks[0].attn
    cache = StaticKVCache(model.N, B, attn.num_head, attn.head_dim, 32, "cpu",
                          torch.float32)
    with torch.no_grad():
        logits = model(idx, static_cache=cache)
        cache.set_len(list(LENS))
        seqs = [list(pr) for pr in prompts]
        for b in range(B):  # right-padded prefill is exact for the real rows
            alone = model(torch.tensor([seqs[b]]))[0, -1]
            torch.testing.assert_close(logits[b, LENS[b] - 1], alone, atol=1e-3, rtol=1e-3)
        for s in range(steps):
            cache.advance(1)
            logits = model(forced[:, s:s + 1], static_cache=cache)
            assert logits.shape == (B, 1, VOCAB)
            for b in range(B):
                seqs[b].append(int(forced[b, s]))
                alone = model(torch.tensor([seqs[b]]))[0, -1]
                torch.testing.assert_close(logits[b, 0], alone, atol=1e-3, rtol=1e-3)
    assert cache.len_t.tolist() == [n + steps for n in LENS]


def test_generate_batch_greedy_equals_per_prompt_generate(model, greedy_ref):
    assert len({t for r in greedy_ref for t in r}) > len(LENS), "model only echoes"
    got = generate_batch(model, _prompts(LENS), N_NEW)
    assert got == greedy_ref


def test_generate_batch_eos_cuts_each_row(model, greedy_ref):
    eos = greedy_ref[1][3]
    assert eos not in greedy_ref[1][:3], "seed: eos must first appear at step 3"
    got = generate_batch(model, _prompts(LENS), N_NEW, eos_token=eos)
    assert got[1] == greedy_ref[1][:3]
    for b, ref in enumerate(greedy_ref):
        cut = ref[: ref.index(eos)] if eos in ref else ref
        assert got[b] == cut


def test_generate_batch_sampling_options_per_row(model, greedy_ref):
    """The sampling branch, made deterministic: top_k=1 leaves one candidate,
    so it must reproduce greedy; and a row's repetition penalty must see its
    own prompt and tokens only, i.e. give what the row gets in a batch of one."""
    prompts = _prompts(LENS)
    torch.manual_seed(SEED)
    got = generate_batch(model, prompts, N_NEW, sample=True, top_k=1,
                         temperature=0.7, top_p=0.9)
    assert got == greedy_ref
    pen = generate_batch(model, prompts, N_NEW, repetition_penalty=1.5)
    assert pen != greedy_ref, "penalty changed nothing: the check below is empty"
    for pr, row in zip(prompts, pen):
        assert generate_batch(model, [pr], N_NEW, repetition_penalty=1.5) == [row]


def test_one_token_prompts_prefill_through_the_decode_step(model):
    """A one-token prompt takes the T == 1 static-cache branch for its
    prefill: the cache length must be set before it, or row 0 is never
    written. generate_fast and generate_batch against model.generate."""
    from zero_transformer_amd.models.inference import generate_fast

    idx = torch.tensor([[17], [301]])
    refs = _greedy_ref(model, idx.tolist(), (N_NEW, N_NEW))
    assert generate_fast(model, idx, N_NEW)[:, 1:].tolist() == refs
    assert generate_batch(model, idx.tolist(), N_NEW) == refs


def test_generate_batch_context_cap_per_sequence():
    m = _model(num_ctx=16)
    lens = (5, 12)
    prompts = _prompts(lens)
    refs = _greedy_ref(m, prompts, (8, 4))
    got = generate_batch(m, prompts, 8)
    assert [len(r) for r in got] == [8, 4]
    assert got == refs


def test_batched_repetition_penalty_and_cache_lengths():
    B, V = 3, 40
    logits = P.randn((B, V), P.FP32, 21, scale=3.0)
    g = torch.Generator().manual_seed(SEED + 3)
    history = [torch.randint(0, V, (n,), generator=g).tolist() for n in (0, 7, 30)]
    seen = torch.zeros(B, V, dtype=torch.bool)
    for b, h in enumerate(history):
        if h:
            seen[b].scatter_(0, torch.tensor(h), True)
    for penalty in (1.0, 1.3, 0.8):
        got = sampling.apply_repetition_penalty_batched(logits.clone(), seen, penalty)
        for b, h in enumerate(history):
            want = sampling.apply_repetition_penalty(logits[b:b + 1].clone(), h, penalty)
            assert torch.equal(got[b:b + 1], want)
    # greedy batched sampling = per-row argmax of the penalised logits
    nxt = sampling.sample_batch(logits, seen, 1.0, 0, 1.0, 1.3, False)
    want = sampling.apply_repetition_penalty_batched(logits, seen, 1.3).argmax(-1)
    assert nxt.dtype == torch.long and torch.equal(nxt, want)

    cache = StaticKVCache(1, B, 2, 8, 16, "cpu", torch.float32)
    assert cache.len_t.shape == (B,) and cache.len_t.dtype == torch.int32
    cache.set_len(4)
    assert cache.len_t.tolist() == [4, 4, 4]
    cache.advance()
    assert cache.len_t.tolist() == [5, 5, 5]
    cache.set_len([5, 12, 9])
    assert cache.len_t.tolist() == [5, 12, 9]
    cache.set_len(torch.tensor([1, 2, 3]))
    cache.advance(torch.tensor([1, 0, 1], dtype=torch.int32))
    cache.advance(2)
    assert cache.len_t.tolist() == [4, 4, 6] and cache.len_t.dtype == torch.int32
