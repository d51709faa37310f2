"""Speculative verify on the GPU: the split-S kernels of
ops/csrc/attn_verify.hip against the float64 prefill reference of
tests/_prefill.py (the op has the prefill op's rounding points, so its bound
is used as it is), GPT2.verify and generate_speculative on top of them."""

from __future__ import annotations

import copy
import math

import pytest
import torch

from zero_transformer_amd.ops import reference

from . import _paged as PG
from . import _parity as P
from . import _prefill as PF
from ._parity import BF16, FP16
from ._ragged import LENS, VOCAB, make_model, make_prompts

pytestmark = pytest.mark.gpu

B, H, S_ALLOC = 3, 3, 2112  # 33 pages of 64 rows, 11 of 192
# (T, lens, start, alibi, page rows). The kernel cuts keys [0, start + n) into
# 32-key tiles, 8 contiguous chunks of them, 4 waves per chunk:
#   start 0: only the causal triangle, and 1 or 7 keys leave 7 chunks empty;
#   2040 keys are 64 tiles, so every wave loops twice (1000: once); lens 0 and
#     lens < T; 254 + 3 crosses a chunk, tile and page boundary at 256;
#   start + n == S_alloc, and 63 + 2 across the first page boundary;
#   one row; pages of 192 rows with rows on both sides of 192 and 384.
CASES = (
    (16, (16, 7, 1), (0, 0, 0), True, 64),
    (5, (5, 0, 3), (2040, 40, 254), True, 64),
    (5, (2, 5, 4), (1000, 31, 60), False, 64),
    (2, (2, 1, 2), (S_ALLOC - 2, S_ALLOC - 1, 63), True, 64),
    (1, (1, 1, 0), (0, 191, 5), False, 64),
    (5, (5, 5, 2), (190, 382, 575), True, 192),
)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _i32(x, dev):
    return torch.tensor(x, dtype=torch.int32, device=dev)


@pytest.mark.parametrize("dtype", [BF16, FP16])
@pytest.mark.parametrize("D", [32, 64, 96, 128])
def test_verify_kernel_edges(dev, D, dtype):
    """Both ops on every case: caches bit for bit, dead rows zero, live rows
    within the prefill bound (ratio <= 1; merging the splits adds fp32 terms of
    relative size 2^-23, which the bound's ACC = 1e-5 term already holds), and
    the paged result bit-identical to the contiguous one."""
    from zero_transformer_amd import ops

    C, bad = H * D, []
    for i, (T, lens, start, alibi, R) in enumerate(CASES):
        seed = 3100 + 10 * i
        slopes = reference.alibi_slopes(H) if alibi else None
        sl = None if slopes is None else slopes.to(dev)
        qkv = P.randn((B, T, 3 * C), dtype, seed)
        k0 = P.randn((B, H, S_ALLOC, D), dtype, seed + 1)
        v0 = P.randn((B, H, S_ALLOC, D), dtype, seed + 2)
        ranges = PF.clamp_range(lens, start, T, S_ALLOC)
        for b, (st, n) in enumerate(ranges):
            qkv[b, n:] = math.nan
            k0[b, :, st:] = math.nan
            v0[b, :, st:] = math.nan
        k_want, v_want = PF.expected_caches(qkv, k0, v0, H, ranges)
        ref = PF.prefill_ref(qkv, k_want, v_want, H, slopes, ranges, dtype)

        kd, vd = k0.to(dev), v0.to(dev)
        got = ops.attention_verify_append(
            qkv.to(dev), kd, vd, H, sl, _i32(lens, dev), _i32(start, dev)).cpu()
        M, pages = S_ALLOC // R, B * (S_ALLOC // R) + 1
        bt = PG.make_table(B, M, pages, seed + 3)
        kp = PG.scatter(torch.full((pages, H, R, D), math.nan, dtype=dtype), bt, k0).to(dev)
        vp = PG.scatter(torch.full((pages, H, R, D), math.nan, dtype=dtype), bt, v0).to(dev)
        paged = ops.attention_verify_paged(
            qkv.to(dev), kp, vp, H, sl, bt.to(dev), _i32(lens, dev), _i32(start, dev)).cpu()

        tag = f"verify D={D} {str(dtype)[6:]} T={T} lens={lens} start={start} R={R}"
        assert got.shape == (B, T, C) and got.dtype == dtype
        assert torch.equal(PG.bits(kd), PG.bits(k_want)), f"k cache differs: {tag}"
        assert torch.equal(PG.bits(vd), PG.bits(v_want)), f"v cache differs: {tag}"
        assert torch.equal(PG.bits(PG.gather(kp.cpu(), bt)), PG.bits(k_want)), f"k pool: {tag}"
        assert torch.equal(PG.bits(PG.gather(vp.cpu(), bt)), PG.bits(v_want)), f"v pool: {tag}"
        assert torch.equal(PG.bits(paged), PG.bits(got)), f"paged != contiguous: {tag}"
        for b, (st, n) in enumerate(ranges):
            assert torch.count_nonzero(got[b, n:]) == 0, f"rows >= n not zero, b={b}: {tag}"
            if n:
                r = P.worst_ratio(got[b, :n], ref[b][0], dtype, ref[b][1])
                print(f"[parity] {tag} b={b}: worst error/bound = {r:.3f}")
                if not r <= 1.0:
                    bad.append(f"{tag} b={b}: error is {r:.3f} x the bound")
    assert not bad, "; ".join(bad)


def test_model_verify_logits(dev):
    """GPT2.verify (fp16 lively model, prompts of 5 / 12 / 9 cached, T = 5 rows
    of which 5 / 3 / 1 are live) against the fp32 CPU forward of the same
    weights and tokens, next to the parent's way to the same logits: T decode
    steps on a clone of the cache. verify may be further from the CPU forward
    than the sequential path by the fp16 logit floor recorded in
    tests/test_gpu_prefill.py (2 x 0.003932 = 0.0079), no more."""
    from zero_transformer_amd.models.inference import StaticKVCache

    T, live = 5, (5, 3, 1)
    model = make_model().to(dev).to(FP16)
    prompts = make_prompts(LENS)
    g = torch.Generator().manual_seed(77)
    new = torch.randint(1, VOCAB, (len(prompts), T), generator=g)
    m32 = copy.deepcopy(model).to("cpu").float()
    for blk in m32.blocks:
        blk.attn._qkv_w = None
    with torch.no_grad():
        want = [m32(torch.tensor([pr + new[b, :n].tolist()]))[0, -n:]
                for b, (pr, n) in enumerate(zip(prompts, live))]

    attn = model.blocks[0].attn
    cache = StaticKVCache(model.N, len(prompts), attn.num_head, attn.head_dim, 32, dev, FP16)
    idx = torch.zeros(len(prompts), max(LENS), dtype=torch.long)
    for b, pr in enumerate(prompts):
        idx[b, :len(pr)] = torch.tensor(pr)
    model.prefill(idx.to(dev), cache, torch.tensor(LENS))
    seq_cache = copy.deepcopy(cache)
    got = model.verify(new.to(dev), cache, _i32(live, dev), _i32(LENS, dev)).float().cpu()
    seq = []
    for i in range(T):
        seq_cache.set_len([n + i + 1 for n in LENS])
        seq.append(model(new[:, i:i + 1].to(dev), static_cache=seq_cache)[:, 0])
    seq = torch.stack(seq, 1).float().cpu()
    err_v = max(float((got[b, :n] - want[b]).abs().max()) for b, n in enumerate(live))
    err_s = max(float((seq[b, :n] - want[b]).abs().max()) for b, n in enumerate(live))
    print(f"[verify] max logit error: verify {err_v:.5f}, sequential decode {err_s:.5f}")
    assert err_v <= err_s + 0.0079


@pytest.fixture(scope="module")
def greedy(dev):
    """fp16 model and, for scenario prompts 0 / 6 / 8 (5, 70 and 130 tokens),
    generate_fast's tokens for the scenario's own counts (10 / 9 / 3), over
    which its top-2 gap is >= 0.05 (tests/_paged.MIN_GAP)."""
    from zero_transformer_amd.models.inference import generate_fast

    model = make_model(num_ctx=192).to(dev).to(FP16)
    prompts, counts = PG.scenario()
    runs = []
    for i in (0, 6, 8):
        idx = torch.tensor([prompts[i]], device=dev)
        runs.append((idx, counts[i], generate_fast(model, idx, counts[i])))
    return model, runs


def _draft(kind, ref, K):
    """Row 0 (and every row of 'oracle') is proposed the known continuation;
    row 1 of 'mixed' and every row of 'wrong' a first token that is not it."""
    def fn(tokens):
        out = []
        for b, t in enumerate(tokens):
            nxt = ref[len(t):len(t) + K]
            right = kind == "oracle" or (kind == "mixed" and b == 0)
            out.append(nxt if right else [(x + 1) % VOCAB for x in nxt])
        return out
    return None if kind == "lookup" else fn


@pytest.mark.parametrize("kind", ["oracle", "wrong", "lookup", "mixed"])
def test_generate_speculative_equals_generate_fast(greedy, kind):
    from zero_transformer_amd.models.inference import generate_speculative

    model, runs = greedy
    K = 4
    for idx, n, want in runs:
        Bn = 2 if kind == "mixed" else 1
        fn = _draft(kind, want[0].tolist(), K)
        res = [generate_speculative(model, idx.repeat(Bn, 1), n, draft_len=K,
                                    use_graph=ug, draft_fn=fn) for ug in (True, False)]
        for toks, steps, accepted in res:
            assert torch.equal(toks, want.repeat(Bn, 1)), f"{kind}, prompt of {idx.shape[1]}"
        assert res[0][1:] == res[1][1:]
        steps, accepted = res[0][1:]
        print(f"[spec] {kind} prompt {idx.shape[1]} new {n}: {steps} steps, {accepted} accepted")
        if kind == "oracle":
            assert steps == -(-n // (K + 1)) and accepted == n - steps
        if kind == "wrong":
            assert steps == n and accepted == 0
        if kind == "mixed":
            assert steps == n and accepted == n - -(-n // (K + 1))
