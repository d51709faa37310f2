"""Native int8 verify attention (ops/csrc/attn_verify_kv8.hip): the op against
the float64 prefill reference of tests/_prefill.py over the exact dequantized
K and the 16-bit V the kernel forms, its independence of the paging, and
GPT2.verify on a PagedKVCacheQ8."""

from __future__ import annotations

import copy
import math

import pytest
import torch

from zero_transformer_amd import ops
from zero_transformer_amd.ops import reference

from . import _paged as PG
from . import _parity as P
from . import _prefill as PF
from ._parity import BF16, FP16
from ._ragged import LENS, VOCAB, make_model, make_prompts
from .test_gpu_kv8 import _blank_pools, _same
from .test_gpu_verify import B, CASES, H, S_ALLOC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _i32(x, dev):
    return torch.tensor(x, dtype=torch.int32, device=dev)


def _run(dev, D, dtype, case, Rn, Mn, table_seed, check):
    """CASES[case] through the op under one layout (pages of Rn rows, Mn table
    entries, Mn * Rn >= S_ALLOC); the logical rows do not depend on the
    layout. -> (o (B, T, C) on the CPU, worst ratios of the live sequences)."""
    T, lens, start, alibi, _ = CASES[case]
    C, cap, seed = H * D, Mn * Rn, 3500 + 10 * case
    slopes = reference.alibi_slopes(H) if alibi else None
    ranges = PF.clamp_range(lens, start, T, cap)
    qkv = P.randn((B, T, 3 * C), dtype, seed)
    for b, (st, n) in enumerate(ranges):
        qkv[b, n:] = math.nan
    logical = []
    for i in range(2):  # cached rows [0, st); a byte / NaN where nothing is cached
        u, s = reference.quantize_kv_rows(P.randn((B, H, S_ALLOC, D), dtype, seed + 1 + i))
        uu = torch.full((B, H, cap, D), 7, dtype=torch.uint8)
        ss = torch.full((B, H, cap), math.nan)
        for b, (st, n) in enumerate(ranges):
            uu[b, :, :st], ss[b, :, :st] = u[b, :, :st], s[b, :, :st]
        logical += [uu, ss.unsqueeze(-1)]
    pages = B * Mn + 1
    bt = PG.make_table(B, Mn, pages, table_seed)
    blank = _blank_pools(pages, H, Rn, D)
    pools = [PG.scatter(blank[0], bt, logical[0]), PG.scatter(blank[1], bt, logical[2]),
             PG.scatter(blank[2].unsqueeze(-1), bt, logical[1]).squeeze(-1),
             PG.scatter(blank[3].unsqueeze(-1), bt, logical[3]).squeeze(-1)]
    got, got_qkv = [t.to(dev) for t in pools], qkv.to(dev)
    out = ops.attention_verify_paged_q8(
        got_qkv, *got, H, None if slopes is None else slopes.to(dev), bt.to(dev),
        _i32(lens, dev), _i32(start, dev)).cpu()
    assert out.shape == (B, T, C) and out.dtype == dtype
    if not check:
        return out, []
    tag = f"verify_q8 D={D} {str(dtype)[6:]} T={T} lens={lens} start={start} R={Rn}"
    reference.kv8_quantize_paged(qkv, *pools, bt, _i32(lens, "cpu"), _i32(start, "cpu"))
    _same(got, pools, tag)  # the new rows' codes and scales, and nothing else
    assert torch.equal(PG.bits(got_qkv), PG.bits(qkv)), f"qkv differs: {tag}"
    kc, vc = (PG.gather(t, bt) for t in pools[:2])
    ks, vs = (PG.gather(t.unsqueeze(-1), bt) for t in pools[2:])
    kf = (kc.double() - 128.0) * ks.double()
    vf = reference.dequantize_kv_rows(vc, vs.squeeze(-1), dtype)
    ref = PF.prefill_ref(qkv, kf, vf, H, slopes, ranges, dtype)
    ratios = []
    for b, (st, n) in enumerate(ranges):
        assert torch.count_nonzero(out[b, n:]) == 0, f"rows >= n not zero, b={b}: {tag}"
        if n:
            ratios.append(P.worst_ratio(out[b, :n], ref[b][0], dtype, ref[b][1]))
            print(f"[parity] {tag} b={b}: worst error/bound = {ratios[-1]:.3f}")
    return out, ratios


@pytest.mark.parametrize("dtype", [BF16, FP16])
@pytest.mark.parametrize("D", [32, 64, 96, 128])
def test_verify_q8_kernel_edges(dev, D, dtype):
    """Every case of tests/test_gpu_verify.py: pools and qkv bit for bit those
    of reference.kv8_quantize_paged, dead rows zero, live rows within the
    prefill bound over K = (u - 128) * scale in float64 and V = the 16-bit
    dequantize_kv_rows, the kernel's operand: ratio <= 1 with no extra term
    (K enters the kernel as exact codes; its scale multiplies the fp32 score,
    one more fp32 rounding, which ACC holds)."""
    bad = []
    for case, (T, lens, start, _, R) in enumerate(CASES):
        _, ratios = _run(dev, D, dtype, case, R, S_ALLOC // R, 3503 + 10 * case, True)
        bad += [f"case {case} (T={T} lens={lens} start={start}): {r:.3f} x the bound"
                for r in ratios if not r <= 1.0]
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("D,dtype", [(128, FP16), (96, BF16)])
def test_verify_q8_layout_independent(dev, D, dtype):
    """Case 1 (ALiBi on, 2045 / 40 / 257 keys) under another table, under pages
    of 128 rows, and under a table row of 66 entries: the same bits."""
    base, _ = _run(dev, D, dtype, 1, 64, 33, 8, False)
    for Rn, Mn, seed in ((64, 33, 11), (128, 17, 8), (64, 66, 8)):
        other, _ = _run(dev, D, dtype, 1, Rn, Mn, seed, False)
        assert torch.equal(PG.bits(other), PG.bits(base)), f"R={Rn} M={Mn} table {seed}"


def test_model_verify_int8(dev):
    """tests/test_gpu_verify.py's test_model_verify_logits on a PagedKVCacheQ8:
    GPT2.verify against T int8 decode steps on a copy of the cache, both
    measured against the fp32 CPU forward, with that test's criterion (the
    fp16 logit floor, 0.0079). verify must not touch the staging pair."""
    from zero_transformer_amd.models.paged import PagedKVCacheQ8

    T, live = 5, (5, 3, 1)
    model = make_model().to(dev).to(FP16)
    prompts = make_prompts(LENS)
    new = torch.randint(1, VOCAB, (len(prompts), T), generator=torch.Generator().manual_seed(77))
    m32 = copy.deepcopy(model).to("cpu").float()
    for blk in m32.blocks:
        blk.attn._qkv_w = None
    with torch.no_grad():
        want = [m32(torch.tensor([pr + new[b, :n].tolist()]))[0, -n:]
                for b, (pr, n) in enumerate(zip(prompts, live))]

    attn = model.blocks[0].attn
    cache = PagedKVCacheQ8(model.N, len(prompts), attn.num_head, attn.head_dim,
                           len(prompts) + 1, 64, 1, dev, FP16)
    idx = torch.zeros(len(prompts), max(LENS), dtype=torch.long)
    for b, pr in enumerate(prompts):
        cache.assign(b, len(pr) + T)
        idx[b, :len(pr)] = torch.tensor(pr)
    model.prefill(idx.to(dev), cache, torch.tensor(LENS))
    seq_cache = copy.deepcopy(cache)
    cache.stage_k.fill_(math.nan)
    got = model.verify(new.to(dev), cache, _i32(live, dev), _i32(LENS, dev)).float().cpu()
    assert bool(torch.isnan(cache.stage_k).all()), "verify wrote the staging cache"
    seq = []
    for i in range(T):
        seq_cache.set_len([n + i + 1 for n in LENS])
        seq.append(model(new[:, i:i + 1].to(dev), static_cache=seq_cache)[:, 0])
    seq = torch.stack(seq, 1).float().cpu()
    err_v = max(float((got[b, :n] - want[b]).abs().max()) for b, n in enumerate(live))
    err_s = max(float((seq[b, :n] - want[b]).abs().max()) for b, n in enumerate(live))
    print(f"[verify int8] max logit error: verify {err_v:.5f}, sequential decode {err_s:.5f}")
    assert err_v <= err_s + 0.0079
