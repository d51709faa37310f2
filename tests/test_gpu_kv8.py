"""The int8 paged KV cache (ops/csrc/attn_kv8.hip): the quantizing append and
the dequantizing load bit for bit against ops/reference.py, the native int8
decode attention against a float64 attention over the dequantized cache
((u - 128) * scale is exact in float64; the kernel subtracts the offset per
element, so the bound is _parity.attn_decode_ref's with no extra term), and
the serving engine on the int8 cache. One CPU test at the end."""

from __future__ import annotations

import math

import pytest
import torch

from zero_transformer_amd import ops
from zero_transformer_amd.ops import reference

from . import _paged as PG
from . import _parity as P
from . import _prefill as PF
from ._parity import BF16, FP16
from ._ragged import make_model
from .test_gpu_paged import DECODE_LENS, PREFILL_CASES

gpu = pytest.mark.gpu
R = 64
B, H, T, M, PAGES = 3, 3, 200, 5, 20
GRID = [pytest.param(D, dt, id=f"D{D}-{str(dt)[6:]}")
        for D in (32, 64, 96, 128) for dt in (BF16, FP16)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _i32(x, dev):
    return torch.as_tensor(x, dtype=torch.int32).to(dev)


def _blank_pools(pages, Hn, Rn, D):
    """Code pools holding a byte pattern and NaN scale pools: (k, v, ks, vs)."""
    pat = (torch.arange(pages * Hn * Rn * D) % 251).to(torch.uint8).view(pages, Hn, Rn, D)
    nan = torch.full((pages, Hn, Rn), math.nan)
    return pat.clone(), pat.flip(0).contiguous(), nan.clone(), nan.clone()


def _same(got, want, what):
    for name, g, w in zip(("k_pool", "v_pool", "k_scale", "v_scale"), got, want):
        g, w = g.cpu(), w.cpu()
        same = torch.equal(g, w) if g.dtype == torch.uint8 else torch.equal(PG.bits(g), PG.bits(w))
        assert same, f"{name} differs: {what}"


@gpu
@pytest.mark.parametrize("case", range(len(PREFILL_CASES)))
@pytest.mark.parametrize("D,dtype", GRID)
def test_quantize_paged_bits(dev, D, dtype, case):
    lens, start = PREFILL_CASES[case]
    C = H * D
    ranges = PF.clamp_range(lens, start, T, M * R)
    qkv = P.randn((B, T, 3 * C), dtype, 3100 + case)
    big = torch.finfo(dtype).max
    for b, (st, n) in enumerate(ranges):
        qkv[b, 0, C:C + D] = 0.0           # a zero row (head 0 of K)
        qkv[b, 0, C + D + 3] = big         # the largest finite value (head 1 of K)
        qkv[b, 0, 2 * C + D + 5] = -big    # and of V
        qkv[b, n:] = math.nan              # never read
    bt = PG.make_table(B, M, PAGES, 7, PG.pages_used([st + n for st, n in ranges], R))
    want_qkv, want = qkv.clone(), _blank_pools(PAGES, H, R, D)
    reference.kv8_quantize_paged(want_qkv, *want, bt, _i32(lens, "cpu"), _i32(start, "cpu"))
    got_qkv, got = qkv.to(dev), [t.to(dev) for t in _blank_pools(PAGES, H, R, D)]
    ops.kv8_quantize_paged(got_qkv, *got, bt.to(dev), _i32(lens, dev), _i32(start, dev))
    tag = f"lens={lens} start={start}"
    _same(got, want, tag)  # written rows and everything that must stay
    assert torch.equal(PG.bits(got_qkv), PG.bits(want_qkv)), f"qkv differs: {tag}"
    # the reference's paging aside: the written logical rows are quantize_kv_rows
    for col, (pool, sc) in ((C, (got[0], got[2])), (2 * C, (got[1], got[3]))):
        codes = PG.gather(pool.cpu(), bt)
        scales = PG.gather(sc.cpu().unsqueeze(-1), bt).squeeze(-1)
        for b, (st, n) in enumerate(ranges):
            x = qkv[b, :n, col:col + C].reshape(n, H, D).transpose(0, 1)
            u, s = reference.quantize_kv_rows(x)
            assert torch.equal(codes[b, :, st:st + n], u), f"codes, b={b}: {tag}"
            assert torch.equal(PG.bits(scales[b, :, st:st + n]), PG.bits(s)), f"scales: {tag}"
            assert torch.equal(PG.bits(got_qkv[b, :n, col:col + C].cpu()),
                               PG.bits(reference.dequantize_kv_rows(u, s, dtype)
                                       .transpose(0, 1).reshape(n, C))), f"rewrite: {tag}"


@gpu
@pytest.mark.parametrize("D,dtype", GRID)
def test_load_paged_bits(dev, D, dtype):
    """rows = nothing, one row past a page, more than the capacity."""
    g = torch.Generator().manual_seed(3200 + D)
    pools = [torch.randint(0, 256, (PAGES, H, R, D), generator=g, dtype=torch.uint8)
             for _ in range(2)]
    pools += [torch.rand(PAGES, H, R, generator=g) + 0.01 for _ in range(2)]
    bt = PG.make_table(B, M, PAGES, 9)
    rows = (0, 65, M * R + 80)
    want = [torch.full((B, H, M * R, D), math.nan, dtype=dtype) for _ in range(2)]
    reference.kv8_load_paged(*pools, bt, _i32(rows, "cpu"), *want)
    got = [t.to(dev) for t in (torch.full_like(w, math.nan) for w in want)]
    ops.kv8_load_paged(*(t.to(dev) for t in pools), bt.to(dev), _i32(rows, dev), *got)
    for g_, w in zip(got, want):
        assert torch.equal(PG.bits(g_), PG.bits(w))
    assert not torch.isnan(want[0][2]).any() and torch.isnan(want[0][1, :, 65:]).all()


def _decode_run(dev, dtype, D, Rn, Mn, pages, table_seed, slopes, check):
    """DECODE_LENS through the op under one layout; the logical rows do not
    depend on the layout. -> out (B, 1, C) on the CPU."""
    Bn, C, top = len(DECODE_LENS), H * D, max(DECODE_LENS)
    qkv = P.randn((Bn, 1, 3 * C), dtype, 3300)
    logical = []
    for i in range(2):
        u, s = reference.quantize_kv_rows(P.randn((Bn, H, top, D), dtype, 3301 + i))
        u = torch.cat([u, torch.full((Bn, H, Mn * Rn - top, D), 7, dtype=torch.uint8)], 2)
        s = torch.cat([s, torch.full((Bn, H, Mn * Rn - top), math.nan)], 2)
        for b, n in enumerate(DECODE_LENS):  # the row to be written and the dead tail
            u[b, :, max(n - 1, 0):] = 7
            s[b, :, max(n - 1, 0):] = math.nan
        logical += [u, s.unsqueeze(-1)]
    used = PG.pages_used(DECODE_LENS, Rn)
    bt = PG.make_table(Bn, Mn, pages, table_seed, used)
    blank = _blank_pools(pages, H, Rn, D)
    pools = [PG.scatter(blank[0], bt, logical[0], used), PG.scatter(blank[1], bt, logical[2], used),
             PG.scatter(blank[2].unsqueeze(-1), bt, logical[1], used).squeeze(-1),
             PG.scatter(blank[3].unsqueeze(-1), bt, logical[3], used).squeeze(-1)]
    got = [t.to(dev) for t in pools]
    out = ops.attention_decode_paged_q8(
        qkv.to(dev), *got, H, None if slopes is None else slopes.to(dev), bt.to(dev),
        _i32(DECODE_LENS, dev)).cpu()
    assert out.shape == (Bn, 1, C) and out.dtype == dtype
    if not check:
        return out
    tag = f"decode_q8 D={D} {str(dtype)[6:]} alibi={slopes is not None}"
    reference.attention_decode_paged_q8(qkv, *pools, H, slopes, bt, _i32(DECODE_LENS, "cpu"))
    _same(got, pools, tag)  # the appended codes and scale, and nothing else
    kf, vf = ((PG.gather(got[i].cpu(), bt).double() - 128.0)
              * PG.gather(got[i + 2].cpu().unsqueeze(-1), bt).double() for i in (0, 1))
    q = qkv[:, 0, :C].view(Bn, H, 1, D)
    bad = []
    for b, n in enumerate(DECODE_LENS):
        o = out[b].view(1, H, 1, D)
        if n == 0:
            assert torch.count_nonzero(o) == 0, f"empty slot not zero: {tag}"
            continue
        want, a = P.attn_decode_ref(q[b:b + 1], kf[b:b + 1], vf[b:b + 1], slopes, n)
        r = P.worst_ratio(o, want, dtype, a)
        print(f"[parity] {tag} S={n}: worst error/bound = {r:.3f}")
        if not r <= 1.0:
            bad.append(f"{tag} S={n}: error is {r:.3f} x the bound")
    assert not bad, "; ".join(bad)
    return out


@gpu
@pytest.mark.parametrize("D,dtype", GRID)
def test_decode_q8_kernel_edges(dev, D, dtype):
    """Both ALiBi settings against float64; then the same logical cache under
    another table, under pages of 128 rows, and under a table row of 66
    entries (looked up in memory, not in a register): the same bits."""
    slopes = reference.alibi_slopes(H)
    _decode_run(dev, dtype, D, R, M, 32, 8, None, True)
    base = _decode_run(dev, dtype, D, R, M, 32, 8, slopes, True)
    for Rn, Mn, pages, seed in ((R, M, 32, 11), (128, 3, 20, 8), (R, 66, 400, 8)):
        other = _decode_run(dev, dtype, D, Rn, Mn, pages, seed, slopes, False)
        assert torch.equal(PG.bits(other), PG.bits(base)), f"R={Rn} M={Mn} table {seed}"


@pytest.fixture(scope="module")
def served(dev):
    """tests/_paged.py's scenario (a 130-token prompt, a shared first page) on
    the int8 cache, with and without the captured graph."""
    model = make_model(num_ctx=192).to(dev).to(FP16)
    return {g: PG.serve(model, use_graph=g, kv_int8=True) for g in (True, False)}


@gpu
def test_engine_int8_graph_equals_eager(served):
    from zero_transformer_amd.models.paged import PagedKVCacheQ8

    for g, (tokens, eng, seen) in served.items():
        assert (eng.graph is not None) == g and isinstance(eng.cache, PagedKVCacheQ8)
        assert [len(t) for t in tokens] == list(PG.N_NEW) + [PG.N_NEW_11]
        assert seen["shared_pages"] == 1 and seen["start"] == R
        PG.assert_drained(eng)
    assert served[True][0] == served[False][0]


def test_kv8_references_cpu():
    """The quantizer's round trip, and the paged int8 decode reference against
    the 16-bit one on the gathered, dequantized fp32 pools."""
    D, C, lens = 32, H * 32, (0, 1, 65, 130)
    x = P.randn((4, H, 9, D), torch.float32, 3400, scale=3.0)
    x[0, 0, 0] = 0.0
    u, s = reference.quantize_kv_rows(x)
    assert u.dtype == torch.uint8 and int(u.min()) >= 1 and bool((u[0, 0, 0] == 128).all())
    assert float(s[0, 0, 0]) == 0.0
    # half a step, plus the two fp32 roundings on the way (the quotient x /
    # scale and the product q * scale, half an ulp of |x| each)
    err = (P.f64(x) - P.f64(reference.dequantize_kv_rows(u, s, torch.float32))).abs()
    assert bool((err <= P.f64(s).unsqueeze(-1) / 2 + 2.0 ** -23 * P.f64(x).abs()).all())

    g = torch.Generator().manual_seed(3401)
    bt = PG.make_table(len(lens), 3, 16, 5)
    pools = [torch.randint(1, 256, (16, H, R, D), generator=g, dtype=torch.uint8) for _ in range(2)]
    pools += [torch.rand(16, H, R, generator=g) + 0.01 for _ in range(2)]
    qkv = P.randn((len(lens), 1, 3 * C), torch.float32, 3402)
    slopes = reference.alibi_slopes(H)
    kf, vf = (reference.dequantize_kv_rows(pools[i], pools[i + 2], torch.float32) for i in (0, 1))
    q_in = qkv.clone()
    for col in (C, 2 * C):  # the new row as the cache will hold it
        new = reference.quantize_kv_rows(qkv[:, 0, col:col + C].reshape(-1, H, D))
        q_in[:, 0, col:col + C] = reference.dequantize_kv_rows(*new, torch.float32).reshape(-1, C)
    want = reference.attention_decode_paged(q_in, kf, vf, H, slopes, bt, _i32(lens, "cpu"))
    got = reference.attention_decode_paged_q8(qkv, *pools, H, slopes, bt, _i32(lens, "cpu"))
    assert torch.equal(got, want)
    # the pools now hold the new rows: dequantized, they are the 16-bit op's
    for i, f in ((0, kf), (1, vf)):
        assert torch.equal(reference.dequantize_kv_rows(pools[i], pools[i + 2], torch.float32), f)
