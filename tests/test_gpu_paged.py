"""Paged KV cache on the GPU: the kernels of ops/csrc/attn_paged.hip against
the float64 references of tests/_prefill.py / tests/_parity.py on the gathered
logical cache (the bound is the contiguous ops' one, tests/test_gpu_prefill.py
and tests/test_gpu_ragged_decode.py), the pool bit for bit, and the serving
engine against generate_batch."""

from __future__ import annotations

import math

import pytest
import torch

from zero_transformer_amd.ops import reference

from . import _paged as PG
from . import _parity as P
from . import _prefill as PF
from ._parity import BF16, FP16
from ._ragged import make_model

pytestmark = pytest.mark.gpu

R = 64
B, H, T, M, PAGES = 3, 3, 200, 5, 20
# (lens, start): an append that spans three pages, a single row, one row past a
# page; an empty sequence, an end on a page boundary behind nothing, an
# unaligned past; the first row of a fresh page, a page-aligned past that ends
# on a boundary, the last row of the capacity.
PREFILL_CASES = (
    ((200, 1, 65), (0, 0, 0)),
    ((0, 128, 100), (0, 0, 37)),
    ((1, 64, 1), (64, 64, 319)),
)
# an inactive slot, fewer keys than splits, the last row of a page, the first
# row of a new page, several pages
DECODE_LENS = (0, 1, 5, 64, 65, 200)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _i32(x, dev):
    return torch.as_tensor(x, dtype=torch.int32).to(dev)


def _nan_pool(pages, Hn, Rn, D, dtype):
    return torch.full((pages, Hn, Rn, D), math.nan, dtype=dtype)


def _prefill_inputs(dtype, Bn, Hn, D, Tn, Mn, Rn, lens, start, seed):
    """qkv with NaN rows >= n; logical caches random below `start`, NaN from
    there on; the ranges and the logical caches the op must leave."""
    C = Hn * D
    qkv = P.randn((Bn, Tn, 3 * C), dtype, seed)
    k0 = P.randn((Bn, Hn, Mn * Rn, D), dtype, seed + 1)
    v0 = P.randn((Bn, Hn, Mn * Rn, D), dtype, seed + 2)
    ranges = PF.clamp_range(lens, start, Tn, Mn * Rn)
    for b, (st, n) in enumerate(ranges):
        qkv[b, n:] = math.nan
        k0[b, :, st:] = math.nan
        v0[b, :, st:] = math.nan
    k_want, v_want = PF.expected_caches(qkv, k0, v0, Hn, ranges)
    return qkv, k0, v0, k_want, v_want, ranges


def _pools(bt, used, pages, k0, v0, k_want, v_want):
    """NaN pools (page 0 and every unassigned page stay NaN) holding the live
    pages of the logical caches, and the pools the op must leave."""
    _, Hn, _, D = k0.shape
    Rn = k0.shape[2] // bt.shape[1]
    kp, vp = (PG.scatter(_nan_pool(pages, Hn, Rn, D, k0.dtype), bt, c, used) for c in (k0, v0))
    kw, vw = (PG.scatter(p.clone(), bt, c, used) for p, c in ((kp, k_want), (vp, v_want)))
    return kp, vp, kw, vw


def _run_prefill(dev, dtype, Bn, Hn, D, Tn, Mn, Rn, pages, lens, start, slopes, seed, bad,
                 table_seed=7):
    from zero_transformer_amd import ops

    qkv, k0, v0, k_want, v_want, ranges = _prefill_inputs(
        dtype, Bn, Hn, D, Tn, Mn, Rn, lens, start, seed)
    used = PG.pages_used([st + n for st, n in ranges], Rn)
    bt = PG.make_table(Bn, Mn, pages, table_seed, used)  # unused entries are 0
    kp, vp, kp_want, vp_want = _pools(bt, used, pages, k0, v0, k_want, v_want)
    kd, vd = kp.to(dev), vp.to(dev)
    got = ops.attention_prefill_paged(
        qkv.to(dev), kd, vd, Hn, None if slopes is None else slopes.to(dev),
        bt.to(dev), _i32(lens, dev), _i32(start, dev))
    assert got.shape == (Bn, Tn, Hn * D) and got.dtype == dtype
    got = got.cpu()
    tag = (f"prefill_paged D={D} R={Rn} {str(dtype)[6:]} lens={lens} start={start} "
           f"alibi={slopes is not None}")
    assert torch.equal(PG.bits(kd), PG.bits(kp_want)), f"k pool differs: {tag}"
    assert torch.equal(PG.bits(vd), PG.bits(vp_want)), f"v pool differs: {tag}"
    ref = PF.prefill_ref(qkv, k_want, v_want, Hn, slopes, ranges, dtype)
    for b, (st, n) in enumerate(ranges):
        assert torch.count_nonzero(got[b, n:]) == 0, f"rows >= n not zero, b={b}: {tag}"
        if n:
            r = P.worst_ratio(got[b, :n], ref[b][0], dtype, ref[b][1])
            print(f"[parity] {tag} b={b}: worst error/bound = {r:.3f}")
            if not r <= 1.0:
                bad.append(f"{tag} b={b}: error is {r:.3f} x the bound")
    return got


@pytest.mark.parametrize("dtype", [BF16, FP16])
@pytest.mark.parametrize("D", [32, 64, 96, 128])
def test_prefill_paged_kernel_edges(dev, D, dtype):
    slopes = reference.alibi_slopes(H)
    bad = []
    for i, (lens, start) in enumerate(PREFILL_CASES):
        for sl in (slopes, None):
            _run_prefill(dev, dtype, B, H, D, T, M, R, PAGES, lens, start, sl,
                         2100 + 10 * i, bad)
    assert not bad, "; ".join(bad)


def _decode_inputs(dtype, Hn, D, Mn, Rn, lens, eff, seed):
    """qkv, logical caches with NaN from row eff - 1 on (the row about to be
    written and the dead tail), and the logical caches the op must leave."""
    Bn, C = len(lens), Hn * D
    qkv = P.randn((Bn, 1, 3 * C), dtype, seed)
    k0 = P.randn((Bn, Hn, Mn * Rn, D), dtype, seed + 1)
    v0 = P.randn((Bn, Hn, Mn * Rn, D), dtype, seed + 2)
    q, kn, vn = (t.view(Bn, Hn, D) for t in qkv.split(C, dim=-1))
    for b, n in enumerate(eff):
        k0[b, :, max(n - 1, 0):] = math.nan
        v0[b, :, max(n - 1, 0):] = math.nan
    k_want, v_want = k0.clone(), v0.clone()
    for b, n in enumerate(eff):
        if n:
            k_want[b, :, n - 1] = kn[b]
            v_want[b, :, n - 1] = vn[b]
    return qkv, q, kn, vn, k0, v0, k_want, v_want


def _run_decode(dev, dtype, Hn, D, Mn, Rn, pages, lens, slopes, seed, items, eff=None,
                table_seed=8):
    from zero_transformer_amd import ops

    eff = lens if eff is None else eff
    Bn, C = len(lens), Hn * D
    qkv, q, kn, vn, k0, v0, k_want, v_want = _decode_inputs(dtype, Hn, D, Mn, Rn, lens, eff, seed)
    used = PG.pages_used(eff, Rn)
    bt = PG.make_table(Bn, Mn, pages, table_seed, used)
    kp, vp, kp_want, vp_want = _pools(bt, used, pages, k0, v0, k_want, v_want)
    kd, vd = kp.to(dev), vp.to(dev)
    got = ops.attention_decode_paged(
        qkv.to(dev), kd, vd, Hn, None if slopes is None else slopes.to(dev), bt.to(dev),
        _i32(lens, dev))
    assert got.shape == (Bn, 1, C) and got.dtype == dtype
    got = got.cpu().view(Bn, Hn, 1, D)
    tag = f"decode_paged D={D} R={Rn} {str(dtype)[6:]} alibi={slopes is not None}"
    assert torch.equal(PG.bits(kd), PG.bits(kp_want)), f"k pool differs, lens={lens}: {tag}"
    assert torch.equal(PG.bits(vd), PG.bits(vp_want)), f"v pool differs, lens={lens}: {tag}"
    kg, vg = PG.gather(kd.cpu(), bt), PG.gather(vd.cpu(), bt)
    for b, n in enumerate(eff):
        if n == 0:
            assert torch.count_nonzero(got[b]) == 0, f"empty slot not zero: {tag}"
            continue
        # the row at S - 1 is the projection's k / v columns
        assert torch.equal(PG.bits(kg[b, :, n - 1]), PG.bits(kn[b]))
        assert torch.equal(PG.bits(vg[b, :, n - 1]), PG.bits(vn[b]))
        want, a = P.attn_decode_ref(q[b].view(1, Hn, 1, D), k_want[b:b + 1],
                                    v_want[b:b + 1], slopes, n)
        items.append((f"{tag} S={lens[b]}", got[b:b + 1], want, a, dtype))
    return got


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
def test_decode_paged_kernel_edges(dev, D, dtype):
    slopes = reference.alibi_slopes(H)
    items = []
    for sl in (slopes, None):
        _run_decode(dev, dtype, H, D, M, R, 32, DECODE_LENS, sl, 2300, items)
    _check(items)


def test_decode_paged_table_rows_past_one_wave(dev):
    """The decode kernel keeps a table row of up to 64 entries in a register
    (one entry per lane) and looks longer rows up in memory: M = 64 is the
    last size of the first path, M = 66 takes the second, with a sequence
    whose last page is entry 65."""
    items = []
    sl = reference.alibi_slopes(H)
    _run_decode(dev, FP16, H, 32, 64, R, 200, (64 * R, 63 * R + 1, 70), sl, 2700, items)
    _run_decode(dev, FP16, H, 32, 66, R, 200, (65 * R + 3, 70), sl, 2710, items)
    _check(items)


def test_paged_kernels_page_size_no_power_of_two(dev):
    """192 rows per page (a multiple of 64, no power of two): the decode
    kernel finds a key's page by an integer division here and by a shift
    otherwise; the prefill kernels divide either way. Lengths on, next to and
    across page boundaries."""
    sl = reference.alibi_slopes(H)
    items, bad = [], []
    _run_decode(dev, FP16, H, 64, 3, 192, 20, (0, 1, 192, 193, 500), sl, 2800, items)
    _check(items)
    _run_prefill(dev, FP16, 3, H, 64, 200, 2, 192, 12, (200, 1, 65), (0, 0, 300), sl, 2810, bad)
    assert not bad, "; ".join(bad)


def test_paged_kernels_clamp_what_addresses_a_write(dev):
    """lens > T, start + lens > M*R, a negative length and start > M*R for the
    prefill; a length above the capacity and a negative one for decode; pages
    of 128 rows. The clamped rows are written and nothing else is (the pools
    are compared whole)."""
    Tn, Mn, Rn = 70, 2, 128
    cap = Mn * Rn
    lens = (Tn + 5, 9, -3, 4)
    start = (0, cap - 3, 7, cap + 2)
    assert PF.clamp_range(lens, start, Tn, cap) == [(0, Tn), (cap - 3, 3), (7, 0), (cap, 0)]
    bad = []
    sl = reference.alibi_slopes(H)
    _run_prefill(dev, BF16, 4, H, 128, Tn, Mn, Rn, 12, lens, start, sl, 2400, bad)
    assert not bad, "; ".join(bad)
    items = []
    _run_decode(dev, BF16, H, 128, Mn, Rn, 12, (cap + 2, -1, 3), sl, 2410, items,
                eff=(cap, 0, 3))
    _check(items)


def test_paged_kernels_raise_on_a_bad_layout(dev):
    from zero_transformer_amd import ops

    D = 64
    qkv = P.randn((1, 1, 3 * H * D), BF16, 1).to(dev)
    pool = torch.zeros(4, H, 48, D, dtype=BF16, device=dev)  # 48 rows per page
    bt = torch.ones(1, 2, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError):
        ops.attention_decode_paged(qkv, pool, pool.clone(), H, None, bt, _i32([1], dev))
    with pytest.raises(RuntimeError):
        ops.attention_prefill_paged(qkv, pool, pool.clone(), H, None, bt)


@pytest.mark.parametrize("dtype", [BF16, FP16])
def test_layout_independence(dev, dtype):
    """The same logical inputs under two tables, and under pages of 64 and of
    128 rows, give the same bits for both ops: tile order and split partition
    depend on the logical rows only. They are also the bits of the contiguous
    ops (attention_prefill_append / attention_decode_append), whose key order
    the paged kernels keep (profiles/PERF.md "Paged KV")."""
    from zero_transformer_amd import ops

    D, Tn = 128, 200
    lens, start = (200, 64, 100), (0, 64, 37)
    sl = reference.alibi_slopes(H)
    bad, outs = [], []
    for Rn, Mn, pages, ts in ((64, 6, 20, 7), (64, 6, 24, 11), (128, 3, 12, 7)):
        outs.append(_run_prefill(dev, dtype, B, H, D, Tn, Mn, Rn, pages, lens, start, sl,
                                 2500, bad, table_seed=ts))
    assert not bad, "; ".join(bad)
    qkv, k0, v0, *_ = _prefill_inputs(dtype, B, H, D, Tn, 6, 64, lens, start, 2500)
    cont = ops.attention_prefill_append(
        qkv.to(dev), k0.to(dev), v0.to(dev), H, sl.to(dev), _i32(lens, dev),
        _i32(start, dev)).cpu()
    same = torch.equal(PG.bits(outs[0]), PG.bits(cont))
    print(f"[paged] prefill {str(dtype)[6:]}: bit-equal to attention_prefill_append: {same}")
    assert torch.equal(PG.bits(outs[0]), PG.bits(outs[1])), "prefill depends on the table"
    assert torch.equal(PG.bits(outs[0]), PG.bits(outs[2])), "prefill depends on page_rows"
    assert same, "prefill differs from the contiguous op"

    items, outs = [], []
    dl = (0, 1, 5, 64, 65, 200, 384)
    for Rn, Mn, pages, ts in ((64, 6, 48, 8), (64, 6, 60, 12), (128, 3, 24, 8)):
        outs.append(_run_decode(dev, dtype, H, D, Mn, Rn, pages, dl, sl, 2600, items,
                                table_seed=ts))
    _check(items)
    qkv, q, kn, vn, k0, v0, *_ = _decode_inputs(dtype, H, D, 6, 64, dl, dl, 2600)
    cont = ops.attention_decode_append(
        qkv.to(dev), k0.to(dev), v0.to(dev), H, sl.to(dev), _i32(dl, dev)).cpu()
    same = torch.equal(PG.bits(outs[0].reshape(len(dl), -1)), PG.bits(cont.reshape(len(dl), -1)))
    print(f"[paged] decode {str(dtype)[6:]}: bit-equal to attention_decode_append: {same}")
    assert torch.equal(PG.bits(outs[0]), PG.bits(outs[1])), "decode depends on the table"
    assert torch.equal(PG.bits(outs[0]), PG.bits(outs[2])), "decode depends on page_rows"
    assert same, "decode differs from the contiguous op"


@pytest.fixture(scope="module")
def served(dev):
    """The CPU scenario of tests/test_paged.py in fp16 on the GPU: each
    request alone through generate_batch, and the engine with and without the
    captured graph. fp16 because twice its measured logit floor
    (tests/test_gpu_prefill.py: 0.0079) is six times under the 0.05 top-2 gap
    the scenario was chosen for; the bf16 floor (0.032) is not."""
    from zero_transformer_amd.models.inference import generate_batch

    model = make_model(num_ctx=192).to(dev).to(FP16)
    prompts, counts = PG.scenario()
    alone = [generate_batch(model, [pr], n)[0] for pr, n in zip(prompts, counts)]
    runs = {g: PG.serve(model, use_graph=g) for g in (True, False)}
    return alone, runs


@pytest.mark.parametrize("use_graph", [True, False])
def test_engine_equals_generate_batch(served, use_graph):
    alone, runs = served
    got, eng, seen = runs[use_graph]
    assert (eng.graph is not None) == use_graph
    assert [len(r) for r in alone] == list(PG.N_NEW) + [PG.N_NEW_11]
    assert got == alone
    assert seen["shared_pages"] == 1 and seen["start"] == R and seen["ref"] == 2
    PG.assert_drained(eng)


def test_engine_graph_equals_eager(served):
    _, runs = served
    assert runs[True][0] == runs[False][0]
