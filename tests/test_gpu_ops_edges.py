"""HIP kernels at their edge shapes vs float64 references (tests/_parity.py).

Shapes are the smallest that reach each code path: partial and whole waves,
the thresholds between vector and generic kernels, odd sizes, one row, and
row / element counts just past each grid cap (grid-stride loops). Bounds are
the derived ones of tests/_parity.py; every check prints its worst
error / bound ratio, and the module prints the worst per operation at the end.
"""

import math

import pytest
import torch

from zero_transformer_amd.ops import reference

from . import _parity as P
from ._parity import BF16, FP16, FP32

pytestmark = pytest.mark.gpu

EPS = 1e-6
WORST = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    yield torch.device("cuda", 0)
    for op, r in sorted(WORST.items()):
        print(f"[parity-summary] {op}: worst error/bound = {r:.3f}")


def _ext():
    from zero_transformer_amd import ops

    assert ops.hip_available(), "HIP extension must be built on GPU boxes"
    return ops.hip_ops()


def _check(items):
    """items: (name, got, want, abs_term, dtype). Checks all, then asserts."""
    bad = []
    for name, got, want, a, dt in items:
        r = P.worst_ratio(got, want, dt, a)
        print(f"[parity] {name}: worst error/bound = {r:.3f}")
        op = name.split(" ")[0]
        WORST[op] = max(WORST.get(op, 0.0), r)
        if not r <= 1.0:
            bad.append(f"{name}: error is {r:.3f} x the bound")
    assert not bad, "; ".join(bad)


# ---------------------------------------------------------------------------
# LayerNorm forward / backward
#
#   C     rows          reaches
#   512   1, 3, 4100    one wave; 4100 rows > the 4096 grid cap
#   768   1, 3          1.5 waves  (partial wave)
#   1280  1, 3          2.5 waves  (partial wave)
#   1536  1, 3          three whole waves
#   8192  1, 3          16 waves, top of the vector path
#   8200  1, 3          C/8 > 1024 -> generic kernel
#   264   1, 3, 2050    C/8 < 64 -> generic; 2050 rows > the 2048 / 1024 caps
#   100   1, 3          C % 8 != 0 -> generic
# ---------------------------------------------------------------------------


def _ln_case(dev, C, rows, dtype, offset=0.0):
    ext = _ext()
    x, w, dy = P.ln_inputs(C, rows, dtype, offset)
    want = {**P.ln_ref(x, w, EPS), **P.ln_bwd_ref(dy, x, w, EPS)}
    xd, wd, dyd = x.to(dev), w.to(dev), dy.to(dev)
    y, rstd, mean = ext.layernorm_fwd(xd, wd, EPS)
    dx, dw = ext.layernorm_bwd(dyd, xd, wd, rstd, mean)
    assert y.dtype == dtype and dx.dtype == dtype and dw.dtype == dtype
    assert mean.dtype == FP32 and rstd.dtype == FP32 and mean.shape == (rows,)
    got = {"y": y, "mean": mean, "rstd": rstd, "dx": dx, "dw": dw}
    for t in got.values():
        assert torch.isfinite(t).all()
    tag = f"layernorm C={C} rows={rows} {str(dtype)[6:]}" + (" offset" if offset else "")
    _check([
        (f"{tag} {n}", got[n], want[n][0], want[n][1], FP32 if n in ("mean", "rstd") else dtype)
        for n in ("y", "mean", "rstd", "dx", "dw")
    ])


@pytest.mark.parametrize("C,rows", P.LN_SHAPES)
def test_layernorm_bf16(dev, C, rows):
    _ln_case(dev, C, rows, BF16)


@pytest.mark.parametrize("rows", [1, 3, 2050])
def test_layernorm_fp32_generic(dev, rows):
    _ln_case(dev, 264, rows, FP32)


@pytest.mark.parametrize("C", [768, 2048, 264])
def test_layernorm_common_offset(dev, C):
    """Rows of 64 + N(0,1): E[x^2] - mean^2 cancels ~4096:1 in fp32."""
    _ln_case(dev, C, 3, BF16, offset=64.0)


def test_layernorm_wrapper_autograd_partial_wave(dev):
    """ops.layer_norm (autograd path) at a partial-wave width."""
    from zero_transformer_amd import ops

    x, w, dy = P.ln_inputs(768, 3, BF16)
    want = {**P.ln_ref(x, w, EPS), **P.ln_bwd_ref(dy, x, w, EPS)}
    xd = x.to(dev).requires_grad_(True)
    wd = w.to(dev).requires_grad_(True)
    y = ops.layer_norm(xd, wd, EPS)
    y.backward(dy.to(dev))
    _check([
        ("layernorm wrapper y", y, *want["y"], BF16),
        ("layernorm wrapper dx", xd.grad, *want["dx"], BF16),
        ("layernorm wrapper dw", wd.grad, *want["dw"], BF16),
    ])


def test_layernorm_bwd_rejects_oversized_lds(dev):
    """The generic backward keeps dw in (C + 16) * 4 bytes of dynamic LDS; a
    width past the device limit must raise on the host, not launch."""
    ext = _ext()
    limit = torch.cuda.get_device_properties(dev).shared_memory_per_block
    C = 1 << 20
    assert (C + 16) * 4 > limit
    for dtype in (FP32, BF16):  # bf16: C / 8 > 1024 -> generic kernel too
        x = torch.zeros(1, C, device=dev, dtype=dtype)
        w = torch.ones(C, device=dev, dtype=dtype)
        stat = torch.ones(1, device=dev, dtype=FP32)
        with pytest.raises(RuntimeError, match="LDS"):
            ext.layernorm_bwd(x, x, w, stat, stat)


# ---------------------------------------------------------------------------
# Fused add + LayerNorm (decode path)
# ---------------------------------------------------------------------------

ADD_LN_CASES = [(512, r) for r in (1, 3, 4100)] + [
    (C, r) for C in P.ADD_LN_KERNEL_C[1:] for r in (1, 3)
]


def _add_ln_inputs(C, rows, dtype):
    x, w, _ = P.ln_inputs(C, rows, dtype)
    return x, P.randn((rows, C), dtype, 77), w


@pytest.mark.parametrize("dtype", [BF16, FP16])
@pytest.mark.parametrize("C,rows", ADD_LN_CASES)
def test_add_ln_kernel(dev, C, rows, dtype):
    from zero_transformer_amd import ops

    x, h, w = _add_ln_inputs(C, rows, dtype)
    with torch.no_grad():
        y, ln = ops.add_ln(x.to(dev), h.to(dev), w.to(dev), EPS)
        y2, ln2 = _ext().add_ln_fwd(x.to(dev), h.to(dev), w.to(dev), EPS)
    assert torch.equal(y, y2) and torch.equal(ln, ln2), "wrapper must route to the kernel"
    v = P.f64(x) + P.f64(h)
    want, a = P.ln_ref(v, w, EPS)["y"]
    tag = f"add_ln C={C} rows={rows} {str(dtype)[6:]}"
    _check([(f"{tag} y", y, v, 0.0, dtype), (f"{tag} ln", ln, want, a, dtype)])


@pytest.mark.parametrize("dtype", [BF16, FP16])
@pytest.mark.parametrize("C", P.ADD_LN_TORCH_C)
def test_add_ln_torch_widths(dev, C, dtype):
    """Widths outside the kernel's range: the wrapper's torch route is still
    right, and the binding refuses them (gate and TORCH_CHECK agree)."""
    from zero_transformer_amd import ops

    x, h, w = _add_ln_inputs(C, 3, dtype)
    with torch.no_grad():
        y, ln = ops.add_ln(x.to(dev), h.to(dev), w.to(dev), EPS)
        with pytest.raises(RuntimeError):
            _ext().add_ln_fwd(x.to(dev), h.to(dev), w.to(dev), EPS)
    # torch normalises the rounded sum, so that is the input of the reference
    want, a = P.ln_ref(y, w, EPS)["y"]
    tag = f"add_ln-torch C={C} {str(dtype)[6:]}"
    _check([(f"{tag} y", y, P.f64(x) + P.f64(h), 0.0, dtype), (f"{tag} ln", ln, want, a, dtype)])


# ---------------------------------------------------------------------------
# Cross entropy through the binding
#   V = 8: one vector, 255 threads own no column.  2040 / 2056: just below /
#   above one full 256 x 8 sweep.  50304: the model's vocabulary.  1001: bf16
#   generic path.  1000 fp32.  4100 rows at V = 64: past the 4096 grid cap.
# ---------------------------------------------------------------------------

CE_CASES = [(V, r, dt, ig) for V, r, dt in P.CE_SHAPES
            for ig in ((None,) if r == 1 else (None, "divisor", "rows"))]


@pytest.mark.parametrize("V,rows,dtype,ignore", CE_CASES)
def test_cross_entropy_edges(dev, V, rows, dtype, ignore):
    ext = _ext()
    logits, targets = P.ce_inputs(V, rows, dtype, ignore is not None)
    divisor = int((targets >= 0).sum()) if ignore == "divisor" else 0
    dloss = 2.0
    want = P.ce_ref(logits, targets, divisor, dloss)
    ld, td = logits.to(dev), targets.to(dev)
    loss, lse = ext.cross_entropy_fwd(ld, td, divisor)
    d = ext.cross_entropy_bwd(ld, td, lse, torch.tensor(dloss, device=dev), divisor)
    assert d.dtype == dtype and lse.dtype == FP32 and lse.shape == (rows,)
    assert torch.isfinite(lse).all() and torch.isfinite(loss).all() and torch.isfinite(d).all()
    tag = f"cross_entropy V={V} rows={rows} {str(dtype)[6:]} ignore={ignore}"
    _check([
        (f"{tag} lse", lse, *want["lse"], FP32),
        (f"{tag} loss", loss, *want["loss"], FP32),
        (f"{tag} dlogits", d, *want["dlogits"], dtype),
    ])
    # each counted row of dlogits sums to 0 up to the rounding of its entries
    # (tolerance derived in ce_ref); ignored rows are exactly 0
    live, tol = want["live"], want["rowsum_tol"]
    sums = P.f64(d).sum(-1).abs()
    print(f"[parity] {tag} rowsum: worst sum/tol = {float((sums / tol)[live].max()):.3f}")
    assert bool((sums[live] <= tol[live]).all())
    assert not P.f64(d)[~live].any()


# ---------------------------------------------------------------------------
# AdamW: three steps, each checked from the state the kernel read
#   4099: n % 4 != 0 -> scalar kernel.  4224: vector kernel.
#   4096*256*4 + 1028: vector kernel past its 4096-block grid (grid-stride).
# ---------------------------------------------------------------------------

ADAMW_BIG = 4096 * 256 * 4 + 1028
ADAMW_CASES = [(n, g, e, wd, s) for n in (4099, 4224) for g in (BF16, FP32)
               for e in (True, False) for wd in (0.0, 0.1) for s in (1, 10000)]
ADAMW_CASES += [(ADAMW_BIG, g, e, 0.1, 1) for g in (BF16, FP32) for e in (True, False)]
ADAMW_CASES += [(ADAMW_BIG + 3, BF16, True, 0.1, 1)]  # scalar grid-stride


def _adamw_run(dev, n, gdtype, emit, wd, step0, clip):
    from zero_transformer_amd import ops

    p = P.randn((n,), FP32, 1).to(dev)
    if step0 == 1:
        m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    else:
        m = P.randn((n,), FP32, 2, 0.1).to(dev)
        v = P.randn((n,), FP32, 3, 0.1).abs().to(dev)
    pb = torch.zeros(n, device=dev, dtype=BF16) if emit else None
    hp = (1e-3, 0.9, 0.95, 1e-8, wd, clip, 0.5)
    items = []
    for i in range(3):
        g = P.randn((n,), gdtype, 10 + i, 3.0).to(dev)  # x 0.5 scale: many exceed clip 1
        assert (g.float().abs() * 0.5 > 1.0).any()
        (wp, ap), (wm, am), (wv, av) = P.adamw_ref(p, g, m, v, step0 + i, *hp)
        ops.adamw_step(p, pb, g, m, v, step0 + i, *hp)
        tag = f"adamw n={n} g={str(gdtype)[6:]} emit={emit} wd={wd} clip={clip} step={step0 + i}"
        items += [(f"{tag} p", p.clone(), wp, ap, FP32), (f"{tag} m", m.clone(), wm, am, FP32),
                  (f"{tag} v", v.clone(), wv, av, FP32)]
        if emit:
            assert torch.equal(pb, p.to(BF16)), "bf16 copy must be the rounded fp32 param"
    _check(items)
    return m, g


@pytest.mark.parametrize("n,gdtype,emit,wd,step0", ADAMW_CASES)
def test_adamw_edges(dev, n, gdtype, emit, wd, step0):
    _adamw_run(dev, n, gdtype, emit, wd, step0, clip=1.0)


@pytest.mark.parametrize("n", [4099, 4224])
def test_adamw_clip_zero_disables_clipping(dev, n):
    """clip_value = 0 means no clipping, as in reference.adamw_update (the
    kernel used to clamp every gradient to 0)."""
    from zero_transformer_amd import ops

    _adamw_run(dev, n, BF16, True, 0.1, 1, clip=0.0)
    g = P.randn((n,), BF16, 10, 3.0).to(dev)
    p, m, v = P.randn((n,), FP32, 1).to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    pr, mr, vr = p.cpu().clone(), m.cpu().clone(), v.cpu().clone()
    ops.adamw_step(p, None, g, m, v, 1, 1e-3, 0.9, 0.95, 1e-8, 0.0, 0.0, 1.0)
    reference.adamw_update(pr, g.cpu(), mr, vr, 1, 1e-3, 0.9, 0.95, 1e-8, 0.0, 0.0, 1.0)
    assert m.abs().max().item() > 0.1 * 1.5, "gradients above 1 must survive"
    assert torch.allclose(m.cpu(), mr, rtol=1e-6, atol=0.0)


# ---------------------------------------------------------------------------
# Residual-add + dropout
# ---------------------------------------------------------------------------

RES_N = 8 * (4096 * 256 + 3)  # past the 4096-block grid; i4 >> 16 reaches 32


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_residual_dropout_grid_stride_and_high_word(dev, p):
    ext = _ext()
    seed = 777
    x, h, dy = (P.randn((RES_N,), BF16, s) for s in (1, 2, 3))
    keep = reference.residual_drop_mask(seed, RES_N, p)
    inv = reference.drop_inv_keep(p)
    if p == 0.0:
        assert bool(keep.all())
    else:
        assert abs(float(keep.float().mean()) - (1 - 77 / 256)) < 1e-3
    y = ext.residual_dropout_fwd(x.to(dev), h.to(dev), p, seed)
    dh = ext.residual_dropout_bwd(dy.to(dev), p, seed)
    wy, ay = P.residual_ref(x, h, keep, inv)
    wd, ad = P.residual_ref(torch.zeros_like(dy), dy, keep, inv)
    # a wrong mask flips whole elements: exact-mask comparison
    assert torch.equal(dh.cpu() != 0, (keep & (dy != 0)))
    _check([(f"residual_dropout p={p} y", y, wy, ay, BF16),
            (f"residual_dropout p={p} dh", dh, wd, ad, BF16)])


# ---------------------------------------------------------------------------
# GELU
# ---------------------------------------------------------------------------

GELU_BIG = 8 * (2048 * 256 + 3)  # past the 2048-block grid of the vector path


@pytest.mark.parametrize("n,dtype", [(GELU_BIG, BF16), (1003, BF16), (1003, FP32), (1024, FP16)])
def test_gelu_edges(dev, n, dtype):
    ext = _ext()
    x, dy = P.gelu_inputs(n, dtype)
    (wy, ay), (wdx, adx) = P.gelu_ref(x, dy)
    y = ext.gelu_fwd(x.to(dev))
    tag = f"gelu n={n} {str(dtype)[6:]}"
    items = [(f"{tag} y", y, wy, ay, dtype)]
    outs = [y]
    if dtype != FP16:  # fp16 is forward-only (decode path)
        dx = ext.gelu_bwd(dy.to(dev), x.to(dev))
        items.append((f"{tag} dx", dx, wdx, adx, dtype))
        outs.append(dx)
    for t in outs:
        assert t.dtype == dtype and torch.isfinite(t).all()
    # saturated ends: gelu(x) is x or 0, gelu'(x) is 1 or 0
    ns = len(P.GELU_SPECIALS)
    for sl in (slice(0, ns), slice(n - ns, n)):
        xs = P.f64(x[sl])
        sat = xs.abs() >= 10.0
        want_y = torch.where(xs > 0, xs, torch.zeros_like(xs))
        assert bool(((P.f64(y[sl]) - want_y).abs()[sat] <= 1e-30).all())
        if dtype != FP16:
            want_g = P.f64(dy[sl]) * (xs > 0)
            assert bool(((P.f64(outs[1][sl]) - want_g).abs()[sat] <= 1e-30).all())
    _check(items)


# ---------------------------------------------------------------------------
# Decode GEMV: all 16 batch instances, N off the 4-rows-per-block grid
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [BF16, FP16])
@pytest.mark.parametrize("B", list(range(1, 17)))
def test_gemv_edges(dev, B, dtype):
    ext = _ext()
    items = []
    for N in (5, 1023, 1024):
        for K in (512, 1536):
            x = P.randn((B, K), dtype, 100 + B)
            w = P.randn((N, K), dtype, 200 + N + K, 0.05)
            y = ext.gemv(x.to(dev), w.to(dev))
            assert y.shape == (B, N) and y.dtype == dtype
            want, a = P.gemv_ref(x, w)
            items.append((f"gemv B={B} N={N} K={K} {str(dtype)[6:]}", y, want, a, dtype))
    _check(items)


# ---------------------------------------------------------------------------
# Decode attention: head dims on and off the 64-lane grid, cache lengths
# around the 8 splits (S < 8 leaves splits empty), live length < allocation
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [BF16, FP16])
@pytest.mark.parametrize("D", [32, 64, 96, 128, 192, 256])
def test_attention_decode_edges(dev, D, dtype):
    from zero_transformer_amd import ops

    B, H = 2, 3
    slopes = reference.alibi_slopes(H)
    items = []
    for S in (1, 3, 7, 8, 9, 300):
        q = P.randn((B, H, 1, D), dtype, 300 + S)
        k = P.randn((B, H, S, D), dtype, 400 + S)
        v = P.randn((B, H, S, D), dtype, 500 + S)
        for sl in (slopes, None):
            got = ops.attention_decode(q.to(dev), k.to(dev), v.to(dev),
                                       None if sl is None else sl.to(dev))
            assert got.shape == (B, H, 1, D) and got.dtype == dtype
            want, a = P.attn_decode_ref(q, k, v, sl)
            tag = f"attention_decode D={D} S={S} {str(dtype)[6:]} alibi={sl is not None}"
            items.append((tag, got, want, a, dtype))
        if S in (1, 7, 9, 300):
            # live length S inside a larger cache whose dead tail is NaN
            pad = torch.full((B, H, 5, D), math.nan, dtype=dtype)
            kp, vp = torch.cat([k, pad], 2), torch.cat([v, pad], 2)
            used = torch.tensor([S], dtype=torch.int32, device=dev)
            got = ops.attention_decode(q.to(dev), kp.to(dev), vp.to(dev), slopes.to(dev), used)
            want, a = P.attn_decode_ref(q, kp, vp, slopes, S)
            items.append((f"attention_decode D={D} S={S} {str(dtype)[6:]} s_used", got, want, a, dtype))
    _check(items)
