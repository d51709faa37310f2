"""CPU checks of the parity checker itself (tests/_parity.py).

(a) The bounds are not too tight: the project's fp32 reference ops and an
    fp32 emulation of the kernels' own formulas (E[x^2] - mean^2 variance,
    exp(x - lse) gradient, x * sigmoid(2u) GELU, attention backward with its
    bf16 roundings of O, Pd and dS), rounded to the output type, pass at
    every shape the GPU tests use.
(b) The bounds have power: deliberately wrong results fail (three for the
    row kernels, five for attention backward).
"""

import math

import pytest
import torch

from zero_transformer_amd.ops import reference

from . import _parity as P
from ._parity import BF16, FP16, FP32

EPS = 1e-6


# ---------------------------------------------------------------------------
# fp32 emulations of the kernels' formulas
# ---------------------------------------------------------------------------


def ln_emul(x, w, dy, eps, cols=None):
    """Kernel formulas in fp32. `cols` restricts the row statistics to the
    first `cols` columns (the partial-wave bug) while keeping 1/C."""
    X, W, DY = x.float(), w.float(), dy.float()
    C = X.shape[-1]
    inv = torch.tensor(1.0 / C, dtype=torch.float32)
    Xs = X if cols is None else X[:, :cols]
    mu = Xs.sum(-1) * inv
    rstd = torch.rsqrt((Xs * Xs).sum(-1) * inv - mu * mu + eps)
    xh = (X - mu[:, None]) * rstd[:, None]
    y = xh * W
    g = DY * W
    gs, xs = (g, xh) if cols is None else (g[:, :cols], xh[:, :cols])
    s1 = gs.sum(-1, keepdim=True) * inv
    s2 = (gs * xs).sum(-1, keepdim=True) * inv
    dx = (g - s1 - xh * s2) * rstd[:, None]
    dw = (DY * xh).sum(0)
    dt = x.dtype
    return {"y": y.to(dt), "mean": mu, "rstd": rstd, "dx": dx.to(dt), "dw": dw.to(dt)}


def ce_emul(logits, targets, divisor, drop_last=0):
    """fp32 lse / loss / dlogits; `drop_last` leaves that many trailing
    columns out of lse (a lost last vector)."""
    X = logits.float()
    rows, V = X.shape
    lse = torch.logsumexp(X[:, : V - drop_last], -1)
    live = targets >= 0
    idx = targets.clamp(min=0)
    per = torch.where(live, lse - X.gather(1, idx[:, None])[:, 0], torch.zeros(()))
    div = divisor if divisor > 0 else rows
    scale = torch.tensor(1.0 / div, dtype=torch.float32)
    onehot = torch.zeros_like(X)
    onehot[torch.arange(rows), idx] = 1.0
    d = scale * (torch.exp(X - lse[:, None]) - onehot) * live[:, None]
    return {"lse": lse, "loss": per.sum() / div, "dlogits": d.to(logits.dtype)}


def gelu_emul(x, dy):
    X, DY = x.float(), dy.float()
    k0 = torch.tensor(P._K0, dtype=torch.float32)
    k1 = torch.tensor(P._K1, dtype=torch.float32)
    x2 = X * X
    u = k0 * (X + k1 * X * x2)
    sg = 1.0 / (1.0 + torch.exp(-2.0 * u))
    sech2 = 4.0 * sg * (1.0 - sg)
    grad = sg + 0.5 * X * sech2 * k0 * (1.0 + 3.0 * k1 * x2)
    return (X * sg).to(x.dtype), (DY * grad).to(x.dtype)


def attn_bwd_emul(q, k, v, do, slopes, keep, inv_keep, inject=None):
    """The attention kernels' formulas in fp32 with exactly their roundings:
    O, Pd and dS through bf16 before they are used, outputs to bf16.
    -> dq, dk, dv, o, lse. `inject` applies one deliberate error to the
    BACKWARD (the forward's o and lse stay right):
      "row"   dS of the last query row zeroed
      "keep"  keep bits of the last 4 keys of the last query row flipped
      "delta" delta summed over the first D - 8 columns
      "p"     p scaled by 1.01
      "alibi" bias one position off for the keys of the last 64-key tile
    """
    Q, K, V, DO = q.float(), k.float(), v.float(), do.float()
    B, H, T, D = Q.shape
    sc = torch.tensor(1.0 / math.sqrt(D), dtype=torch.float32)
    pos = torch.arange(T, dtype=torch.float32)
    rel = pos.view(1, T) - pos.view(T, 1)
    sl = (torch.zeros(H) if slopes is None else slopes.float()).view(1, H, 1, 1)
    causal = torch.ones(T, T, dtype=torch.bool).tril()
    QK = (Q @ K.transpose(-1, -2)) * sc
    S = (QK + sl * rel).masked_fill(~causal, -math.inf)
    lse = torch.logsumexp(S, -1)
    km = torch.ones(()) if keep is None else keep.float() * torch.tensor(inv_keep, dtype=torch.float32)
    O = ((torch.exp(S - lse[..., None]) * km).to(BF16).float() @ V).to(BF16)

    if inject == "alibi":
        rel = rel + (pos >= 64 * ((T - 1) // 64)).float().view(1, T)
        S = (QK + sl * rel).masked_fill(~causal, -math.inf)
    p = torch.exp(S - lse[..., None])
    if inject == "p":
        p = p * 1.01
    if inject == "keep":
        km = km.clone()
        km[..., -1, -4:] = (~keep[..., -1, -4:]).float() * torch.tensor(inv_keep, dtype=torch.float32)
    Pd = (p * km).to(BF16).float()
    dPd = (DO @ V.transpose(-1, -2)) * km
    cols = D - 8 if inject == "delta" else D
    delta = (DO[..., :cols] * O.float()[..., :cols]).sum(-1, keepdim=True)
    dS = sc * p * (dPd - delta)
    if inject == "row":
        dS[..., -1, :] = 0.0
    dS = dS.to(BF16).float()
    return {
        "dq": (dS @ K).to(BF16),
        "dk": (dS.transpose(-1, -2) @ Q).to(BF16),
        "dv": (Pd.transpose(-1, -2) @ DO).to(BF16),
        "o": O,
        "lse": lse,
    }


def _attn_case(T, D, p, qk_scale=1.0, alibi=True):
    B, H = P.ATTN_BH
    q, k, v, do = P.attn_bwd_inputs(B, H, T, D, qk_scale)
    slopes = reference.alibi_slopes(H) if alibi else None
    keep = reference.drop_mask(P.ATTN_SEED, B, H, T, p) if p > 0 else None
    inv = reference.drop_inv_keep(p)
    return (q, k, v, do, slopes, keep, inv), P.attn_bwd_ref(q, k, v, do, slopes, keep, inv)


def _check_all(got, want, dtype, names, tag):
    worst = 0.0
    for n in names:
        w, a = want[n]
        dt = FP32 if n in ("mean", "rstd", "lse", "loss") else dtype
        worst = max(worst, P.assert_within(got[n], w, dt, a, f"{tag} {n}"))
    return worst


# ---------------------------------------------------------------------------
# (a) not too tight
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("C,rows", P.LN_SHAPES)
def test_layernorm_bounds_admit_fp32(C, rows):
    x, w, dy = P.ln_inputs(C, rows, BF16)
    want = {**P.ln_ref(x, w, EPS), **P.ln_bwd_ref(dy, x, w, EPS)}
    _check_all(ln_emul(x, w, dy, EPS), want, BF16, ("y", "mean", "rstd", "dx", "dw"),
               f"ln-emul C={C} rows={rows}")
    # the project's fp32 reference op, forward and autograd backward
    xr = x.float().requires_grad_(True)
    wr = w.float().requires_grad_(True)
    yr = reference.layer_norm(xr, wr, EPS)
    yr.backward(dy.float())
    got = {"y": yr.detach().to(BF16), "dx": xr.grad.to(BF16), "dw": wr.grad.to(BF16)}
    _check_all(got, want, BF16, ("y", "dx", "dw"), f"ln-ref C={C} rows={rows}")


def test_layernorm_bounds_admit_fp32_output_and_offset():
    x, w, dy = P.ln_inputs(264, 3, FP32)
    want = {**P.ln_ref(x, w, EPS), **P.ln_bwd_ref(dy, x, w, EPS)}
    _check_all(ln_emul(x, w, dy, EPS), want, FP32, ("y", "mean", "rstd", "dx", "dw"), "ln-emul fp32")
    for C in (768, 2048, 264):
        x, w, dy = P.ln_inputs(C, 3, BF16, offset=64.0)
        want = {**P.ln_ref(x, w, EPS), **P.ln_bwd_ref(dy, x, w, EPS)}
        got = ln_emul(x, w, dy, EPS)
        assert all(torch.isfinite(t).all() for t in got.values())
        _check_all(got, want, BF16, ("y", "mean", "rstd", "dx", "dw"), f"ln-emul offset C={C}")


@pytest.mark.parametrize("dtype", [BF16, FP16])
@pytest.mark.parametrize("C", P.ADD_LN_KERNEL_C + P.ADD_LN_TORCH_C)
def test_add_ln_bounds_admit_fp32(C, dtype):
    x, w, _ = P.ln_inputs(C, 3, dtype)
    h = P.randn((3, C), dtype, 77)
    v = x.float() + h.float()
    P.assert_within(v.to(dtype), P.f64(x) + P.f64(h), dtype, 0.0, f"add_ln y C={C}")
    want, a = P.ln_ref(P.f64(x) + P.f64(h), w, EPS)["y"]
    got = ln_emul(v, w.float(), v, EPS)["y"].to(dtype)
    P.assert_within(got, want, dtype, a, f"add_ln ln C={C}")


@pytest.mark.parametrize("ignore", [False, True])
@pytest.mark.parametrize("V,rows,dtype", P.CE_SHAPES)
def test_cross_entropy_bounds_admit_fp32(V, rows, dtype, ignore):
    logits, targets = P.ce_inputs(V, rows, dtype, ignore)
    divisor = int((targets >= 0).sum()) if ignore else 0
    want = P.ce_ref(logits, targets, divisor)
    got = ce_emul(logits, targets, divisor)
    assert all(torch.isfinite(t).all() for t in got.values())
    _check_all(got, want, dtype, ("lse", "loss", "dlogits"), f"ce-emul V={V} rows={rows}")
    live = want["live"]
    sums = P.f64(got["dlogits"]).sum(-1).abs()
    assert bool((sums[live] <= want["rowsum_tol"][live]).all())
    # reference.cross_entropy means over the counted rows
    lr = logits.float().requires_grad_(True)
    loss = reference.cross_entropy(lr, targets)
    loss.backward()
    want = P.ce_ref(logits, targets, int((targets >= 0).sum()))
    got = {"loss": loss.detach(), "dlogits": lr.grad.to(dtype)}
    _check_all(got, want, dtype, ("loss", "dlogits"), f"ce-ref V={V} rows={rows}")


@pytest.mark.parametrize("gdtype", [BF16, FP32])
@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("step0", [1, 10000])
def test_adamw_bounds_admit_fp32(gdtype, wd, step0):
    n = 4099
    p = P.randn((n,), FP32, 1)
    m = torch.zeros(n) if step0 == 1 else P.randn((n,), FP32, 2, 0.1)
    v = torch.zeros(n) if step0 == 1 else P.randn((n,), FP32, 3, 0.1).abs()
    hp = (1e-3, 0.9, 0.95, 1e-8, wd, 1.0, 0.5)
    for i in range(3):
        g = P.randn((n,), gdtype, 10 + i, 3.0)  # * 0.5 grad_scale: many exceed the clip
        (wp, ap), (wm, am), (wv, av) = P.adamw_ref(p, g, m, v, step0 + i, *hp)
        reference.adamw_update(p, g, m, v, step0 + i, *hp)
        P.assert_within(p, wp, FP32, ap, "adamw p")
        P.assert_within(m, wm, FP32, am, "adamw m")
        P.assert_within(v, wv, FP32, av, "adamw v")


@pytest.mark.parametrize("n,dtype", [(8 * (2048 * 256 + 3), BF16), (1003, BF16), (1003, FP32),
                                     (1024, FP16)])
def test_gelu_bounds_admit_fp32(n, dtype):
    # F.gelu's 0.5 x (1 + tanh u) form cancels in the negative tail, so the
    # kernels' own x * sigmoid(2u) form is what gets emulated here
    x, dy = P.gelu_inputs(n, dtype)
    (wy, ay), (wd, ad) = P.gelu_ref(x, dy)
    y, dx = gelu_emul(x, dy)
    assert torch.isfinite(y).all() and torch.isfinite(dx).all()
    P.assert_within(y, wy, dtype, ay, f"gelu y n={n}")
    P.assert_within(dx, wd, dtype, ad, f"gelu dx n={n}")
    # reference.gelu agrees where its form does not cancel
    body = P.f64(x).abs() <= 3.0
    yr = reference.gelu(x.float()).to(dtype)
    if dtype != FP32:
        P.assert_within(yr[body], wy[body], dtype, ay[body], f"gelu-ref y n={n}")


@pytest.mark.parametrize("dtype", [BF16, FP16])
def test_gemv_and_decode_bounds_admit_fp32(dtype):
    x = P.randn((16, 1536), dtype, 1)
    w = P.randn((1023, 1536), dtype, 2, 0.05)
    want, a = P.gemv_ref(x, w)
    P.assert_within((x.float() @ w.float().T).to(dtype), want, dtype, a, "gemv")
    for D, S in ((32, 1), (96, 9), (256, 300)):
        q = P.randn((2, 3, 1, D), dtype, 3)
        k = P.randn((2, 3, S, D), dtype, 4)
        v = P.randn((2, 3, S, D), dtype, 5)
        sl = reference.alibi_slopes(3)
        want, a = P.attn_decode_ref(q, k, v, sl)
        bias = sl.view(1, 3, 1, 1) * (torch.arange(S, dtype=torch.float32) - (S - 1))
        scores = q.float() @ k.float().transpose(-1, -2) / math.sqrt(D) + bias
        got = (torch.softmax(scores, -1) @ v.float()).to(dtype)
        P.assert_within(got, want, dtype, a, f"decode D={D} S={S}")


_ATTN_SHAPES = sorted(set(P.ATTN_BWD_TWO + P.ATTN_BWD_FUSED + P.ATTN_BWD_BIG))
_ATTN_WORST = {}


def _attn_emul_check(args, want, tag):
    got = attn_bwd_emul(*args)
    assert all(torch.isfinite(t.float()).all() for t in got.values())
    for n in ("o", "lse"):
        r = P.worst_abs_ratio(got[n], *want[n])
        print(f"[parity] {tag} {n}: worst error/bound = {r:.3f}")
        assert r <= 1.0
    for n in ("dq", "dk", "dv"):
        P.assert_within(got[n], want[n][0], BF16, want[n][1], f"attn-emul-{n} {tag}", _ATTN_WORST)


@pytest.fixture(scope="module", autouse=True)
def _attn_summary():
    yield
    for op, r in sorted(_ATTN_WORST.items()):
        print(f"[parity-summary] {op}: worst error/bound = {r:.3f}")


@pytest.mark.parametrize("T,D,p,qk_scale,alibi", _ATTN_SHAPES)
def test_attn_bwd_bounds_admit_emulation(T, D, p, qk_scale, alibi):
    """Every (T, D, p, scale) of test_gpu_attn_bwd_edges.py: the fp32
    emulation with the kernels' bf16 roundings stays within the bound."""
    args, want = _attn_case(T, D, p, qk_scale, alibi)
    _attn_emul_check(args, want, f"T={T} D={D} p={p} x{qk_scale:g} alibi={int(alibi)}")


@pytest.mark.parametrize("B,H,T,D", P.ATTN_DELTA_STRIDE)
def test_attn_bwd_bounds_admit_emulation_long(B, H, T, D):
    """The delta grid-stride shapes, on the two (b, h) planes the GPU test
    checks (the first and the last)."""
    q, k, v, do = P.attn_bwd_inputs(B, H, T, D)
    slopes = reference.alibi_slopes(H)
    for b, h in ((0, 0), (B - 1, H - 1)):
        cut = lambda t: t[b:b + 1, h:h + 1]
        args = (cut(q), cut(k), cut(v), cut(do), slopes[h:h + 1], None, 1.0)
        _attn_emul_check(args, P.attn_bwd_ref(*args), f"T={T} D={D} plane=({b},{h})")


# ---------------------------------------------------------------------------
# (b) power
# ---------------------------------------------------------------------------


@pytest.fixture(scope="module", params=[(300, 128, 0.3), (257, 96, 0.1)], ids=str)
def attn_power_case(request):
    return _attn_case(*request.param)


@pytest.mark.parametrize("inject", ["row", "keep", "delta", "p", "alibi"])
def test_bound_rejects_wrong_attention_backward(attn_power_case, inject):
    """Five errors a tile-edge or indexing bug would make; each must exceed
    the bound on at least one of dq / dk / dv."""
    args, want = attn_power_case
    bad = attn_bwd_emul(*args, inject=inject)
    r = {n: P.worst_ratio(bad[n], want[n][0], BF16, want[n][1]) for n in ("dq", "dk", "dv")}
    print(f"[parity] inject {inject}: " + " ".join(f"{n}={v:.2f}" for n, v in r.items()))
    assert max(r.values()) > 1.0, f"{inject} passed: {r}"


@pytest.mark.parametrize("C,whole", [(768, 512), (1280, 1024)])
def test_bound_rejects_partial_wave_layernorm(C, whole):
    """Row statistics over the whole-wave columns only (what a C/8-thread
    block with a dropped trailing wave computes) must fail."""
    x, w, dy = P.ln_inputs(C, 3, BF16)
    want = {**P.ln_ref(x, w, EPS), **P.ln_bwd_ref(dy, x, w, EPS)}
    bad = ln_emul(x, w, dy, EPS, cols=whole)
    for n in ("y", "mean", "rstd", "dx"):
        dt = FP32 if n in ("mean", "rstd") else BF16
        r = P.worst_ratio(bad[n], want[n][0], dt, want[n][1])
        assert r > 1.0, f"{n}: wrong statistics passed at ratio {r}"


@pytest.mark.parametrize("V", [2040, 2056])
def test_bound_rejects_lse_without_last_vector(V):
    logits, targets = P.ce_inputs(V, 5, BF16)
    want = P.ce_ref(logits, targets)
    bad = ce_emul(logits, targets, 0, drop_last=8)
    assert P.worst_ratio(bad["lse"], want["lse"][0], FP32, want["lse"][1]) > 1.0
    assert P.worst_ratio(bad["loss"], want["loss"][0], FP32, want["loss"][1]) > 1.0


def test_bound_rejects_dropout_mask_without_high_word():
    p, seed = 0.3, 777
    inv = reference.drop_inv_keep(p)
    for n, must_fail in ((262144, False), (262144 + 4096, True)):
        x = P.randn((n,), BF16, 1)
        h = P.randn((n,), BF16, 2)
        want, a = P.residual_ref(x, h, reference.residual_drop_mask(seed, n, p), inv)
        bad_keep = P.residual_mask_lowword_only(seed, n, p)
        bad = (x.float() + h.float() * bad_keep.float() * inv).to(BF16)
        r = P.worst_ratio(bad, want, BF16, a)
        assert (r > 1.0) == must_fail, f"n={n}: ratio {r}"


def test_checker_rejects_nonfinite_and_shape():
    want = torch.ones(4, dtype=torch.float64)
    assert P.worst_ratio(torch.ones(4), want, FP32) == 0.0
    assert math.isinf(P.worst_ratio(torch.tensor([1.0, math.nan, 1.0, 1.0]), want, FP32))
    assert math.isinf(P.worst_ratio(torch.ones(3), want, FP32))
    assert P.worst_ratio(torch.full((4,), 1.0 + 2.0 ** -6), want, BF16) > 1.0
    assert P.worst_ratio(torch.full((4,), 1.0 + 2.0 ** -8), want, BF16) <= 1.0
