"""Float64 references and one derived error bound for the HIP kernel parity
tests (tests/test_gpu_ops_edges.py, tests/test_gpu_attn_bwd_edges.py, checked
on CPU by tests/test_parity_helpers.py).

Every reference is computed in float64 from the exact bf16 / fp16 / fp32
values the kernel receives. The one checker is

    |got - want| <= rel(dtype) * |want| + tiny(dtype) + abs_term   (elementwise)

* rel is ONE ulp of the output type (2^-7 bf16, 2^-10 fp16, 1e-6 fp32): twice
  the half-ulp of a correctly rounded result, because the kernels round an
  fp32 value that already carries error (half an ulp leaves no margin: an
  fp32 emulation of LayerNorm / cross-entropy reaches 0.99 of 2^-8).
* tiny is one ulp at the bottom of the format (its subnormal spacing), where
  the spacing stops being relative.
* abs_term covers fp32 accumulation and the fast exp / log: 1e-5 x the sum of
  |terms| of the sum that produces the element, taken from the float64
  reference. Each reference below returns its abs_term next to the value and
  says where it comes from.

The bounds are derived from the formats and the formulas, never fitted to
what a kernel returns. (The training attention's o and lse keep the absolute
bounds of tests/test_gpu_attn_fwd_edges.py instead: see attn_bwd_ref.)
"""

from __future__ import annotations

import math

import numpy as np
import torch

BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32

REL = {BF16: 2.0 ** -7, FP16: 2.0 ** -10, FP32: 1e-6}
TINY = {BF16: 2.0 ** -133, FP16: 2.0 ** -24, FP32: 2.0 ** -149}
ACC = 1e-5  # fp32 accumulation / fast-math factor on the sum of |terms|


def f64(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to("cpu", torch.float64)


def worst_ratio(got, want, dtype, abs_term=0.0) -> float:
    """max over elements of error / bound (inf if any `got` is not finite
    or shapes differ); <= 1 means within the bound."""
    g, w = f64(got), f64(want)
    if g.shape != w.shape:
        return math.inf
    if g.numel() == 0:
        return 0.0
    a = abs_term if isinstance(abs_term, float) else f64(abs_term)
    bound = REL[dtype] * w.abs() + TINY[dtype] + a
    ratio = (g - w).abs() / bound
    ratio = torch.nan_to_num(ratio, nan=math.inf, posinf=math.inf)
    return float(ratio.max())


def assert_within(got, want, dtype, abs_term=0.0, name="", worst=None) -> float:
    """Assert the bound; print (and optionally record) the worst ratio."""
    r = worst_ratio(got, want, dtype, abs_term)
    print(f"[parity] {name}: worst error/bound = {r:.3f}")
    if worst is not None:
        key = name.split(" ")[0]
        worst[key] = max(worst.get(key, 0.0), r)
    assert r <= 1.0, f"{name}: error is {r:.3f} x the bound"
    return r


def randn(shape, dtype, seed, scale=1.0, offset=0.0) -> torch.Tensor:
    """Fixed-seed CPU normal sample, rounded to `dtype`."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + offset).to(dtype)


# ---------------------------------------------------------------------------
# Shapes shared by the CPU self-check and the GPU tests
# ---------------------------------------------------------------------------

# (C, rows): see the table in test_gpu_ops_edges.py
LN_SHAPES = (
    [(512, r) for r in (1, 3, 4100)]
    + [(C, r) for C in (768, 1280, 1536, 8192, 8200) for r in (1, 3)]
    + [(264, r) for r in (1, 3, 2050)]
    + [(100, r) for r in (1, 3)]
)
ADD_LN_KERNEL_C = (512, 768, 1280, 1536, 8192)  # C % 8 == 0, 64 <= C/8 <= 1024
ADD_LN_TORCH_C = (8200, 264, 100)  # ops.add_ln routes these to torch

# (V, rows, dtype)
CE_SHAPES = (
    [(V, r, BF16) for V in (8, 2040, 2056) for r in (1, 5)]
    + [(50304, 8, BF16), (64, 4100, BF16)]
    + [(1001, r, BF16) for r in (1, 5)]
    + [(1000, r, FP32) for r in (1, 5)]
)

GELU_SPECIALS = [s * v for v in (0.0, 1e-3, 3.0, 10.0, 30.0, 100.0) for s in (1.0, -1.0)]


# ---------------------------------------------------------------------------
# LayerNorm (bias-free)
# ---------------------------------------------------------------------------


def ln_inputs(C, rows, dtype, offset=0.0, seed=0):
    x = randn((rows, C), dtype, 1000 + seed, offset=offset)
    w = randn((C,), dtype, 2000 + seed)
    dy = randn((rows, C), dtype, 3000 + seed)
    return x, w, dy


def ln_ref(x, w, eps):
    """-> {name: (want, abs_term)} for y, mean, rstd.

    y = (x - mean) * rstd * w: the only sum behind an element is the mean,
    whose fp32 error (<= ACC * mean|x|, far below 1) enters as
    d_mean * rstd * w  ->  ACC * |w|.
    mean: ACC * mean|x| (sum of |terms| / C).
    rstd: 1e-5 relative for centred rows. var = E[x^2] - mean^2 is a
    difference, so its fp32 error is ACC * (E[x^2] + mean^2), i.e. relative
    ACC * (E[x^2] + mean^2) / (2 var) on rstd; that factor is ~0.5 for
    centred rows (the max() keeps 1e-5 there) and grows with a common offset.
    """
    X, W = f64(x), f64(w)
    mean = X.mean(-1)
    ex2 = (X * X).mean(-1)
    var = ((X - mean[:, None]) ** 2).mean(-1)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (X - mean[:, None]) * rstd[:, None] * W
    cancel = torch.clamp((ex2 + mean * mean) / (2.0 * (var + eps)), min=1.0)
    return {
        "y": (y, ACC * W.abs().expand_as(y)),
        "mean": (mean, ACC * X.abs().mean(-1)),
        "rstd": (rstd, ACC * rstd * cancel),
    }


def ln_bwd_ref(dy, x, w, eps):
    """-> {name: (want, abs_term)} for dx, dw.

    dx = (g - s1 - xhat * s2) * rstd with g = w * dy, s1 = mean(g),
    s2 = mean(g * xhat): ACC * (|g| + |s1| + |xhat * s2|) * rstd.
    dw = sum_rows dy * xhat: ACC * sum_rows |dy * xhat|.
    Both read the saved rstd. Where a common offset makes E[x^2] - mean^2
    cancel, rstd carries the extra relative error ACC * (cancel - 1) of
    ln_ref (0 for centred rows); it enters g - s1 once and xhat * s2 three
    times (xhat twice, the outer factor once), and dw once.
    """
    X, W, DY = f64(x), f64(w), f64(dy)
    mean = X.mean(-1, keepdim=True)
    var = ((X - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (X - mean) * rstd
    g = DY * W
    s1 = g.mean(-1, keepdim=True)
    s2 = (g * xh).mean(-1, keepdim=True)
    dx = (g - s1 - xh * s2) * rstd
    dw = (DY * xh).sum(0)
    ex2 = (X * X).mean(-1, keepdim=True)
    extra = ACC * (torch.clamp((ex2 + mean * mean) / (2.0 * (var + eps)), min=1.0) - 1.0)
    abs_dx = ACC * (g.abs() + s1.abs() + (xh * s2).abs()) * rstd
    abs_dx = abs_dx + extra * (g.abs() + s1.abs() + 3.0 * (xh * s2).abs()) * rstd
    abs_dw = ((ACC + extra) * (DY * xh).abs()).sum(0)
    return {"dx": (dx, abs_dx), "dw": (dw, abs_dw)}


# ---------------------------------------------------------------------------
# Cross entropy
# ---------------------------------------------------------------------------


def ce_inputs(V, rows, dtype, ignore=False, seed=0):
    """Logits ~ 3 * N(0,1) with the edge rows of the issue, and targets.

    row 0: target column 0.            row 1: target column V-1.
    row 2: +60 spike, target inside the last 8-column vector.
    row 3: all logits equal.           row 4: a block of -inf logits.
    With one row, that row carries the target V-1. `ignore` sets every
    third row's target (from row 1) to -1.
    """
    g = torch.Generator().manual_seed(4000 + seed)
    logits = (torch.randn(rows, V, generator=g) * 3.0).to(dtype)
    targets = torch.randint(0, V, (rows,), generator=g)
    targets[0] = 0 if rows > 1 else V - 1
    if rows >= 5:
        targets[1] = V - 1
        logits[2, V // 3] += 60.0
        targets[2] = V - 3
        logits[3] = 1.5
        logits[4, : max(V // 4, 2)] = -math.inf
        targets[4] = V - 1
    if ignore:
        targets[1::3] = -1
    return logits, targets


def ce_ref(logits, targets, divisor=0, dloss=1.0):
    """-> dict of (want, abs_term) for lse, loss, dlogits, plus scale and p.

    lse and loss: 1e-4 absolute (fast exp / log of an fp32 sum).
    dlogits = scale * (p - onehot), p = exp(x - lse): ACC * scale * p.
    rowsum_tol: each counted row of dlogits sums to 0 up to the rounding of
    its entries, half an ulp u each: the V entries scale * p_c give at most
    V * u * scale * max p, and the target entry scale * (p_t - 1), which is
    the large one, adds u * scale * (1 - p_t). (Without that last term a
    correctly rounded all-equal row already reaches 1.35 x the tolerance.)
    fp32 entries also carry the lse budget, scale * 1e-4.
    """
    X = f64(logits)
    T = targets.cpu()
    rows = X.shape[0]
    lse = torch.logsumexp(X, -1)
    live = T >= 0
    idx = T.clamp(min=0)
    picked = X.gather(1, idx[:, None])[:, 0]
    per_row = torch.where(live, lse - picked, torch.zeros_like(lse))
    div = float(divisor) if divisor > 0 else float(rows)
    loss = per_row.sum() / div
    scale = dloss / div
    p = torch.exp(X - lse[:, None])
    onehot = torch.zeros_like(X)
    onehot[torch.arange(rows), idx] = 1.0
    d = scale * (p - onehot) * live[:, None].double()
    u = 2.0 ** -24 if logits.dtype == FP32 else REL[logits.dtype] / 2.0
    p_t = p.gather(1, idx[:, None])[:, 0]
    rowsum_tol = u * scale * (X.shape[1] * p.amax(-1) + (1.0 - p_t))
    if logits.dtype == FP32:
        rowsum_tol = rowsum_tol + 1e-4 * scale
    return {
        "rowsum_tol": rowsum_tol,
        "lse": (lse, 1e-4),
        "loss": (loss, 1e-4),
        "dlogits": (d, ACC * scale * p * live[:, None].double()),
        "scale": scale,
        "p": p,
        "live": live,
    }


# ---------------------------------------------------------------------------
# AdamW (documented update of ops.adamw_step)
# ---------------------------------------------------------------------------


def adamw_ref(p, g, m, v, step, lr, beta1, beta2, eps, wd, clip, gscale):
    """One step in float64 from the kernel's fp32 hyper-parameters.
    -> new (p, m, v) each as (want, abs_term); inputs are not modified.

    m = b1*m + (1-b1)*g, v likewise: ACC * (sum of |terms|).
    p = p - lr * (adam + wd * p): ACC * lr * (|adam| + wd * |p|) plus the
    m / v errors of this step carried through adam.
    Tests call it once per step on the state the kernel is about to read, so
    no error carries over from earlier steps.
    """
    f = lambda s: float(np.float32(s))
    lr, beta1, beta2, eps, wd, clip, gscale = map(f, (lr, beta1, beta2, eps, wd, clip, gscale))
    P, G, M, V = f64(p), f64(g), f64(m), f64(v)
    G = G * gscale
    if clip != 0.0:
        G = G.clamp(-clip, clip)
    m_abs = ACC * (beta1 * M.abs() + (1 - beta1) * G.abs())
    v_abs = ACC * (beta2 * V + (1 - beta2) * G * G)
    M = beta1 * M + (1 - beta1) * G
    V = beta2 * V + (1 - beta2) * G * G
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    den = torch.sqrt(V / bc2) + eps
    adam = (M / bc1) / den
    upd = adam + wd * P
    # d(adam) = dm / (bc1 den) + |adam| * 0.5 * dv / v, and dv / v = ACC
    d_adam = m_abs / (bc1 * den) + 0.5 * ACC * adam.abs()
    p_abs = lr * d_adam + ACC * lr * (adam.abs() + wd * P.abs())
    return (P - lr * upd, p_abs), (M, m_abs), (V, v_abs)


# ---------------------------------------------------------------------------
# Residual-add + dropout
# ---------------------------------------------------------------------------


def residual_ref(x, h, keep, inv_keep):
    """y = x + h * keep * inv_keep: ACC * (|x| + |h * inv_keep|)."""
    X, H = f64(x), f64(h)
    k = keep.cpu().double() * float(np.float32(inv_keep))
    return X + H * k, ACC * (X.abs() + (H * k).abs())


def residual_mask_lowword_only(seed: int, n: int, p: float) -> torch.Tensor:
    """A deliberately WRONG residual-dropout mask: the hash of
    reference.residual_drop_mask with the high word (i4 >> 16) forced to 0.
    Agrees with the right mask for n <= 262144 only."""
    thr = int(p * 256.0 + 0.5)

    def mix32(x):
        x = x.astype(np.uint32, copy=True)
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x85EBCA6B)
        x ^= x >> np.uint32(13)
        x *= np.uint32(0xC2B2AE35)
        x ^= x >> np.uint32(16)
        return x

    i4 = np.arange((n + 3) // 4, dtype=np.uint64)
    lo = (i4 & np.uint64(0xFFFF)).astype(np.uint32)
    with np.errstate(over="ignore"):
        bits = mix32(np.uint32(seed) ^ (lo * np.uint32(0x85EBCA6B)))
    by = np.stack([(bits >> np.uint32(8 * e)) & np.uint32(0xFF) for e in range(4)], -1)
    return torch.from_numpy((by >= np.uint32(thr)).reshape(-1)[:n].copy())


# ---------------------------------------------------------------------------
# GELU (tanh approximation, written as x * sigmoid(2u))
# ---------------------------------------------------------------------------

_K0 = math.sqrt(2.0 / math.pi)
_K1 = 0.044715
_EXP_ERR = 5e-7  # fast exp: argument product rounding + ~1 ulp, x4 margin
_FLUSH = 2.0 ** -125  # sigmoid below fp32's normal range may flush to 0


def gelu_inputs(n, dtype, seed=0):
    """2 * N(0,1) with the special values at both ends of the tensor (the
    tail is what the last grid-stride step / scalar path sees)."""
    x = randn((n,), dtype, 5000 + seed, scale=2.0)
    sp = torch.tensor(GELU_SPECIALS).to(dtype)
    x[: sp.numel()] = sp
    x[-sp.numel():] = sp
    dy = randn((n,), dtype, 6000 + seed)
    return x, dy


def gelu_ref(x, dy=None):
    """-> (y, abs_y), (dx, abs_dx).

    y = x * s, s = sigmoid(2u), u = k0 * (x + k1 x^3). The kernel gets s from
    a fast exp whose relative error is ~1.2e-7 * (1 + |2u|) (the argument is
    rounded to fp32 before v_exp); d s = s (1 - s) * that, so
    abs_y = _EXP_ERR * (1 + |2u|) * |x| * s (1 - s), plus |x| * 2^-125 where
    s itself is below fp32's normal range.
    dx = dy * (s + 2 x u' s (1 - s)), u' = k0 (1 + 3 k1 x^2): the same exp
    error through both terms, and 1 - s formed in fp32 (absolute 2^-24, times
    the factor 4 of sech^2 and the 0.5 x u' in front).
    """
    X = f64(x)
    u2 = 2.0 * _K0 * (X + _K1 * X ** 3)
    s = torch.sigmoid(u2)
    s1 = torch.sigmoid(-u2)  # 1 - s without cancellation
    y = X * s
    e = _EXP_ERR * (1.0 + u2.abs())
    abs_y = e * X.abs() * s * s1 + _FLUSH * X.abs()
    if dy is None:
        return (y, abs_y), None
    up = _K0 * (1.0 + 3.0 * _K1 * X * X)
    xu = (X * up).abs()
    grad = s + 2.0 * X * up * s * s1
    DY = f64(dy).abs()
    abs_dx = DY * (e * s * s1 * (1.0 + 2.0 * xu) + 2.0 ** -22 * xu * s + _FLUSH * (1.0 + 2.0 * xu))
    return (y, abs_y), (f64(dy) * grad, abs_dx)


# ---------------------------------------------------------------------------
# Decode GEMV and decode attention
# ---------------------------------------------------------------------------


def gemv_ref(x, w):
    """y = x @ w^T: ACC * sum_k |x||w|."""
    X, W = f64(x), f64(w)
    return X @ W.T, ACC * (X.abs() @ W.abs().T)


def attn_decode_ref(q, k, v, slopes, s_used=None):
    """q (B,H,1,D), k/v (B,H,S_alloc,D); only the first s_used keys are read.

    score_j = q.k_j / sqrt(D) + slope * (j - (S-1)) carries an fp32 error of
    ds = ACC * max_j (sum_d |q||k| / sqrt(D) + |bias_j|); p_j = softmax has
    relative error 2 ds, so out = sum_j p_j v_j gets
    (ACC + 2 ds) * sum_j p_j |v_j|.
    """
    S = k.shape[2] if s_used is None else int(s_used)
    Q, K, V = f64(q), f64(k)[:, :, :S], f64(v)[:, :, :S]
    H, D = Q.shape[1], Q.shape[3]
    sc = 1.0 / math.sqrt(D)
    scores = (Q @ K.transpose(-1, -2)) * sc  # (B,H,1,S)
    mag = (Q.abs() @ K.abs().transpose(-1, -2)) * sc
    if slopes is not None:
        pos = torch.arange(S, dtype=torch.float64) - (S - 1)
        bias = f64(slopes).view(1, H, 1, 1) * pos.view(1, 1, 1, S)
        scores = scores + bias
        mag = mag + bias.abs()
    p = torch.softmax(scores, -1)
    ds = ACC * mag.amax(-1, keepdim=True)
    return p @ V, (ACC + 2.0 * ds) * (p @ V.abs())


# ---------------------------------------------------------------------------
# Training attention, forward + backward (causal, ALiBi, dropout on P)
# ---------------------------------------------------------------------------

U_BF16 = 2.0 ** -8  # half an ulp: relative error of one rounding to bf16
# o / lse: the absolute bounds of tests/test_gpu_attn_fwd_edges.py
ATTN_O_TOL = 3e-2
ATTN_O_TOL_MASK = 4e-2
ATTN_LSE_TOL = 1e-4

ATTN_BH = (2, 3)
ATTN_SEED = 12345
ATTN_T = (40, 65, 129, 257, 320)
# (T, D, p, q/k scale, alibi): see the table in test_gpu_attn_bwd_edges.py
ATTN_BWD_TWO = (
    [(T, D, 0.0, 1.0, True) for D in (32, 64, 96, 128) for T in ATTN_T]
    + [(T, D, 0.3, 1.0, True) for D in (32, 64, 96, 128) for T in (65, 257)]
    + [(129, 96, 0.1, 1.0, True)]
)
ATTN_BWD_FUSED = (
    [(T, 128, 0.0, 1.0, True) for T in (40, 65, 257, 320, 576)]
    + [(T, 128, 0.3, 1.0, True) for T in (65, 257, 576)]
)
ATTN_BWD_BIG = [(320, 128, 0.0, 4.0, True), (320, 128, 0.0, 4.0, False)]
# (B, H, T, D): rows = B * H * T just past one pass of each delta kernel
ATTN_DELTA_STRIDE = [(1, 8, 1040, 32), (4, 16, 1040, 64)]


def attn_bwd_inputs(B, H, T, D, qk_scale=1.0):
    """q, k, v, do as (B, H, T, D) bf16, fixed per shape and scale."""
    seed = 7000 + 8 * (T * 131 + D) + (4 if qk_scale != 1.0 else 0)
    q = randn((B, H, T, D), BF16, seed, qk_scale)
    k = randn((B, H, T, D), BF16, seed + 1, qk_scale)
    v = randn((B, H, T, D), BF16, seed + 2)
    do = randn((B, H, T, D), BF16, seed + 3)
    return q, k, v, do


def worst_abs_ratio(got, want, tol) -> float:
    """max |got - want| / tol (inf if not finite or shapes differ)."""
    g, w = f64(got), f64(want)
    if g.shape != w.shape:
        return math.inf
    ratio = torch.nan_to_num((g - w).abs() / tol, nan=math.inf, posinf=math.inf)
    return float(ratio.max())


def attn_bwd_ref(q, k, v, do, slopes, keep=None, inv_keep=1.0):
    """q, k, v, do (B, H, T, D); slopes (H,) or None; keep bool (B, H, T, T) or
    None. -> {name: (want, abs_term)} for o, lse, dq, dk, dv, each (B, H, T, D)
    (lse (B, H, T)). Closed formulas in float64, no autograd:

        S = scale Q K^T + slope (j - i), causal;   P = softmax(S)
        Pd = P keep inv_keep;          O = Pd V
        dPd = (dO V^T) keep inv_keep;  delta = rowsum(P dPd)  (= rowsum(dO O))
        dS = scale P (dPd - delta)
        dV = Pd^T dO;   dQ = dS K;   dK = dS^T Q

    o and lse carry the forward edge tests' ABSOLUTE bounds as abs_term (3e-2,
    4e-2 with a mask; 1e-4) and are checked with worst_abs_ratio, so they are
    no wider here than there. dq, dk, dv go through worst_ratio; their
    abs_term follows from what the kernels (ops/csrc/attention_bwd.hip) round,
    with u = 2^-8 one rounding to bf16:

    * p is recomputed in fp32 as exp2(s scale2 + slope2 (j - i) - lse2) from
      the forward's lse. An absolute error e of the exponent is a relative
      error e of p: the saved lse gives ATTN_LSE_TOL, the fp32 score sum and
      the two fp32 additions give ACC x (scale (|Q||K|^T)_ij + |bias_ij|).
      (The bias magnitude is not in the issue's list; it is the other operand
      of the same fp32 sum, as in attn_decode_ref.)
          eps_ij = 1e-4 + ACC (scale (|Q||K|^T)_ij + |slope (j - i)|)
    * Pd is rounded to bf16 for its MFMA:  dv: ((u + eps) |Pd|)^T |dO|
    * delta = rowsum(dO O) reads the bf16 O of the forward (u |O|), which the
      forward formed from bf16-rounded P (another u (|Pd||V|)):
          E_delta_i = 2u sum_d |dO_id| (|Pd||V|)_id
    * dP is an fp32 sum of D products: E_dP = ACC (|dO||V|^T) keep inv_keep
      (also not in the issue's list; a few per cent of the u term).
    * dS is rounded to bf16 for its MFMAs:
          E_dS = (u + eps) |dS| + scale P (E_delta + E_dP)
                 + eps scale P (|dPd| + |delta|)
      dq: E_dS |K|;   dk: E_dS^T |Q|.
    The fp32 accumulation of the three output products (ACC x the same sums of
    |terms|) is far below their u terms and is covered by eps >= 1e-4; the
    fused kernel's f32 atomics add dQ partial sums in fp32 likewise.
    Nothing here is fitted to what a kernel returns.
    """
    Q, K, V, DO = f64(q), f64(k), f64(v), f64(do)
    B, H, T, D = Q.shape
    sc = 1.0 / math.sqrt(D)
    S = (Q @ K.transpose(-1, -2)) * sc
    mag = (Q.abs() @ K.abs().transpose(-1, -2)) * sc
    if slopes is not None:
        pos = torch.arange(T, dtype=torch.float64)
        bias = f64(slopes).view(1, H, 1, 1) * (pos.view(1, T) - pos.view(T, 1))
        S = S + bias
        mag = mag + bias.abs()
    causal = torch.ones(T, T, dtype=torch.bool).tril()
    S = S.masked_fill(~causal, -math.inf)
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    if keep is None:
        km = torch.ones((), dtype=torch.float64)
    else:
        km = keep.cpu().double() * float(np.float32(inv_keep))
    Pd = P * km
    O = Pd @ V
    dPd = (DO @ V.transpose(-1, -2)) * km
    delta = (P * dPd).sum(-1, keepdim=True)
    dS = sc * P * (dPd - delta)
    dV = Pd.transpose(-1, -2) @ DO
    dQ = dS @ K
    dK = dS.transpose(-1, -2) @ Q

    u = U_BF16
    eps = ATTN_LSE_TOL + ACC * mag
    e_delta = 2.0 * u * (DO.abs() * (Pd.abs() @ V.abs())).sum(-1, keepdim=True)
    e_dp = ACC * (DO.abs() @ V.abs().transpose(-1, -2)) * km
    e_ds = (u + eps) * dS.abs() + sc * P * (e_delta + e_dp) + eps * sc * P * (dPd.abs() + delta.abs())
    return {
        "o": (O, ATTN_O_TOL if keep is None else ATTN_O_TOL_MASK),
        "lse": (lse, ATTN_LSE_TOL),
        "dq": (dQ, e_ds @ K.abs()),
        "dk": (dK, e_ds.transpose(-1, -2) @ Q.abs()),
        "dv": (dV, ((u + eps) * Pd.abs()).transpose(-1, -2) @ DO.abs()),
    }
