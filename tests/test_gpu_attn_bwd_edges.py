"""Attention backward at its tile edges vs the float64 reference with the
derived bound (tests/_parity.py attn_bwd_ref), for both schemes.

`attn_fwd` then `attn_bwd` are called through the binding with the explicit
`fused` argument on CPU-generated inputs (B = 2, H = 3), the dropout mask
comes from reference.drop_mask, and all five outputs are checked: o and lse
with the forward edge tests' absolute bounds, dq / dk / dv with the derived
per-element bound. Every check asserts finiteness and prints its worst
error / bound ratio; the module prints the worst per scheme and tensor at the
end.

  T     reaches
  40    a single partial tile, fewer keys than one wave
  65    one row / key past a 64 tile
  129   second 128-key dKdV block holding one key
  257   second 256-row dQ block and second 256-key fused block, one row each
  320   interior plus diagonal tiles
  576   three fused key blocks: dQ rows receive 1, 2 or 3 atomic adds
        (fused scratch indexing across B = 2 batches and the blocks)

  scheme            D                T                      p
  two-kernel (0)    32, 64, 96, 128  40 65 129 257 320      0
  two-kernel (0)    32, 64, 96, 128  65 257                 0.3  (the dropout
                    96               129                    0.1   branches of
                                                                  dq and dkdv4)
  fused (1)         128              40 65 257 320 576      0
  fused (1)         128              65 257 576             0.3
  both              128              320, q and k x4        0    with ALiBi and
                                                                 with zero slopes
  two-kernel (0)    96               257, launched twice    0.3  bitwise equal

  delta kernels, rows = B H T just past one pass (grid-stride loop entered):
  delta_kernel      32   B=1 H=8  T=1040   8320 rows  > 8192
  delta_kernel_v8   64   B=4 H=16 T=1040   66560 rows > 65536
  (reference on (b, h) planes 0 and the last, which holds the second pass)

The binding's argument checks are tested at the end: each raises before any
launch.
"""

import pytest
import torch

from zero_transformer_amd.ops import reference

from . import _parity as P
from ._parity import BF16

pytestmark = pytest.mark.gpu

B, H = P.ATTN_BH
SEED = P.ATTN_SEED
WORST = {}
_REF = {}


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


def _case(T, D, p, qk_scale, alibi):
    """CPU inputs, mask and float64 reference of one shape; built once and
    shared (read-only) by the schemes that use it."""
    key = (T, D, p, qk_scale, alibi)
    if key not in _REF:
        q, k, v, do = P.attn_bwd_inputs(B, H, T, D, qk_scale)
        slopes = reference.alibi_slopes(H) if alibi else torch.zeros(H)
        keep = reference.drop_mask(SEED, B, H, T, p) if p > 0 else None
        want = P.attn_bwd_ref(q, k, v, do, slopes, keep, reference.drop_inv_keep(p))
        _REF[key] = (q, k, v, do, slopes, want)
    return _REF[key]


def _pack(t):
    """(B, H, T, D) -> (B, T, H * D)"""
    b, h, T, D = t.shape
    return t.transpose(1, 2).reshape(b, T, h * D)


def _unpack(t, h):
    """(B, T, H * D) -> (B, H, T, D)"""
    b, T, C = t.shape
    return t.view(b, T, h, C // h).transpose(1, 2)


def _run(dev, q, k, v, do, slopes, p, fused):
    """attn_fwd + attn_bwd through the binding -> the five outputs on the CPU
    in the reference's (B, H, T, D) layout."""
    ext = _ext()
    h = q.shape[1]
    qkv = torch.cat([_pack(q), _pack(k), _pack(v)], -1).contiguous().to(dev)
    sl = slopes.to(dev)
    dout = _pack(do).contiguous().to(dev)
    o, lse = ext.attn_fwd(qkv, sl, h, p, SEED)
    (dqkv,) = ext.attn_bwd(dout, qkv, sl, o, lse, h, p, SEED, fused)
    assert dqkv.shape == qkv.shape and dqkv.dtype == BF16
    dq, dk, dv = (_unpack(t, h) for t in dqkv.cpu().split(qkv.shape[-1] // 3, dim=-1))
    return {"o": _unpack(o.cpu(), h), "lse": lse.cpu(), "dq": dq, "dk": dk, "dv": dv}


def _check(scheme, tag, got, want):
    bad = []
    for n in ("o", "lse", "dq", "dk", "dv"):
        assert torch.isfinite(got[n].float()).all(), f"{scheme} {tag}: {n} not finite"
        if n in ("o", "lse"):
            r = P.worst_abs_ratio(got[n], *want[n])
        else:
            r = P.worst_ratio(got[n], want[n][0], BF16, want[n][1])
        print(f"[parity] {scheme}-{n} {tag}: worst error/bound = {r:.3f}")
        WORST[f"{scheme}-{n}"] = max(WORST.get(f"{scheme}-{n}", 0.0), r)
        if not r <= 1.0:
            bad.append(f"{scheme}-{n} {tag}: error is {r:.3f} x the bound")
    assert not bad, "; ".join(bad)


def _parity(dev, fused, T, D, p, qk_scale, alibi):
    q, k, v, do, slopes, want = _case(T, D, p, qk_scale, alibi)
    got = _run(dev, q, k, v, do, slopes, p, fused)
    tag = f"T={T} D={D} p={p}" + (f" x{qk_scale:g} alibi={int(alibi)}" if qk_scale != 1.0 else "")
    _check("fused" if fused else "two-kernel", tag, got, want)


@pytest.mark.parametrize("T,D,p,qk_scale,alibi", P.ATTN_BWD_TWO)
def test_two_kernel_bwd_parity(dev, T, D, p, qk_scale, alibi):
    _parity(dev, 0, T, D, p, qk_scale, alibi)


@pytest.mark.parametrize("T,D,p,qk_scale,alibi", P.ATTN_BWD_FUSED)
def test_fused_bwd_parity(dev, T, D, p, qk_scale, alibi):
    _parity(dev, 1, T, D, p, qk_scale, alibi)


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("T,D,p,qk_scale,alibi", P.ATTN_BWD_BIG)
def test_bwd_parity_large_scores(dev, fused, T, D, p, qk_scale, alibi):
    """q and k x4: scores of +-60 and more, p spans its whole range; with
    ALiBi and with zero slopes."""
    _parity(dev, fused, T, D, p, qk_scale, alibi)


def test_two_kernel_bwd_is_bitwise_reproducible(dev):
    """dQ on the caller's stream and dKdV on the side stream write disjoint
    columns with no atomics: two launches agree bit for bit."""
    T, D, p = 257, 96, 0.3
    q, k, v, do, slopes, _ = _case(T, D, p, 1.0, True)
    a = _run(dev, q, k, v, do, slopes, p, 0)
    b = _run(dev, q, k, v, do, slopes, p, 0)
    for n in ("o", "lse", "dq", "dk", "dv"):
        assert torch.equal(a[n], b[n]), f"{n} differs between launches"


@pytest.mark.parametrize("b,h,T,D", P.ATTN_DELTA_STRIDE)
def test_delta_grid_stride(dev, b, h, T, D):
    """More rows than one pass of the delta kernel covers; the last (b, h)
    plane holds every row of the second pass."""
    q, k, v, do = P.attn_bwd_inputs(b, h, T, D)
    slopes = reference.alibi_slopes(h)
    got = _run(dev, q, k, v, do, slopes, 0.0, 0)
    for t in got.values():
        assert torch.isfinite(t.float()).all()
    for ib, ih in ((0, 0), (b - 1, h - 1)):
        cut = lambda t: t[ib:ib + 1, ih:ih + 1]
        want = P.attn_bwd_ref(cut(q), cut(k), cut(v), cut(do), slopes[ih:ih + 1])
        _check("two-kernel", f"T={T} D={D} rows={b * h * T} plane=({ib},{ih})",
               {n: cut(t) for n, t in got.items()}, want)


# ---------------------------------------------------------------------------
# Binding validation
# ---------------------------------------------------------------------------


@pytest.fixture(scope="module")
def valid(dev):
    """A valid argument set (T = 8, D = 32, H = 2)."""
    ext = _ext()
    h, T, D = 2, 8, 32
    C = h * D
    qkv = P.randn((1, T, 3 * C), BF16, 1).to(dev)
    slopes = reference.alibi_slopes(h).to(dev)
    o, lse = ext.attn_fwd(qkv, slopes, h, 0.0, SEED)
    return dict(dout=P.randn((1, T, C), BF16, 2).to(dev), qkv=qkv, slopes=slopes, o=o,
                lse=lse, H=h)


def _bf16_like(t, shape=None):
    return torch.zeros(shape or t.shape, dtype=BF16, device=t.device)


_BAD = {
    "qkv_fp16": ("qkv must be bf16", lambda a: {"qkv": a["qkv"].half()}),
    "qkv_fp32": ("qkv must be bf16", lambda a: {"qkv": a["qkv"].float()}),
    "dout_cpu": ("dout must be on qkv's device", lambda a: {"dout": a["dout"].cpu()}),
    "o_cpu": ("o must be on qkv's device", lambda a: {"o": a["o"].cpu()}),
    "lse_cpu": ("lse must be on qkv's device", lambda a: {"lse": a["lse"].cpu()}),
    "dout_fp16": ("dout must be bf16", lambda a: {"dout": a["dout"].half()}),
    "o_fp32": ("o must be bf16", lambda a: {"o": a["o"].float()}),
    "dout_wide": (r"dout must be \(B, T, C\)", lambda a: {"dout": _bf16_like(a["dout"], (1, 8, 72))}),
    "dout_long": (r"dout must be \(B, T, C\)", lambda a: {"dout": _bf16_like(a["dout"], (1, 9, 64))}),
    "dout_2d": (r"dout must be \(B, T, C\)", lambda a: {"dout": _bf16_like(a["dout"], (8, 64))}),
    "o_batch": (r"o must be \(B, T, C\)", lambda a: {"o": _bf16_like(a["o"], (2, 8, 64))}),
    "o_short": (r"o must be \(B, T, C\)", lambda a: {"o": _bf16_like(a["o"], (1, 7, 64))}),
    "lse_f64": (r"lse must be float32 \(B, H, T\)", lambda a: {"lse": a["lse"].double()}),
    "lse_bf16": (r"lse must be float32 \(B, H, T\)", lambda a: {"lse": a["lse"].bfloat16()}),
    "lse_bth": (r"lse must be float32 \(B, H, T\)",
                lambda a: {"lse": a["lse"].transpose(1, 2).contiguous()}),
    "o_strided": ("o must be contiguous",
                  lambda a: {"o": _bf16_like(a["o"], (1, 64, 8)).transpose(1, 2)}),
    "lse_strided": ("lse must be contiguous",
                    lambda a: {"lse": torch.zeros(1, 8, 2, device=a["lse"].device).transpose(1, 2)}),
    "C_mod_H": ("C % H == 0", lambda a: {"H": 3, "slopes": a["slopes"].new_zeros(3)}),
    "not_3C": ("must be 3C", lambda a: {"qkv": _bf16_like(a["qkv"], (1, 8, 193))}),
    "slopes_long": ("slopes must have H", lambda a: {"slopes": a["slopes"].new_zeros(3)}),
    "slopes_short": ("slopes must have H", lambda a: {"slopes": a["slopes"][:1]}),
}


@pytest.mark.parametrize("name", list(_BAD))
def test_attn_bwd_rejects(valid, name):
    match, change = _BAD[name]
    a = {**valid, **change(valid)}
    with pytest.raises(RuntimeError, match=match):
        _ext().attn_bwd(a["dout"], a["qkv"], a["slopes"], a["o"], a["lse"], a["H"], 0.0, SEED, 0)


def test_attn_bwd_accepts_the_valid_arguments(valid):
    a = valid
    (dqkv,) = _ext().attn_bwd(a["dout"], a["qkv"], a["slopes"], a["o"], a["lse"], a["H"], 0.0, SEED, 0)
    assert dqkv.shape == a["qkv"].shape and torch.isfinite(dqkv.float()).all()
