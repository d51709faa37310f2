"""Sum of squared gradients out of the AdamW kernel, and the optimizer-level
changes around it: the first weight gradient of a step written straight into
the flat bucket, and no separate gradient shard on one rank.

Bound on the sum of squares. All terms are non-negative, so the fp32 result
is within gamma_k = k u / (1 - k u), u = 2^-24, of the exact sum of the
stored gradients' squares, k being the longest chain of roundings behind the
result as the kernels are written (ops/csrc/adamw.hip):
  per thread   one rounding for the square (exact for bf16 gradients, counted
               anyway) and one per accumulated element: 4 x iterations in the
               vector kernel, 1 x iterations in the scalar kernel
  per block    block_reduce_sum: 6 butterfly steps in the wave, 6 across the
               waves
  final        sumsq_final: ceil(grid / 256) partials per thread in series,
               then the same 6 + 6
with block = 256, grid = min(ceil(work / 256), 4096) and iterations =
ceil(work / (grid * 256)); work = n / 4 for n % 4 == 0, else n.

Every check prints its count of differing elements or its worst
error / bound ratio.
"""

import math

import pytest
import torch

from zero_transformer_amd import ops

from . import _parity as P
from ._parity import BF16, FP32

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BLOCK, GRID_CAP = 256, 4096
BIG = 4096 * 256 * 4 + 128  # vector kernel past its 4096-block grid
HP = (1e-3, 0.9, 0.95, 1e-8, 0.1)  # lr, beta1, beta2, eps, wd


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.hip_available(), "HIP extension must be built on GPU boxes"
    return torch.device("cuda", 0)


def chain_length(n: int) -> int:
    v4 = n % 4 == 0
    work = n // 4 if v4 else n
    grid = min(max((work + BLOCK - 1) // BLOCK, 1), GRID_CAP)
    iters = (work + grid * BLOCK - 1) // (grid * BLOCK)
    per_thread = 1 + iters * (4 if v4 else 1)
    return per_thread + 12 + (grid + 255) // 256 + 12


def gamma(k: int) -> float:
    return k * U / (1 - k * U)


def _same(name, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, name
    es = got.element_size()
    a = got.contiguous().view(torch.uint8).view(-1, es)
    b = want.contiguous().view(torch.uint8).view(-1, es)
    bad = int((a != b).any(-1).sum())
    print(f"[parity] {name}: {bad} of {got.numel()} elements differ")
    return [] if bad == 0 else [f"{name}: {bad} of {got.numel()} elements differ"]


def _state(n, dev):
    p = P.randn((n,), FP32, 1).to(dev)
    m = P.randn((n,), FP32, 2, 0.1).to(dev)
    v = P.randn((n,), FP32, 3, 0.1).abs().to(dev)
    return p, m, v, torch.zeros(n, device=dev, dtype=BF16)


def _step(n, g, dev, sumsq, clip=1.0, gscale=0.5, emit=True):
    p, m, v, pb = _state(n, dev)
    out = torch.full((1,), float("nan"), device=dev) if sumsq else None
    ops.adamw_step(p, pb if emit else None, g, m, v, 7, *HP, clip, gscale, sumsq_out=out)
    return p, m, v, pb, out


@pytest.mark.parametrize("scale", [1.0, 1e3])
@pytest.mark.parametrize("gdtype", [BF16, FP32])
@pytest.mark.parametrize("n", [4, 128, 131, BIG])
def test_adamw_sumsq(dev, n, gdtype, scale):
    g = P.randn((n,), gdtype, 10, scale).to(dev)
    tag = f"adamw_sumsq n={n} g={str(gdtype)[6:]} x{scale:g}"
    p0, m0, v0, pb0, _ = _step(n, g, dev, False)
    p1, m1, v1, pb1, sq1 = _step(n, g, dev, True)
    bad = (_same(f"{tag} p", p1, p0) + _same(f"{tag} m", m1, m0) + _same(f"{tag} v", v1, v0)
           + _same(f"{tag} bf16", pb1, pb0))
    # without the bf16 emission: other template instances, whose own bits
    # (update and sum alike) may differ from the emitting ones in the last
    # place, so they are compared among themselves and against float64
    p2, m2, v2, _, _ = _step(n, g, dev, False, emit=False)
    p3, m3, v3, _, sq3 = _step(n, g, dev, True, emit=False)
    bad += (_same(f"{tag} p (no emit)", p3, p2) + _same(f"{tag} m (no emit)", m3, m2)
            + _same(f"{tag} v (no emit)", v3, v2))
    bad += _same(f"{tag} sumsq again (no emit)", _step(n, g, dev, True, emit=False)[4], sq3)
    # a second call: same bits
    bad += _same(f"{tag} sumsq again", _step(n, g, dev, True)[4], sq1)
    # the sum is of the RAW gradient: neither the clip nor grad_scale enter
    bad += _same(f"{tag} sumsq clip=0", _step(n, g, dev, True, clip=0.0)[4], sq1)
    bad += _same(f"{tag} sumsq scale=1", _step(n, g, dev, True, gscale=1.0)[4], sq1)
    want = float((P.f64(g) ** 2).sum())
    k = chain_length(n)
    for name, sq in (("emit", sq1), ("no emit", sq3)):
        r = abs(float(sq.double().item()) - want) / (gamma(k) * want)
        print(f"[parity] {tag} sumsq ({name}) vs float64 (k={k}): worst error/bound = {r:.3f}")
        if not r <= 1.0:
            bad.append(f"{tag} ({name}): sum of squares is {r:.3f} x the bound gamma_{k}")
    assert not bad, "; ".join(bad)


def test_adamw_sumsq_rejects_wrong_output(dev):
    g = P.randn((128,), BF16, 10).to(dev)
    p, m, v, pb = _state(128, dev)
    with pytest.raises(RuntimeError):
        ops.adamw_step(p, pb, g, m, v, 1, *HP, 1.0, 1.0,
                       sumsq_out=torch.zeros(2, device=dev))


# ---------------------------------------------------------------------------
# Optimizer level: tiny model, 2 blocks, C = 512, 8 heads, T = 64, B = 2
# ---------------------------------------------------------------------------


def _tiny(dev):
    from zero_transformer_amd.models.gpt import GPT
    from zero_transformer_amd.utils.config import DotDict

    cfg = DotDict(embedding_dim=512, vocab_size=1024, num_head=8, block_size=64,
                  dropout=0.1, N=2, alibi_attn=True)
    torch.manual_seed(0)
    return GPT(cfg).to(dev).train()  # fp32 module; the parameters turn bf16 below


def _batches():
    gen = torch.Generator().manual_seed(5)
    return [torch.randint(0, 1024, (2, 64), generator=gen) for _ in range(2)]


def _backward(model, batch, dev):
    mb = batch.to(dev)
    _, loss = model(mb, labels=mb)
    loss.backward()


def _reseed():
    torch.manual_seed(99)
    ops._DROP_RNG = None


def _compare_buckets(tag, opt, model, twin, rows):
    """Matrices (through ops.linear, or the tied embedding) bit for bit.

    LayerNorm weights: their gradient is added up by ln_dw_reduce's fp32
    atomics in an order that is not fixed from run to run (parent and twin
    alike), so two runs may differ by a reordered fp32 sum of `rows` terms,
    gamma_{rows-1} * sum|terms| <= gamma * rows * max|dw| taking the largest
    entry as the size of a term, and then by one bf16 step (2^-7 relative)."""
    bad = []
    for (n, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        if n == "lm_head.weight":
            continue
        view, want = opt._grad_view[id(p)], q.grad
        assert want is not None, n
        if p.dim() > 1:
            bad += _same(f"{tag} {n}", view, want)
        else:
            a = gamma(rows - 1) * rows * float(want.float().abs().max())
            r = P.worst_ratio(view, want, BF16, a)
            print(f"[parity] {tag} {n}: worst error/bound = {r:.3f}")
            if not r <= 1.0:
                bad.append(f"{tag} {n}: error is {r:.3f} x the bound")
    return bad


def _norm_check(tag, opt, accum):
    """last_grad_norm = sqrt(sum over buckets of sumsq) / accum against the
    float64 norm of the buckets: each bucket's sum within gamma_k, their sum
    (torch, one more addition per bucket) and the square root and division
    (one rounding each, the root halves the relative error) on top."""
    want = math.sqrt(sum(float((P.f64(b.flat_grad) ** 2).sum()) for b in opt.buckets)) / accum
    k = max(chain_length(b.numel) for b in opt.buckets) + len(opt.buckets)
    bound = (gamma(k) / 2 + 2 * U) * want
    r = abs(float(opt.last_grad_norm.double().item()) - want) / bound
    print(f"[parity] {tag} last_grad_norm (k={k}): worst error/bound = {r:.3f}")
    return [] if r <= 1.0 else [f"{tag}: last_grad_norm is {r:.3f} x the bound"]


@pytest.mark.parametrize("accum", [1, 2])
def test_bucket_holds_the_gradient_bits(dev, accum):
    """accum = 1: after one backward every bucket view holds the bits p.grad
    holds in a twin model without the optimizer (the weight-gradient GEMM
    wrote them there itself). accum = 2: the second micro-step goes through
    the temporary and add_, and the bucket equals autograd's own accumulation
    in the twin, which is the copy-then-add_ result. One rank: grad_shard is
    the bucket itself, and step() reports the norm of what it holds."""
    from zero_transformer_amd.parallel.zero import ZeRO1Optimizer

    model, twin = _tiny(dev), _tiny(dev)
    opt = ZeRO1Optimizer(list(model.named_parameters()), lr=1e-4, bucket_mb=2.0,
                         param_dtype=BF16, accum_steps=accum)
    for q in twin.parameters():  # the optimizer's own rounding of the working copy
        q.data = q.data.to(BF16)
    written = []
    grad_written = opt.grad_written
    opt.grad_written = lambda p: (written.append(id(p)), grad_written(p))[1]
    assert len(opt.buckets) > 2
    for b in opt.buckets:
        assert b.grad_shard.data_ptr() == b.flat_grad.data_ptr()
    batches = _batches()[:accum]
    for mdl in (model, twin):
        _reseed()
        for i, mb in enumerate(batches):
            if mdl is model:
                opt.set_sync(i == accum - 1)
            _backward(mdl, mb, dev)
    linear_w = [id(p) for n, p in model.named_parameters() if p.dim() > 1 and n != "wte.weight"]
    assert sorted(written) == sorted(linear_w) and len(written) == 8, (
        "each ops.linear weight takes the direct path once, in the first micro-step")
    tag = f"zero accum={accum}"
    bad = _compare_buckets(tag, opt, model, twin, rows=2 * 64)
    before = [b.flat_grad.clone() for b in opt.buckets]
    opt.step()
    for b, g in zip(opt.buckets, before):
        bad += _same(f"{tag} bucket {b.idx} untouched by step()", b.flat_grad, g)
    bad += _norm_check(tag, opt, accum)
    assert not bad, "; ".join(bad)
