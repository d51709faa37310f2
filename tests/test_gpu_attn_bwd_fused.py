"""Fused attention backward (one key-stationary kernel, dQ through f32
atomics) against the CPU fp32 reference, called through the binding with the
explicit scheme selector (fused=1 / fused=0). All fused shapes are D = 128;
the criterion is the project's attention-backward bound,
max|diff| / max|want| < 5e-2 for each of dq, dk, dv."""

import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 5e-2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _ext():
    from zero_transformer_amd import ops

    assert ops.hip_available(), "HIP extension must be built on GPU boxes"
    return ops.hip_ops()


_CASES = {}


def _case(dev, B, H, T, D, p=0.0, seed=0, gen=21):
    """Inputs, forward outputs and the CPU fp32 reference gradients of one
    shape; built once and shared (read-only) by the tests that use it."""
    key = (B, H, T, D, p, seed, gen)
    if key in _CASES:
        return _CASES[key]
    from zero_transformer_amd.ops import reference

    ext = _ext()
    torch.manual_seed(gen)
    q, k, v = (torch.randn(B, H, T, D, device=dev).to(torch.bfloat16) for _ in range(3))
    slopes = reference.alibi_slopes(H).to(dev)
    C = H * D
    qkv = torch.cat([t.transpose(1, 2).reshape(B, T, C) for t in (q, k, v)], -1).contiguous()
    o, lse = ext.attn_fwd(qkv, slopes, H, p, seed)
    do = torch.randn_like(o)

    qr, kr, vr = (t.detach().float().cpu().requires_grad_(True) for t in (q, k, v))
    if p > 0.0:
        keep = reference.drop_mask(seed, B, H, T, p)
        ref = reference.attention_with_mask(
            qr, kr, vr, slopes.cpu(), keep, reference.drop_inv_keep(p)
        )
    else:
        ref = reference.attention(qr, kr, vr, slopes.cpu())
    ref.backward(do.view(B, T, H, D).transpose(1, 2).float().cpu())
    case = dict(B=B, H=H, T=T, D=D, C=C, p=p, seed=seed, qkv=qkv, slopes=slopes, o=o,
                lse=lse, do=do, want=(qr.grad, kr.grad, vr.grad))
    _CASES[key] = case
    return case


def _bwd(case, fused):
    (dqkv,) = _ext().attn_bwd(case["do"], case["qkv"], case["slopes"], case["o"],
                              case["lse"], case["H"], case["p"], case["seed"], fused)
    return dqkv


def _split(case, dqkv):
    B, T, H, D = case["B"], case["T"], case["H"], case["D"]
    return tuple(t.view(B, T, H, D).transpose(1, 2) for t in dqkv.split(case["C"], dim=-1))


def _errors(case, dqkv):
    errs = {}
    for got, want, name in zip(_split(case, dqkv), case["want"], ("dq", "dk", "dv")):
        diff = (got.float().cpu() - want).abs().max().item()
        errs[name] = diff / (want.abs().max().item() + 1e-6)
    return errs


def _check(case, dqkv, what):
    errs = _errors(case, dqkv)
    print(f"{what} B{case['B']} H{case['H']} T{case['T']} D{case['D']} p{case['p']}: "
          + " ".join(f"{n}={e:.4e}" for n, e in errs.items()))
    for name, e in errs.items():
        assert e < BOUND, f"{what}: {name} rel-max diff {e}"
    return errs


# (1,2,576): key blocks 256 + 256 + 64, dQ rows get 1, 2 or 3 atomic adds.
# (1,1,300): T no multiple of 32, ragged last query slice and key group.
# (1,1,40):  a single partial block, fewer keys than one wave's 64.
@pytest.mark.parametrize("shape", [(1, 2, 576), (1, 1, 300), (1, 1, 40)])
def test_fused_bwd_parity(dev, shape):
    B, H, T = shape
    case = _case(dev, B, H, T, 128)
    _check(case, _bwd(case, 1), "fused")


def test_fused_bwd_dropout_exact_mask(dev):
    """p = 0.3 with a fixed seed against the reference evaluated with the
    kernels' regenerated keep-mask; two key blocks, so the mask is checked
    across the block seam."""
    case = _case(dev, 1, 2, 320, 128, p=0.3, seed=12345)
    _check(case, _bwd(case, 1), "fused dropout")


def test_fused_bwd_relaunch(dev):
    """Two launches on identical inputs: dk and dv involve no atomics and
    must be bit-identical; dq agrees within the bound (f32 atomic order), which
    also catches a scratch buffer that is not zeroed again."""
    case = _case(dev, 1, 2, 576, 128)
    a = _bwd(case, 1)
    b = _bwd(case, 1)
    C = case["C"]
    assert torch.equal(a[..., C:], b[..., C:]), "dk/dv differ between launches"
    _check(case, a, "fused launch 1")
    _check(case, b, "fused launch 2")
    qa, qb = a[..., :C].float(), b[..., :C].float()
    rel = (qa - qb).abs().max().item() / (case["want"][0].abs().max().item() + 1e-6)
    assert rel < BOUND, f"dq differs between launches: {rel}"


def test_fused_vs_two_kernel(dev):
    """Both schemes on the same inputs meet the bound against the fp32
    reference (the two error sets are printed for the record)."""
    case = _case(dev, 1, 2, 576, 128)
    _check(case, _bwd(case, 1), "fused")
    _check(case, _bwd(case, 0), "two-kernel")


def test_fused_selector_falls_back_for_other_head_dims(dev):
    """D = 64 with the fused scheme requested takes the two-kernel path and
    still returns correct gradients."""
    case = _case(dev, 1, 2, 200, 64)
    got = _bwd(case, 1)
    _check(case, got, "fallback D64")
    assert torch.equal(got, _bwd(case, 0))
