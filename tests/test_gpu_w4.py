"""Group-scaled int4 decode on the MI355X: the kernels of ops/csrc/gemv_w4.hip
against float64 references computed from the exact (packed, scale, x) they
receive, with the checker and bound of tests/_parity.py (one ulp of the
output + TINY + ACC * |x| @ |W|^T, W = unpack * scale), and a quantized model
through the decode step, the captured graph and the serving engine."""

import functools

import pytest
import torch

from zero_transformer_amd.models.inference import (GPT2, StaticKVCache, generate_batch,
                                                   generate_fast)
from zero_transformer_amd.models.quant import quantize_w4_
from zero_transformer_amd.ops.reference import (dequantize_rows_w4, quantize_rows_w4,
                                                unpack_rows_w4)

from . import _parity as P
from ._ragged import make_prompts

pytestmark = pytest.mark.gpu

NS = (5, 17, 1023, 1024)  # off both the 4-rows-per-block grid and the 16-row tile
# (K, ksplit): 512 is the smallest K (one streaming step with 16 live lanes;
# one 128-k step per wave of the matrix body); 1536 ends the streaming step
# at 48 lanes; 2048 is exactly one full streaming step, 2560 a full step plus
# a 16-lane one; 1024 is the smallest K the matrix body splits across
# workgroups (2 x 512, partial buffer + reduce kernel); (1536, 2) forces a
# first workgroup of two units (two steps per wave: the prefetch) and a last
# one whose chunk (512) is shorter.
KS = ((512, 0), (1536, 0), (2048, 0), (2560, 0), (1024, 0), (1536, 2))

# test_decode_step_logits: floor measured on the MI355X (see its docstring)
LOGIT_FLOOR = 0.0647
LOGIT_BOUND = 2 * LOGIT_FLOOR


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _case(dtype, N, K):
    """x (16, K), (packed, scale) made hostile to a wrong-group read, float64
    want and abs_term. Neighbouring groups of a row differ by 10x to 1e5x
    (another pattern in every row); row 0 has a group of scale 0, row 1 a
    group at 1e-4 x its neighbour, row 2 a group of code 0 (q = -8) and row 3
    a group of all +7."""
    x = P.randn((16, K), dtype, 100 + K)
    packed, scale = quantize_rows_w4(P.randn((N, K), dtype, 200 + N + K, 0.05))
    G = K // 128
    pat = torch.tensor([1.0, 1e3, 1e-2, 10.0])
    scale *= pat[(torch.arange(N)[:, None] + torch.arange(G)[None, :]) % 4]
    scale[0, 1] = 0.0
    scale[1, 2] = 1e-4 * scale[1, 3]
    packed[2, :64] = 0x00
    packed[3, 64:128] = 0xFF
    W = unpack_rows_w4(packed).double() * scale.double().repeat_interleave(128, 1)
    X = P.f64(x)
    return x.cuda(), packed.cuda(), scale.cuda(), X @ W.T, P.ACC * (X.abs() @ W.abs().T)


@pytest.mark.parametrize("dtype", [P.BF16, P.FP16])
@pytest.mark.parametrize("B", range(1, 17))
def test_kernel_parity(dev, B, dtype):
    from zero_transformer_amd import ops

    ext = ops.hip_ops()
    bad = []
    for N in NS:
        for K, ksplit in KS:
            x16, packed, scale, want, a = _case(dtype, N, K)
            x = x16[:B]
            with torch.no_grad():  # as in inference: grad on takes the many-row route
                routed = ops.linear_w4(x.view(B, 1, K), packed, scale).view(B, N)
            runs = {"gemm": ext.w4_gemm(x, packed, scale, ksplit), "linear_w4": routed}
            if B <= 4:
                runs["gemv"] = ext.w4_gemv(x, packed, scale)
            for name, y in runs.items():
                assert y.shape == (B, N) and y.dtype == dtype
                r = P.worst_ratio(y, want[:B], dtype, a[:B])
                if r > 1.0:
                    bad.append(f"{name} N={N} K={K}: {r:.3f} x the bound")
            again = {"gemm": ext.w4_gemm(x, packed, scale, ksplit)}
            if B <= 4:
                again["gemv"] = ext.w4_gemv(x, packed, scale)
            for name, y in again.items():
                assert torch.equal(P.f64(y), P.f64(runs[name])), f"{name} not deterministic"
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("dtype", [P.BF16, P.FP16])
def test_dequant_and_many_rows(dev, dtype):
    from zero_transformer_amd import ops

    for N, K in ((1023, 1536), (5, 512)):
        _, packed, scale, _, _ = _case(dtype, N, K)
        got = ops.hip_ops().dequant_w4(packed, scale, dtype == P.BF16)
        want = dequantize_rows_w4(packed.cpu(), scale.cpu(), dtype)
        assert got.dtype == dtype and torch.equal(got.cpu().view(torch.int16),
                                                  want.view(torch.int16))
    # 17 rows: by definition the GEMM over the once-rounded dequantized weight
    x = P.randn((17, 1536), dtype, 7)
    _, packed, scale, _, _ = _case(dtype, 1023, 1536)
    W = P.f64(dequantize_rows_w4(packed.cpu(), scale.cpu(), dtype))
    y = ops.linear_w4(x.to(dev), packed, scale)
    P.assert_within(y, P.f64(x) @ W.T, dtype, P.ACC * (P.f64(x).abs() @ W.abs().T),
                    name=f"linear_w4 17 rows {dtype}")


def _lively(dtype=torch.float32):
    """GPT2(512, 4 heads of 128, N=2, vocab 512), made lively as
    tests/_ragged.make_model does, so that the blocks decide the logits."""
    torch.manual_seed(5)
    m = GPT2(embedding_dim=512, vocab_size=512, num_head=4, num_ctx=64, N=2)
    with torch.no_grad():
        torch.nn.init.normal_(m.wte.weight, std=0.1)
        for b in m.blocks:
            b.attn.fc_resid.weight.mul_(8.0)
            b.mlp.fc_resid.weight.mul_(8.0)
    return m.to(dtype).eval()


def _decode_step_logits(model, prompts, tok=None):
    """Ragged prefill, then one static-cache decode step on `tok` (None: the
    prefill's greedy tokens) -> ((B, V) logits, tok)."""
    p = next(model.parameters())
    lens = [len(pr) for pr in prompts]
    idx = torch.zeros(len(prompts), max(lens), dtype=torch.long)
    for b, pr in enumerate(prompts):
        idx[b, :lens[b]] = torch.tensor(pr)
    cache = StaticKVCache(model.N, len(prompts), 4, 128, 32, p.device, p.dtype)
    with torch.no_grad():
        cache.set_len(lens)
        last = model.prefill(idx.to(p.device), cache, lens=lens)
        cache.advance(1)
        tok = last.argmax(-1, keepdim=True).cpu() if tok is None else tok
        return model(tok.to(p.device), static_cache=cache)[:, -1].float().cpu(), tok


def test_decode_step_logits(dev):
    """One static-cache decode step at B = 3 (prompt lengths 5/12/9; the
    ragged prefill runs the many-row route) of a quantized bf16 model on the
    GPU against the same quantized model on the CPU in fp32; both feed the
    CPU's token.

    The bound is 2x a floor: max |GPU bf16 logits - CPU fp32 logits| of the
    UNQUANTIZED model holding the dequantized weights, which runs no code of
    the W4 path. Measured on the MI355X: floor 0.0647 (logit std 2.37), so
    the bound is 0.1294 <= 0.237; the W4 model's own difference came out as
    0.0536 (in fp16: floor 0.0070, W4 0.0065). Also in profiles/PERF.md
    ("W4A16 decode")."""
    quant = quantize_w4_(_lively())
    prompts = make_prompts((5, 12, 9))
    want, tok = _decode_step_logits(quant, prompts)
    got, _ = _decode_step_logits(quant.to(dev).to(torch.bfloat16), prompts, tok)
    diff, std = float((got - want).abs().max()), float(want.std())
    print(f"[w4] decode-step logits: max diff {diff:.4f}, bound {LOGIT_BOUND}, std {std:.2f}")
    assert LOGIT_BOUND <= 0.1 * std, "bound too loose to show anything"
    assert diff <= LOGIT_BOUND


def test_graph_and_engine(dev):
    """generate_batch under the captured graph equals eager, and a 4-slot
    ServingEngine gives each of 5 greedy requests the tokens generate_fast
    gives its prompt alone, in fp16 as tests/test_gpu_w8.py does."""
    from zero_transformer_amd.models.paged import ServingEngine

    model = quantize_w4_(_lively()).to(dev).to(torch.float16)
    prompts = make_prompts((5, 12, 9))
    eager = generate_batch(model, prompts, 6, use_graph=False)
    assert [len(r) for r in eager] == [6, 6, 6]
    assert generate_batch(model, prompts, 6, use_graph=True) == eager

    prompts = make_prompts((5, 12, 9, 3, 20))
    alone = [generate_fast(model, torch.tensor([pr], device=dev), 6)[0, len(pr):].tolist()
             for pr in prompts]
    eng = ServingEngine(model, 4, 6, 64)
    ids = [eng.submit(pr, 6) for pr in prompts]
    out = eng.run()
    assert [out[i] for i in ids] == alone
