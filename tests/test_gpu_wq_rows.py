"""Quantized projections at 17..64 rows on the MI355X: the fused-dequant MFMA
body of ops/csrc/gemm_wq_rows.hip, through its bindings and through
ops.linear_w8 / ops.linear_w4, against float64 products with the checker and
bound of tests/_parity.py (one ulp of the output + TINY + ACC * |x| @ |W|^T).
W8: W = q * scale. W4: W = dequantize_rows_w4(packed, scale, dtype), the
once-rounded weight that linear_w4 defines the many-row result over."""

import functools

import pytest
import torch

from zero_transformer_amd.models.inference import GPT2, generate_batch, generate_fast
from zero_transformer_amd.models.quant import quantize_w4_, quantize_w8_
from zero_transformer_amd.ops.reference import (dequantize_rows_w4, quantize_rows_w4,
                                                quantize_rows_w8)

from . import _parity as P
from ._ragged import make_prompts

pytestmark = pytest.mark.gpu

NS = (5, 1023, 1024)  # less than a tile, one short of 8 workgroups' rows, exact
# (K, ksplit): (512, 0) is one unit: two 256-k pieces of x, no split, direct
# store; (1536, 0) picks three splits of one unit each (partial buffer +
# reduce kernel); (1536, 2) forces a first chunk of two units (four pieces,
# the weight prefetch crossing a restaged piece) and a shorter last one (512);
# (1024, 1) runs two units unsplit.
KS = ((512, 0), (1536, 0), (1536, 2), (1024, 1))
LENS = (5, 12, 9, 3, 20, 7, 1, 16, 2, 11, 4, 8, 13, 6, 10, 15, 3, 9, 14, 5)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _case(fmt, dtype, N, K):
    """x (65, K), the weight with the hostile rows / groups of the _case of
    tests/test_gpu_w8.py / test_gpu_w4.py, float64 want and abs_term."""
    x = P.randn((65, K), dtype, 100 + K)
    w = P.randn((N, K), dtype, 200 + N + K, 0.05)
    if fmt == "w8":
        q, scale = quantize_rows_w8(w)
        scale[0] = 0.0
        scale[1] = 1e-4 * scale[3]
        q[2] = -127
        W = q.double() * scale.double()[:, None]
    else:
        q, scale = quantize_rows_w4(w)
        pat = torch.tensor([1.0, 1e3, 1e-2, 10.0])
        scale *= pat[(torch.arange(N)[:, None] + torch.arange(K // 128)[None, :]) % 4]
        scale[0, 1] = 0.0
        scale[1, 2] = 1e-4 * scale[1, 3]
        q[2, :64] = 0x00
        q[3, 64:128] = 0xFF
        W = P.f64(dequantize_rows_w4(q, scale, dtype))
    X = P.f64(x)
    return x.cuda(), q.cuda(), scale.cuda(), X @ W.T, P.ACC * (X.abs() @ W.abs().T)


def _fns(fmt):
    from zero_transformer_amd import ops

    ext = ops.hip_ops()
    if fmt == "w8":
        return ext.w8_gemm_rows, ops.linear_w8, ext.w8_gemm
    return ext.w4_gemm_rows, ops.linear_w4, ext.w4_gemm


@pytest.mark.parametrize("B", [17, 32, 33, 64])
@pytest.mark.parametrize("dtype", [P.BF16, P.FP16])
@pytest.mark.parametrize("fmt", ["w8", "w4"])
def test_kernel_parity(dev, fmt, dtype, B):
    rows_fn, linear, _ = _fns(fmt)
    bad = []
    for N in NS:
        for K, ksplit in KS:
            x65, q, scale, want, a = _case(fmt, dtype, N, K)
            x = x65[:B]
            y = rows_fn(x, q, scale, ksplit)
            with torch.no_grad():
                routed = linear(x.view(B, 1, K), q, scale).view(B, N)
            for name, got in (("binding", y), ("linear", routed)):
                assert got.shape == (B, N) and got.dtype == dtype
                r = P.worst_ratio(got, want[:B], dtype, a[:B])
                if r > 1.0:
                    bad.append(f"{name} N={N} K={K} ks={ksplit}: {r:.3f} x the bound")
            assert torch.equal(rows_fn(x, q, scale, ksplit), y), "not deterministic"
            assert torch.equal(routed, rows_fn(x, q, scale, 0)), "linear took another route"
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("fmt", ["w8", "w4"])
def test_row_cap_edges(dev, fmt):
    """65 rows keep the library route (same bound); 16 rows keep the <= 16-row
    MFMA body, bit for bit."""
    _, linear, gemm16 = _fns(fmt)
    x65, q, scale, want, a = _case(fmt, P.FP16, 1023, 1536)
    with torch.no_grad():
        P.assert_within(linear(x65, q, scale), want, P.FP16, a, name=f"linear_{fmt} 65 rows")
        assert torch.equal(linear(x65[:16], q, scale), gemm16(x65[:16], q, scale, 0))


@pytest.mark.parametrize("quantize", [quantize_w4_, quantize_w8_])
def test_graph_and_engine_20_rows(dev, quantize):
    """The 2-layer C = 512 model of tests/test_gpu_w4.py at 20 rows per decode
    step (every projection in the new body): generate_batch under the captured
    graph equals eager, and a 20-slot ServingEngine gives each greedy request
    the tokens generate_fast gives its prompt alone."""
    from zero_transformer_amd.models.paged import ServingEngine

    torch.manual_seed(5)
    m = GPT2(embedding_dim=512, vocab_size=512, num_head=4, num_ctx=64, N=2)
    with torch.no_grad():
        torch.nn.init.normal_(m.wte.weight, std=0.1)
        for b in m.blocks:
            b.attn.fc_resid.weight.mul_(8.0)
            b.mlp.fc_resid.weight.mul_(8.0)
    model = quantize(m.eval()).to(dev).to(torch.float16)
    prompts = make_prompts(LENS)
    eager = generate_batch(model, prompts, 6, use_graph=False)
    assert [len(r) for r in eager] == [6] * 20
    assert generate_batch(model, prompts, 6, use_graph=True) == eager

    alone = [generate_fast(model, torch.tensor([pr], device=dev), 6)[0, len(pr):].tolist()
             for pr in prompts]
    eng = ServingEngine(model, 20, 24, 64)
    ids = [eng.submit(pr, 6) for pr in prompts]
    out = eng.run()
    assert [out[i] for i in ids] == alone
