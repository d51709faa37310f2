"""Weight-only int8 storage on the CPU: the row quantizer, the memory it
saves and the quantized inference model against a plain fp32 model that
holds q * scale."""

import copy

import pytest
import torch

from zero_transformer_amd.models.inference import GPT2, StaticKVCache
from zero_transformer_amd.models.quant import quantize_w8_
from zero_transformer_amd.ops.reference import dequantize_rows_w8, quantize_rows_w8


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_quantizer(dtype):
    g = torch.Generator().manual_seed(1)
    w = (torch.randn(37, 512, generator=g) * 0.05).to(dtype)
    w[5] = 0
    q, scale = quantize_rows_w8(w)
    assert q.dtype == torch.int8 and q.shape == w.shape and q.is_contiguous()
    assert scale.dtype == torch.float32 and scale.shape == (37,)
    assert int(q.abs().max()) <= 127 and int(q.min()) >= -127
    assert scale[5] == 0 and not q[5].any() and torch.isfinite(scale).all()
    live = scale > 0
    assert (q[live].abs().amax(1) == 127).all()
    err = (w.double() - q.double() * scale.double()[:, None]).abs()
    assert (err <= 0.5 * scale.double()[:, None] * (1 + 1e-5)).all()
    for out in (torch.float16, torch.bfloat16):
        assert torch.equal(dequantize_rows_w8(q, scale, out),
                           (q.float() * scale[:, None]).to(out))


def _model(dtype=torch.float32):
    torch.manual_seed(0)
    return GPT2(embedding_dim=64, vocab_size=96, num_head=4, num_ctx=64, N=2).to(dtype).eval()


def test_memory():
    def block_bytes(m):
        ts = [t for b in m.blocks for t in list(b.parameters()) + list(b.buffers())]
        return sum(t.numel() * t.element_size() for t in ts)

    m = _model(torch.float16)
    before = block_bytes(m)
    assert block_bytes(quantize_w8_(m)) <= 0.55 * before


def test_cpu_model_equals_dequantized_fp32_model():
    plain = _model()
    quant = quantize_w8_(copy.deepcopy(plain))
    sd = quant.state_dict()
    assert sd["blocks.0.attn.qkv_w8.q"].dtype == torch.int8
    with torch.no_grad():
        for pb, qb in zip(plain.blocks, quant.blocks):
            w = dequantize_rows_w8(qb.attn.qkv_w8.q, qb.attn.qkv_w8.scale, torch.float32)
            for lin, part in zip((pb.attn.query, pb.attn.key, pb.attn.value), w.chunk(3)):
                lin.weight.copy_(part)
            for pm, qm in ((pb.attn.fc_resid, qb.attn.fc_resid), (pb.mlp.fc1, qb.mlp.fc1),
                           (pb.mlp.fc_resid, qb.mlp.fc_resid)):
                pm.weight.copy_(dequantize_rows_w8(qm.q, qm.scale, torch.float32))
    # a dtype cast of the model leaves the fp32 scales bit for bit
    for cast in (lambda m: m.half(), lambda m: m.to(torch.bfloat16)):
        m16 = cast(copy.deepcopy(quant))
        for b16, qb in zip(m16.blocks, quant.blocks):
            for w16, w in ((b16.attn.qkv_w8, qb.attn.qkv_w8), (b16.mlp.fc1, qb.mlp.fc1)):
                assert w16.scale.dtype == torch.float32 and torch.equal(w16.scale, w.scale)
                assert torch.equal(w16.q, w.q)
        assert m16.wte.weight.dtype != torch.float32
    # a quantized model takes its own state_dict back
    again = quantize_w8_(_model())
    again.load_state_dict(sd)
    assert torch.equal(again.blocks[1].mlp.fc1.q, quant.blocks[1].mlp.fc1.q)

    idx = torch.randint(0, 96, (2, 9), generator=torch.Generator().manual_seed(2))
    nxt = torch.tensor([[3], [7]])
    outs = []
    with torch.no_grad():
        for m in (plain, again):
            cache = StaticKVCache(2, 2, 4, 16, 16, "cpu", torch.float32)
            cache.set_len([9, 6])
            last = m.prefill(idx, cache, lens=[9, 6])
            cache.advance(1)
            outs.append((m(idx), last, m(nxt, static_cache=cache)))
    for a, b in zip(*outs):
        torch.testing.assert_close(b, a, rtol=1e-5, atol=1e-5 * float(a.abs().max()))
