"""Group-scaled int4 storage on the CPU: the packing, the quantizer and the
quantized inference model against a plain fp32 model that holds the
dequantized weights."""

import copy

import pytest
import torch

from zero_transformer_amd.models.inference import GPT2, StaticKVCache
from zero_transformer_amd.models.quant import quantize_w4_
from zero_transformer_amd.ops.reference import (dequantize_rows_w4, quantize_rows_w4,
                                                unpack_rows_w4)


def test_every_code_at_every_position():
    """Row p of a (32, 128) weight holds code (p + k) % 16 at position k, so
    every position of a 32-k block sees all 16 codes; q = -8 cannot come out
    of the quantizer, so the nibbles are packed here by the documented order:
    nibble j of dword d holds k = 8 d + [0, 2, 4, 6, 1, 3, 5, 7][j]."""
    u = (torch.arange(32)[:, None] + torch.arange(128)[None, :]) % 16
    dwords = torch.zeros(32, 16, dtype=torch.int64)
    for j, k in enumerate((0, 2, 4, 6, 1, 3, 5, 7)):
        dwords |= u[:, k::8] << (4 * j)
    packed = torch.stack([(dwords >> (8 * b)) & 255 for b in range(4)], 2)
    packed = packed.reshape(32, 64).to(torch.uint8)
    assert torch.equal(unpack_rows_w4(packed), (u - 8).to(torch.int8))
    # the quantizer packs in the same order: codes 1..15 with scale 1
    w = (u.clamp(min=1) - 8).float()
    w[:, ::16] = 7.0  # every group reaches max |w| = 7 -> scale exactly 1
    got, scale = quantize_rows_w4(w)
    assert torch.equal(scale, torch.ones(32, 1))
    assert torch.equal(unpack_rows_w4(got), w.to(torch.int8))


def test_hand_written_case():
    w = torch.zeros(2, 128)
    w[0, :4] = torch.tensor([7.0, -7.0, 2.5, 3.5])  # scale 1; ties go to even: 2, 4
    w[1, :3] = torch.tensor([0.5, -0.3, 0.1])       # scale 0.5 / 7: 7, -4.2, 1.4
    w = torch.cat([w, torch.zeros(2, 128)], 1)      # second group of both rows: zero
    packed, scale = quantize_rows_w4(w)
    assert packed.dtype == torch.uint8 and packed.shape == (2, 128) and packed.is_contiguous()
    assert scale.dtype == torch.float32 and scale.shape == (2, 2)
    assert torch.equal(scale, torch.tensor([[7.0, 0.0], [0.5, 0.0]]) / 7.0)
    q = unpack_rows_w4(packed)
    assert q[0, :4].tolist() == [7, -7, 2, 4] and q[1, :3].tolist() == [7, -4, 1]
    assert not q[:, 4:].any()
    # byte 0 of a row: k0 in the low nibble, k2 in the high one; byte 2: k1, k3
    assert packed[0, 0] == (7 + 8) | ((2 + 8) << 4) and packed[0, 2] == (-7 + 8) | ((4 + 8) << 4)
    for bad in (torch.zeros(2, 192), torch.zeros(128)):
        with pytest.raises(AssertionError):
            quantize_rows_w4(bad)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_dequantize_rounds_once(dtype):
    g = torch.Generator().manual_seed(1)
    packed, scale = quantize_rows_w4((torch.randn(37, 512, generator=g) * 0.05).to(dtype))
    want = unpack_rows_w4(packed).float() * scale.repeat_interleave(128, 1)
    for out in (torch.float16, torch.bfloat16, torch.float32):
        assert torch.equal(dequantize_rows_w4(packed, scale, out), want.to(out))


def _model(dtype=torch.float32):
    torch.manual_seed(0)
    return GPT2(embedding_dim=128, vocab_size=96, num_head=4, num_ctx=64, N=2).to(dtype).eval()


def test_cpu_model_equals_dequantized_fp32_model():
    plain = _model()
    quant = quantize_w4_(copy.deepcopy(plain))
    sd = quant.state_dict()
    twice = quantize_w4_(quant).state_dict()  # idempotent: the same buffers
    assert twice.keys() == sd.keys()
    assert all(twice[k].data_ptr() == sd[k].data_ptr() for k in sd)
    fused = quant.blocks[0].attn.qkv_w8
    assert sd["blocks.0.attn.qkv_w8.packed"].dtype == torch.uint8
    assert fused.shape == (384, 128) and fused.rows(128, 256).shape == (128, 128)
    m16 = copy.deepcopy(quant).half()  # a dtype cast leaves the fp32 scales bit for bit
    assert m16.blocks[1].mlp.fc1.scale.dtype == torch.float32
    assert torch.equal(m16.blocks[1].mlp.fc1.scale, quant.blocks[1].mlp.fc1.scale)
    with torch.no_grad():
        for pb, qb in zip(plain.blocks, quant.blocks):
            w = dequantize_rows_w4(qb.attn.qkv_w8.packed, qb.attn.qkv_w8.scale, torch.float32)
            for lin, part in zip((pb.attn.query, pb.attn.key, pb.attn.value), w.chunk(3)):
                lin.weight.copy_(part)
            for pm, qm in ((pb.attn.fc_resid, qb.attn.fc_resid), (pb.mlp.fc1, qb.mlp.fc1),
                           (pb.mlp.fc_resid, qb.mlp.fc_resid)):
                pm.weight.copy_(dequantize_rows_w4(qm.packed, qm.scale, torch.float32))
    # a quantized model takes its own state_dict back, bit for bit
    again = quantize_w4_(_model())
    with torch.no_grad():
        again.blocks[1].mlp.fc1.packed.zero_()
    again.load_state_dict(sd)
    for k, v in again.state_dict().items():
        assert torch.equal(v, sd[k]), k

    idx = torch.randint(0, 96, (2, 9), generator=torch.Generator().manual_seed(2))
    nxt = torch.tensor([[3], [7]])
    outs = []
    with torch.no_grad():
        for m in (plain, again):
            cache = StaticKVCache(2, 2, 4, 32, 16, "cpu", torch.float32)
            cache.set_len([9, 6])
            last = m.prefill(idx, cache, lens=[9, 6])
            cache.advance(1)
            outs.append((m(idx), last, m(nxt, static_cache=cache)))
    for a, b in zip(*outs):
        torch.testing.assert_close(b, a, rtol=1e-5, atol=1e-5 * float(a.abs().max()))
