"""Attention forward at the shapes where its tile logic can go wrong.

The binding `attn_fwd(qkv, slopes, H, p, seed) -> (o, lse)` is called
directly and both outputs are compared against the fp32 CPU reference, for
the default kernel and for the round-1 kernel (`ZTA_FWD_V1=1`). The selector
is read once per process, so each arm computes every case in ONE fresh child
process (this file run as a script) and the tests read its saved outputs.
Head dims below 128 run the round-1 kernel in both arms (attention_fwd.hip
header); their cases stay so that a later re-routing is covered.

Bounds. `o`: the project's forward bounds (tests/test_gpu_ops.py), 3e-2
without dropout and 4e-2 against the exact-mask reference; O is a convex
combination of V rows, so scaled scores do not loosen it. `lse`: 4x the
round-1 kernel's own max |lse - reference| over these inputs as measured on
an MI355X (1.9e-5, profiles/PERF.md) is 7.6e-5, below the floor of 1e-4, so
the floor is the bound.
"""

import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

O_TOL = 3e-2
O_TOL_MASK = 4e-2
LSE_TOL = 1e-4

B, H = 2, 3
SEED = 12345

# name -> (T, D, alibi, q/k scale, dropout p)
CASES = {}
for _T in (40, 64, 65, 200, 257, 320, 576):
    # partial sub-tile, exact tile, one row past a tile, clamped padding
    # rows, second q block with one interior tile, both interior/diagonal
    # transitions, three q blocks with many interior tiles
    CASES[f"T{_T}_D128"] = (_T, 128, True, 1.0, 0.0)
for _D in (32, 64, 96):
    CASES[f"T200_D{_D}"] = (200, _D, True, 1.0, 0.0)
# large and rising scores: the threshold rescale and the once-per-64-keys
# decision fire (bounded random data never exercises them)
CASES["T320_D128_x4_alibi"] = (320, 128, True, 4.0, 0.0)
CASES["T320_D128_x4_noalibi"] = (320, 128, False, 4.0, 0.0)
CASES["T257_D128_drop"] = (257, 128, True, 1.0, 0.3)
CASES["T200_D128_drop"] = (200, 128, True, 1.0, 0.3)

ARMS = ("default", "v1")


def _inputs(name):
    """CPU-generated, so the child and the parent see the same tensors."""
    T, D, alibi, qk_scale, p = CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    q, k, v = (torch.randn(B, H, T, D, generator=g) for _ in range(3))
    q, k, v = (q * qk_scale).bfloat16(), (k * qk_scale).bfloat16(), v.bfloat16()
    from zero_transformer_amd.ops import reference

    slopes = reference.alibi_slopes(H) if alibi else torch.zeros(H)
    return q, k, v, slopes


def _child(out_path):
    from zero_transformer_amd import ops

    ext = ops.hip_ops()
    dev = torch.device("cuda", 0)
    res = {}
    for name, (T, D, alibi, qk_scale, p) in CASES.items():
        q, k, v, slopes = _inputs(name)
        qkv = torch.cat([t.transpose(1, 2).reshape(B, T, H * D) for t in (q, k, v)], -1)
        qkv = qkv.contiguous().to(dev)
        sl = slopes.to(dev)
        o, lse = ext.attn_fwd(qkv, sl, H, p, SEED)
        res[name] = {"o": o.cpu(), "lse": lse.cpu()}
        if p > 0:
            o2, lse2 = ext.attn_fwd(qkv, sl, H, p, SEED)
            _, lse0 = ext.attn_fwd(qkv, sl, H, 0.0, SEED)
            res[name].update(o2=o2.cpu(), lse2=lse2.cpu(), lse_p0=lse0.cpu())
    torch.cuda.synchronize()
    torch.save(res, out_path)


@pytest.fixture(scope="module")
def arm_outputs(tmp_path_factory):
    cache = {}

    def get(arm):
        if arm not in cache:
            path = str(tmp_path_factory.mktemp("attn_fwd_edges") / f"{arm}.pt")
            env = {**os.environ, "PYTHONPATH": REPO}
            env.pop("ZTA_FWD_V1", None)
            if arm == "v1":
                env["ZTA_FWD_V1"] = "1"
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path],
                               env=env, cwd=REPO, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            cache[arm] = torch.load(path)
        return cache[arm]

    return get


_REF = {}


def _reference(name):
    """(o, lse) of the fp32 CPU reference, computed once per case."""
    if name not in _REF:
        from zero_transformer_amd.ops import reference

        T, D, alibi, qk_scale, p = CASES[name]
        q, k, v, slopes = _inputs(name)
        q, k, v = q.float(), k.float(), v.float()
        sl = slopes if alibi else None
        if p > 0:
            keep = reference.drop_mask(SEED, B, H, T, p)
            o = reference.attention_with_mask(q, k, v, sl, keep, reference.drop_inv_keep(p))
        else:
            o = reference.attention(q, k, v, sl)
        scores = (q @ k.transpose(-1, -2)) / math.sqrt(D)
        if alibi:
            pos = torch.arange(T, dtype=torch.float32)
            scores = scores + slopes.view(1, H, 1, 1) * (pos.view(1, T) - pos.view(T, 1))
        causal = torch.ones(T, T, dtype=torch.bool).tril()
        scores = scores.masked_fill(~causal, float("-inf"))
        _REF[name] = (o, torch.logsumexp(scores, dim=-1))
    return _REF[name]


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("arm", ARMS)
def test_attn_fwd_edge_parity(arm_outputs, arm, name):
    T, D, alibi, qk_scale, p = CASES[name]
    got = arm_outputs(arm)[name]
    o_ref, lse_ref = _reference(name)
    o = got["o"].float().view(B, T, H, D).transpose(1, 2)
    lse = got["lse"]
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    o_err = (o - o_ref).abs().max().item()
    lse_err = (lse - lse_ref).abs().max().item()
    print(f"{arm} {name}: max|o - ref| = {o_err:.3e}  max|lse - ref| = {lse_err:.3e}")
    assert o_err < (O_TOL_MASK if p > 0 else O_TOL), f"o max diff {o_err}"
    assert lse_err < LSE_TOL, f"lse max diff {lse_err}"


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c[4] > 0])
@pytest.mark.parametrize("arm", ARMS)
def test_attn_fwd_dropout_lse_and_relaunch(arm_outputs, arm, name):
    """The denominator ignores dropout, and a relaunch with the same seed is
    bit-identical (no value depends on uninitialised or padding-row state)."""
    got = arm_outputs(arm)[name]
    for t in got.values():
        assert torch.isfinite(t.float()).all()
    assert torch.equal(got["lse"], got["lse_p0"]), "lse must not depend on dropout"
    assert torch.equal(got["o"], got["o2"]) and torch.equal(got["lse"], got["lse2"])


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    _child(sys.argv[2])
