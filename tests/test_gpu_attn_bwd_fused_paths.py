"""The fused attention backward's per-slice softmax selection vs the float64
reference with the derived bound (tests/_parity.py attn_bwd_ref).

flash_bwd_fused_kernel picks, per 32-row slice and wave, an interior softmax
(no element of the wave's 64 keys x 32 rows masked: no compare, no select) or
a masked one, and shares the dropout hash within a lane quad. The procedure
is that of test_gpu_attn_bwd_edges.py (attn_fwd + attn_bwd(fused=1) through
the binding, B = 2, H = 3, D = 128, mask from reference.drop_mask, all of
o / lse / dq / dk / dv, ratio <= 1.0, finiteness asserted, ratios printed) at
the smallest shapes that reach the selection logic:

  T     p         reaches
  288   0, 0.3    key block 0 has exactly one slice that is interior for all
                  four waves (rows 256..287), block 1 is all diagonal
  300   0, 0.3    the slice that is interior by key position (rows 288..299)
                  is partial in rows (qi >= T): it must take the masked path
  545   0.1       three key blocks, the last holding 33 keys; one-row tail
                  slice; the benchmark's dropout threshold
  320   0.1       interior plus diagonal with dropout
  288   0         q and k x4: large scores in an interior slice, with ALiBi
                  and with zero slopes

dK and dV are bitwise equal across two launches (T = 300, p = 0.3); dQ is
summed with f32 atomics and is not.

The CPU test runs the fp32 emulation of the kernels' roundings
(test_parity_helpers.attn_bwd_emul) at the same shapes: the bound is
reachable.
"""

import pytest
import torch

from zero_transformer_amd.ops import reference

from . import _parity as P
from ._parity import BF16
from .test_gpu_attn_bwd_edges import _case, _run
from .test_parity_helpers import attn_bwd_emul

# (T, D, p, q/k scale, alibi)
PATHS = [
    (288, 128, 0.0, 1.0, True),
    (288, 128, 0.3, 1.0, True),
    (300, 128, 0.0, 1.0, True),
    (300, 128, 0.3, 1.0, True),
    (545, 128, 0.1, 1.0, True),
    (320, 128, 0.1, 1.0, True),
]
BIG = [(288, 128, 0.0, 4.0, True), (288, 128, 0.0, 4.0, False)]
WORST = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    yield torch.device("cuda", 0)
    for n, r in sorted(WORST.items()):
        print(f"[parity-summary] fused-paths-{n}: worst error/bound = {r:.3f}")


def _tag(T, D, p, qk_scale, alibi):
    return f"T={T} D={D} p={p} x{qk_scale:g} alibi={int(alibi)}"


def _check(scheme, tag, got, want, worst=None):
    bad = []
    for n in ("o", "lse", "dq", "dk", "dv"):
        assert torch.isfinite(got[n].float()).all(), f"{scheme} {tag}: {n} not finite"
        if n in ("o", "lse"):
            r = P.worst_abs_ratio(got[n], *want[n])
        else:
            r = P.worst_ratio(got[n], want[n][0], BF16, want[n][1])
        print(f"[parity] {scheme}-{n} {tag}: worst error/bound = {r:.3f}")
        if worst is not None:
            worst[n] = max(worst.get(n, 0.0), r)
        if not r <= 1.0:
            bad.append(f"{scheme}-{n} {tag}: error is {r:.3f} x the bound")
    assert not bad, "; ".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("T,D,p,qk_scale,alibi", PATHS + BIG)
def test_fused_bwd_softmax_paths(dev, T, D, p, qk_scale, alibi):
    q, k, v, do, slopes, want = _case(T, D, p, qk_scale, alibi)
    got = _run(dev, q, k, v, do, slopes, p, 1)
    _check("fused", _tag(T, D, p, qk_scale, alibi), got, want, WORST)


@pytest.mark.gpu
def test_fused_bwd_dk_dv_bitwise_reproducible(dev):
    """Each workgroup owns its keys' dK / dV outright; only dQ goes through
    atomics."""
    T, D, p = 300, 128, 0.3
    q, k, v, do, slopes, _ = _case(T, D, p, 1.0, True)
    a = _run(dev, q, k, v, do, slopes, p, 1)
    b = _run(dev, q, k, v, do, slopes, p, 1)
    for n in ("o", "lse", "dk", "dv"):
        assert torch.equal(a[n], b[n]), f"{n} differs between launches"


@pytest.mark.parametrize("T,D,p,qk_scale,alibi", PATHS + BIG)
def test_bounds_admit_emulation(T, D, p, qk_scale, alibi):
    """The fp32 emulation with the kernels' bf16 roundings stays within the
    bound at every shape above."""
    q, k, v, do, slopes, want = _case(T, D, p, qk_scale, alibi)
    keep = reference.drop_mask(P.ATTN_SEED, *P.ATTN_BH, T, p) if p > 0 else None
    got = attn_bwd_emul(q, k, v, do, slopes, keep, reference.drop_inv_keep(p))
    _check("emul", _tag(T, D, p, qk_scale, alibi), got, want)
