"""Float64 reference and derived bound for the prefill attention op
(ops.attention_prefill_append), shared by tests/test_prefill.py (CPU) and
tests/test_gpu_prefill.py. Uses the checker and constants of tests/_parity.py.
"""

from __future__ import annotations

import math

import torch

from . import _parity as P


def clamp_range(lens, start, T, S_alloc):
    """-> [(st, n)] per sequence, the op's documented clamps."""
    out = []
    for ln, st in zip(lens, start):
        st = min(max(int(st), 0), S_alloc)
        out.append((st, min(max(int(ln), 0), min(T, S_alloc - st))))
    return out


def expected_caches(qkv, k0, v0, H, ranges):
    """Old caches with rows [st, st + n) replaced by the k / v columns of qkv
    rows [0, n): what the op must leave, bit for bit."""
    B, T, C3 = qkv.shape
    C = C3 // 3
    D = C // H
    k_want, v_want = k0.clone(), v0.clone()
    for b, (st, n) in enumerate(ranges):
        if n:
            _, kn, vn = (t.reshape(n, H, D).transpose(0, 1)
                         for t in qkv[b, :n].split(C, dim=-1))
            k_want[b, :, st:st + n] = kn
            v_want[b, :, st:st + n] = vn
    return k_want, v_want


def prefill_ref(qkv, k_cache, v_cache, H, slopes, ranges, dtype):
    """Float64 prefill attention from the exact input bits.

    qkv (B, T, 3C); k_cache / v_cache (B, H, S_alloc, D) ALREADY holding the
    new rows (expected_caches); ranges = clamp_range(...). Only q rows < n and
    cache rows < st + n are read, so NaN elsewhere is harmless.
    -> [(want (n, C), abs_term (n, C))] per sequence.

    Row i sits at position st + i: score_j = q.k_j / sqrt(D) +
    slope * (j - (st + i)) over j <= st + i carries an fp32 error of
    ds = ACC * max_j (sum_d |q||k| / sqrt(D) + |bias_j|), so p_j = softmax has
    relative error 2 ds (tests/_parity.attn_decode_ref). The flash kernel
    also rounds P to the element type for the P.V matrix product while the
    normaliser sums the unrounded fp32 P: half an ulp (REL / 2) on each p_j,
    and as much again allowed for a normaliser that sums the rounded P
    instead, REL[dtype] together. Hence
        abs_term = (ACC + 2 ds + REL[dtype]) * sum_j p_j |v_j|;
    the checker (_parity.worst_ratio) adds the rounding of the output.
    """
    B, T, C3 = qkv.shape
    C = C3 // 3
    D = C // H
    sc = 1.0 / math.sqrt(D)
    out = []
    for b, (st, n) in enumerate(ranges):
        if n == 0:
            out.append((torch.zeros(0, C, dtype=torch.float64),) * 2)
            continue
        S = st + n
        Q = P.f64(qkv[b, :n, :C]).reshape(n, H, D).transpose(0, 1)  # (H, n, D)
        K, V = P.f64(k_cache[b, :, :S]), P.f64(v_cache[b, :, :S])   # (H, S, D)
        scores = (Q @ K.transpose(-1, -2)) * sc
        mag = (Q.abs() @ K.abs().transpose(-1, -2)) * sc
        rel = (torch.arange(S, dtype=torch.float64).view(1, S)
               - torch.arange(st, S, dtype=torch.float64).view(n, 1))
        if slopes is not None:
            bias = P.f64(slopes).view(H, 1, 1) * rel
            scores = scores + bias
            mag = mag + bias.abs()
        dead = rel > 0
        scores = scores.masked_fill(dead, -math.inf)
        mag = mag.masked_fill(dead, 0.0)
        p = torch.softmax(scores, -1)
        ds = P.ACC * mag.amax(-1, keepdim=True)
        want = (p @ V).transpose(0, 1).reshape(n, C)
        a = ((P.ACC + 2.0 * ds + P.REL[dtype]) * (p @ V.abs())).transpose(0, 1).reshape(n, C)
        out.append((want, a))
    return out
