"""Pure-PyTorch fp32-reference implementations of every fused HIP op.

These serve two purposes:
  1. CPU execution path (tests, gloo-based distributed plumbing tests).
  2. Numerics references for HIP-kernel parity tests (tests/test_ops_gpu.py):
     each HIP kernel is compared against the plain fp32 PyTorch op here.

Semantics mirror the JAX reference:
  - fp32 softmax in attention (reference src/models/layers.py:167-173 — bf16
    softmax caused a documented model failure, logs/580.md:94-98).
  - tanh-approximate GELU (flax nn.gelu default, reference layers.py:68).
  - one-hot-free shifted cross entropy in fp32 (reference src/utils/losses.py
    computes one-hot x log_softmax; we fuse the gather instead).
"""

from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F


def alibi_slopes(num_heads: int) -> torch.Tensor:
    """Standard ALiBi per-head slopes (Press et al., Train Short Test Long).

    Matches reference src/models/layers.py:17-30 (get_slopes).
    """

    def pow2_slopes(n: int):
        start = 2.0 ** (-(2.0 ** -(math.log2(n) - 3)))
        return [start * (start ** i) for i in range(n)]

    if math.log2(num_heads).is_integer():
        s = pow2_slopes(num_heads)
    else:
        p = 2 ** math.floor(math.log2(num_heads))
        extra = pow2_slopes(2 * p)[0::2][: num_heads - p]
        s = pow2_slopes(p) + extra
    return torch.tensor(s, dtype=torch.float32)


def attention(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    slopes: Optional[torch.Tensor] = None,
    dropout_p: float = 0.0,
    training: bool = False,
) -> torch.Tensor:
    """Causal multi-head attention with optional ALiBi bias, fp32 softmax.

    q, k, v: (B, H, T, D). Returns (B, H, T, D) in q.dtype.

    ALiBi bias for query i, key j (j <= i): slope_h * (j - i)  (<= 0).
    The reference applies the shift-invariant single-row form
    (layers.py:33-44); per-row they differ by a constant, so softmax output
    is identical.
    """
    B, H, T, D = q.shape
    scores = (q.float() @ k.float().transpose(-1, -2)) / math.sqrt(D)
    if slopes is not None:
        pos = torch.arange(T, device=q.device, dtype=torch.float32)
        rel = pos.view(1, T) - pos.view(T, 1)  # (j - i), negative below diag
        scores = scores + slopes.to(q.device).float().view(1, H, 1, 1) * rel.view(1, 1, T, T)
    causal = torch.ones(T, T, dtype=torch.bool, device=q.device).tril()
    scores = scores.masked_fill(~causal.view(1, 1, T, T), torch.finfo(torch.float32).min)
    probs = F.softmax(scores, dim=-1)
    if dropout_p > 0.0 and training:
        probs = F.dropout(probs, p=dropout_p)
    out = probs.to(v.dtype) @ v
    return out.to(q.dtype)


def attention_decode_append(
    qkv: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    num_head: int,
    slopes: Optional[torch.Tensor],
    lens: torch.Tensor,
) -> torch.Tensor:
    """One decode step on the fused projection, one sequence at a time.

    qkv: (B, 1, 3C); k_cache / v_cache: (B, H, S_alloc, D), written in place
    at row lens[b] - 1 with the new k / v; lens: (B,) int32 INCLUDING the new
    token. Sequence b attends over its rows [0, lens[b]) with the ALiBi bias
    slope_h * (j - (lens[b] - 1)); rows >= lens[b] are never read. fp32
    softmax; returns (B, 1, C) in qkv.dtype. lens[b] == 0 writes nothing and
    returns zeros for that row.
    """
    B, _, C3 = qkv.shape
    C = C3 // 3
    H = num_head
    D = C // H
    S_alloc = k_cache.shape[2]
    q, k_new, v_new = (t.reshape(B, H, D) for t in qkv.split(C, dim=-1))
    out = torch.zeros(B, H, D, dtype=torch.float32, device=qkv.device)
    for b, S in enumerate(lens.tolist()):
        S = min(max(int(S), 0), S_alloc)
        if S == 0:
            continue
        k_cache[b, :, S - 1] = k_new[b].to(k_cache.dtype)
        v_cache[b, :, S - 1] = v_new[b].to(v_cache.dtype)
        k = k_cache[b, :, :S].float()  # (H, S, D)
        v = v_cache[b, :, :S].float()
        scores = (k @ q[b].float().unsqueeze(-1)).squeeze(-1) / math.sqrt(D)
        if slopes is not None:
            pos = torch.arange(S, device=qkv.device, dtype=torch.float32) - (S - 1)
            scores = scores + slopes.to(qkv.device).float().view(H, 1) * pos
        probs = F.softmax(scores, dim=-1)  # (H, S)
        out[b] = (probs.unsqueeze(1) @ v).squeeze(1)
    return out.reshape(B, 1, C).to(qkv.dtype)


def attention_prefill_append(
    qkv: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    num_head: int,
    slopes: Optional[torch.Tensor],
    lens: Optional[torch.Tensor] = None,
    start: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Prefill (or one chunk of it) on the fused projection, one sequence at
    a time.

    qkv: (B, T, 3C); k_cache / v_cache: (B, H, S_alloc, D), written in place.
    lens[b] is the number of new rows of sequence b, start[b] the number of
    rows already in its cache (None: every row is new / nothing is cached).
    With st = clamp(start[b], 0, S_alloc) and
    n = clamp(lens[b], 0, min(T, S_alloc - st)), the k / v columns of rows
    i < n go to cache rows st + i and no other cache row is touched; query row
    i < n sits at position st + i and attends over cache rows [0, st + i]
    with the ALiBi bias slope_h * (j - (st + i)). fp32 softmax; returns
    (B, T, C) in qkv.dtype with rows i >= n zero. Rows >= n of qkv and cache
    rows >= st + n are never read.
    """
    B, T, C3 = qkv.shape
    C = C3 // 3
    H = num_head
    D = C // H
    S_alloc = k_cache.shape[2]
    lens_l = [T] * B if lens is None else lens.tolist()
    start_l = [0] * B if start is None else start.tolist()
    out = torch.zeros(B, T, C, dtype=torch.float32, device=qkv.device)
    for b in range(B):
        st = min(max(int(start_l[b]), 0), S_alloc)
        n = min(max(int(lens_l[b]), 0), min(T, S_alloc - st))
        if n == 0:
            continue
        q, k_new, v_new = (
            t.reshape(n, H, D).transpose(0, 1) for t in qkv[b, :n].split(C, dim=-1)
        )  # (H, n, D)
        k_cache[b, :, st:st + n] = k_new.to(k_cache.dtype)
        v_cache[b, :, st:st + n] = v_new.to(v_cache.dtype)
        S = st + n
        k = k_cache[b, :, :S].float()  # (H, S, D)
        v = v_cache[b, :, :S].float()
        scores = (q.float() @ k.transpose(-1, -2)) / math.sqrt(D)  # (H, n, S)
        qpos = torch.arange(st, S, device=qkv.device, dtype=torch.float32)
        kpos = torch.arange(S, device=qkv.device, dtype=torch.float32)
        rel = kpos.view(1, S) - qpos.view(n, 1)  # j - (st + i)
        if slopes is not None:
            scores = scores + slopes.to(qkv.device).float().view(H, 1, 1) * rel
        scores = scores.masked_fill(rel > 0, torch.finfo(torch.float32).min)
        probs = F.softmax(scores, dim=-1)
        out[b, :n] = (probs @ v).transpose(0, 1).reshape(n, C)
    return out.to(qkv.dtype)


def paged_gather(pool: torch.Tensor, block_table: torch.Tensor) -> torch.Tensor:
    """The logical caches of a paged pool: pool (P, H, R, D), block_table
    (B, M) -> (B, H, M*R, D), a copy. Page ids are clamped to [0, P)."""
    P, H, R, D = pool.shape
    B, M = block_table.shape
    pages = pool[block_table.long().clamp(0, P - 1)]  # (B, M, H, R, D)
    return pages.permute(0, 2, 1, 3, 4).reshape(B, H, M * R, D)


def _paged_scatter_rows(pool, block_table, cache, b: int, lo: int, hi: int) -> None:
    """pool rows of sequence b's logical rows [lo, hi) <- cache[b, :, lo:hi]."""
    P, _, R, _ = pool.shape
    for j in range(lo, hi):
        page = min(max(int(block_table[b, j // R]), 0), P - 1)
        pool[page, :, j % R] = cache[b, :, j]


def attention_prefill_paged(
    qkv: torch.Tensor,
    k_pool: torch.Tensor,
    v_pool: torch.Tensor,
    num_head: int,
    slopes: Optional[torch.Tensor],
    block_table: torch.Tensor,
    lens: Optional[torch.Tensor] = None,
    start: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """attention_prefill_append on a paged cache: k_pool / v_pool (P, H, R, D)
    written in place, block_table (B, M) int32; logical row j of sequence b is
    pool[block_table[b, j // R], :, j % R] and S_alloc = M * R. Gathers each
    sequence's pages, runs the contiguous reference and scatters the rows it
    wrote, [st, st + n), back: no other pool row changes."""
    B, T, _ = qkv.shape
    R = k_pool.shape[2]
    S_alloc = block_table.shape[1] * R
    k = paged_gather(k_pool, block_table)
    v = paged_gather(v_pool, block_table)
    out = attention_prefill_append(qkv, k, v, num_head, slopes, lens, start)
    lens_l = [T] * B if lens is None else lens.tolist()
    start_l = [0] * B if start is None else start.tolist()
    for b in range(B):
        st = min(max(int(start_l[b]), 0), S_alloc)
        n = min(max(int(lens_l[b]), 0), min(T, S_alloc - st))
        _paged_scatter_rows(k_pool, block_table, k, b, st, st + n)
        _paged_scatter_rows(v_pool, block_table, v, b, st, st + n)
    return out


def attention_decode_paged(
    qkv: torch.Tensor,
    k_pool: torch.Tensor,
    v_pool: torch.Tensor,
    num_head: int,
    slopes: Optional[torch.Tensor],
    block_table: torch.Tensor,
    lens: torch.Tensor,
) -> torch.Tensor:
    """attention_decode_append on a paged cache (layout as in
    attention_prefill_paged): the new row lands at logical row lens[b] - 1 of
    sequence b; lens[b] == 0 writes nothing and returns zeros."""
    S_alloc = block_table.shape[1] * k_pool.shape[2]
    k = paged_gather(k_pool, block_table)
    v = paged_gather(v_pool, block_table)
    out = attention_decode_append(qkv, k, v, num_head, slopes, lens)
    for b, S in enumerate(lens.tolist()):
        S = min(max(int(S), 0), S_alloc)
        if S:
            _paged_scatter_rows(k_pool, block_table, k, b, S - 1, S)
            _paged_scatter_rows(v_pool, block_table, v, b, S - 1, S)
    return out


def drop_mask(seed: int, B: int, H: int, T: int, p: float) -> torch.Tensor:
    """Regenerate the attention-dropout keep mask of the HIP kernels.

    Exact Python mirror of csrc/common.h drop_bits32 (murmur3-finalizer
    mix32; 4x 8-bit thresholds per hash over key groups of 4). Returns a
    bool (B, H, T, T) tensor: True = keep. Used by GPU parity tests to
    compare kernel backward against autograd with the explicit mask.
    """
    import numpy as np

    thr = int(p * 256.0 + 0.5)

    def mix32(x):
        x = x.astype(np.uint32, copy=True)
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x85EBCA6B)
        x ^= x >> np.uint32(13)
        x *= np.uint32(0xC2B2AE35)
        x ^= x >> np.uint32(16)
        return x

    bh = np.arange(B * H, dtype=np.uint32)
    qi = np.arange(T, dtype=np.uint32)
    kg = np.arange((T + 3) // 4, dtype=np.uint32)
    bhT_qi = (bh[:, None] * np.uint32(T) + qi[None, :]).reshape(-1, 1)  # (BH*T, 1)
    with np.errstate(over="ignore"):
        x = (
            np.uint32(seed)
            ^ (bhT_qi * np.uint32(0x9E3779B9))
            ^ (kg[None, :] * np.uint32(0x85EBCA6B))
        )
        bits = mix32(x)  # (BH*T, ceil(T/4))
    bytes_ = np.stack([(bits >> np.uint32(8 * e)) & np.uint32(0xFF) for e in range(4)], axis=-1)
    keep = (bytes_ >= np.uint32(thr)).reshape(B * H * T, -1)[:, :T]
    return torch.from_numpy(keep.reshape(B, H, T, T).copy())


def residual_drop_mask(seed: int, n: int, p: float) -> torch.Tensor:
    """Mirror of csrc/residual.hip's element mask: element i keeps iff byte
    (i & 3) of drop_bits32(seed, i4 >> 16, i4 & 0xffff) >= thr, i4 = i >> 2."""
    import numpy as np

    thr = int(p * 256.0 + 0.5)

    def mix32(x):
        x = x.astype(np.uint32, copy=True)
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x85EBCA6B)
        x ^= x >> np.uint32(13)
        x *= np.uint32(0xC2B2AE35)
        x ^= x >> np.uint32(16)
        return x

    i4 = np.arange((n + 3) // 4, dtype=np.uint64)
    hi = (i4 >> np.uint64(16)).astype(np.uint32)
    lo = (i4 & np.uint64(0xFFFF)).astype(np.uint32)
    with np.errstate(over="ignore"):
        bits = mix32(
            np.uint32(seed) ^ (hi * np.uint32(0x9E3779B9)) ^ (lo * np.uint32(0x85EBCA6B))
        )
    by = np.stack([(bits >> np.uint32(8 * e)) & np.uint32(0xFF) for e in range(4)], -1)
    keep = (by >= np.uint32(thr)).reshape(-1)[:n]
    return torch.from_numpy(keep.copy())


def uniform01(seed: int, counter: int) -> float:
    """Python-integer mirror of csrc/common.h uniform01 (splitmix64 finalizer,
    top 24 bits): the uniform in [0, 1) that the HIP sampler draws for
    (seed, counter). Both are taken modulo 2**64."""
    M = (1 << 64) - 1

    def mix64(x):
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)

    return (mix64((int(seed) & M) ^ mix64(int(counter) & M)) >> 40) / 16777216.0


def sample_rows(logits, seen, temperature, top_k, top_p, penalty, seed, counter):
    """The definition of ops.sample_rows in float64, one row at a time (the
    oracle of the HIP sampler; also what CPU tensors take).

    logits (B, V) float; seen (B, V) bool or None; temperature, top_p, penalty
    (B,) float32; top_k (B,) int32; seed, counter (B,) int64 ->
    (tokens (B,) int64, cut (B,) float32). Per row, with x = logits[b]:

    1. penalty: where seen and penalty != 1, y = x / r if x > 0 else x * r,
       computed and rounded as apply_repetition_penalty_batched does (in the
       dtype of logits); otherwise y = x.
    2. greedy (temperature <= 0): token = lowest index of max y, cut = max y.
    3. top-k: kth = the k-th largest y, ties counted, if 0 < k < V, else -inf;
       K = {y >= kth} (ties at kth are all kept).
    4. weights w = exp((y - max y) / max(T, 1e-5)) on K.
    5. top-p (p < 1): cut = the largest value v in y_K whose upper mass
       sum{w : y >= v} exceeds p * sum_K w, else cut = kth; S = K & {y >= cut}
       (values tied with the cut are all kept; never empty).
    6. draw: u = uniform01(seed, counter); token = the smallest i in S, in
       token order, whose inclusive mass over S exceeds u * sum_S w, or the
       largest i in S if rounding leaves none.
    """
    B, V = logits.shape
    toks = torch.zeros(B, dtype=torch.long)
    cuts = torch.zeros(B, dtype=torch.float32)
    neg_inf = float("-inf")
    for b in range(B):
        x = logits[b]
        r = float(penalty[b])
        if seen is not None and r != 1.0:
            x = torch.where(seen[b], torch.where(x > 0, x / r, x * r), x)
        y = x.detach().to("cpu", torch.float64)
        y = torch.where(y.isnan(), torch.full_like(y, neg_inf), y)
        m = float(y.max())
        T = float(temperature[b])
        if not T > 0.0:
            toks[b], cuts[b] = int(y.argmax()), m
            continue
        k = int(top_k[b])
        kth = float(torch.topk(y, k).values[-1]) if 0 < k < V else neg_inf
        keep = y >= kth
        w = torch.exp((y - m) / max(T, 1e-5)) * keep
        cut = kth
        p = max(float(top_p[b]), 0.0)
        if p < 1.0:
            ys, order = torch.sort(y[keep], descending=True)
            upper = torch.cumsum(w[keep][order], 0)  # mass{y >= ys[j]} at a group's end
            ends = torch.ones_like(ys, dtype=torch.bool)
            ends[:-1] = ys[1:] != ys[:-1]
            ok = ends & (upper > p * float(w.sum()))
            if bool(ok.any()):
                cut = max(float(ys[int(ok.nonzero()[0])]), kth)
        in_s = keep & (y >= cut)
        cdf = torch.cumsum(w * in_s, 0)
        u = uniform01(int(seed[b]), int(counter[b]))
        hit = (in_s & (cdf > u * float(cdf[-1]))).nonzero()
        members = in_s.nonzero()
        if hit.numel():
            tok = int(hit[0])
        else:
            tok = int(members[-1]) if members.numel() else 0
        toks[b], cuts[b] = min(max(tok, 0), V - 1), cut
    return toks.to(logits.device), cuts.to(logits.device)


def drop_inv_keep(p: float) -> float:
    """Rescale factor matching the kernels' realized 8-bit threshold."""
    thr = int(p * 256.0 + 0.5)
    return 256.0 / (256.0 - thr) if thr else 1.0


def attention_with_mask(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    slopes: Optional[torch.Tensor],
    keep: torch.Tensor,
    inv_keep: float,
) -> torch.Tensor:
    """Reference attention with an explicit dropout keep-mask on the probs
    (denominator keeps the full softmax, matching the fused kernel)."""
    B, H, T, D = q.shape
    scores = (q.float() @ k.float().transpose(-1, -2)) / math.sqrt(D)
    if slopes is not None:
        pos = torch.arange(T, device=q.device, dtype=torch.float32)
        rel = pos.view(1, T) - pos.view(T, 1)
        scores = scores + slopes.to(q.device).float().view(1, H, 1, 1) * rel.view(1, 1, T, T)
    causal = torch.ones(T, T, dtype=torch.bool, device=q.device).tril()
    scores = scores.masked_fill(~causal.view(1, 1, T, T), torch.finfo(torch.float32).min)
    probs = F.softmax(scores, dim=-1)
    probs = probs * keep.to(probs.dtype).to(probs.device) * inv_keep
    out = probs.to(v.dtype) @ v
    return out.to(q.dtype)


def layer_norm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """Bias-free LayerNorm in fp32, cast back to input dtype.

    Matches flax nn.LayerNorm(use_bias=False) (reference src/models/GPT.py:42).
    """
    y = F.layer_norm(x.float(), (x.shape[-1],), weight=weight.float(), bias=None, eps=eps)
    return y.to(x.dtype)


def gelu(x: torch.Tensor) -> torch.Tensor:
    """tanh-approximate GELU (flax default, reference layers.py:68)."""
    return F.gelu(x, approximate="tanh")


def cross_entropy(logits: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """Mean cross entropy over all positions, fp32 log-softmax.

    logits: (N, V), targets: (N,) int64. Equivalent to the reference's
    one-hot * log_softmax mean (src/utils/losses.py:10-23) without
    materializing the one-hot.
    """
    return F.cross_entropy(logits.float(), targets, ignore_index=-1)


def grad_sumsq(grad: torch.Tensor) -> torch.Tensor:
    """fp32 sum of squares of a gradient shard as stored (the grad-norm
    metric's per-shard term; the GPU AdamW kernel returns the same sum)."""
    return grad.float().square().sum()


def adamw_update(
    param_f32: torch.Tensor,
    grad: torch.Tensor,
    exp_avg: torch.Tensor,
    exp_avg_sq: torch.Tensor,
    step: int,
    lr: float,
    beta1: float,
    beta2: float,
    eps: float,
    weight_decay: float,
    clip_value: float = 1.0,
    grad_scale: float = 1.0,
) -> None:
    """In-place AdamW on an fp32 master shard, reference semantics.

    Order matches the reference optax chain (main_zero.py:160-168):
    grad * grad_scale (the 1/accum divide of xmap_train_functions.py:81),
    element-wise clip of the gradient to +-clip_value (optax.clip(1.0) —
    NOT global-norm clipping), then scale_by_adam(b2=0.95), then masked
    weight decay, then -lr scaling.  Decoupled decay: update includes
    weight_decay * param (optax.add_decayed_weights semantics).
    """
    g = grad.float() * grad_scale
    if clip_value:
        g.clamp_(-clip_value, clip_value)
    exp_avg.mul_(beta1).add_(g, alpha=1 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    m_hat = exp_avg / bc1
    v_hat = exp_avg_sq / bc2
    update = m_hat / (v_hat.sqrt() + eps)
    if weight_decay:
        update = update + weight_decay * param_f32
    param_f32.add_(update, alpha=-lr)
