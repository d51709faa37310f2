"""KV-cached inference GPT (the torch_compatability sidecar model).

Same capability as the reference's PyTorch inference mirror
(torch_compatability/GPT2.py:49-474): ALiBi attention via
scaled_dot_product_attention with an additive mask, per-layer KV cache
(concat along the sequence axis), dynamic ALiBi mask rebuild when the
context grows, weight-tied lm_head, greedy/sampling generate, shifted CE
loss. Loads / saves the .pth state-dict contract
(flax_to_pytorch.py:10-35,96-114 key layout).
"""

from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..ops.reference import alibi_slopes
from ..utils.config import load_config


def _proj(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """Linear that routes single-token decode through the weight-streaming
    GEMV kernel (ops.decode_linear); prefill/CPU keep F.linear."""
    if x.shape[-2] == 1:
        return ops.decode_linear(x, w)
    return F.linear(x, w)


class StaticKVCache:
    """Preallocated per-layer KV buffers with DEVICE-side per-sequence lengths.

    Makes the whole decode step hipGraph-replayable: the cache write position
    and the decode-attention kernel's live length both come from device
    memory (ops.attention_decode_append reads `len_t` in-kernel and appends
    the new row at len - 1), so one captured graph serves every token as the
    cache grows. `len_t` is (batch,) int32: sequences of a batch may differ
    in length.
    """

    def __init__(self, n_layers: int, batch: int, heads: int, head_dim: int,
                 max_ctx: int, device, dtype):
        self.k = [torch.zeros(batch, heads, max_ctx, head_dim, device=device,
                              dtype=dtype) for _ in range(n_layers)]
        self.v = [torch.zeros(batch, heads, max_ctx, head_dim, device=device,
                              dtype=dtype) for _ in range(n_layers)]
        self.len_t = torch.zeros(batch, dtype=torch.int32, device=device)
        self.max_ctx = max_ctx

    def advance(self, n=1):
        """Add an int, or a (B,) int32 device tensor (0/1 per sequence: only
        the active ones grow). Device adds: correct inside a graph replay."""
        self.len_t += n

    # The attention layers reach a cache through these two calls, so that
    # another cache kind (models/paged.py) brings its own addressing.
    def attend_decode(self, layer_idx, qkv, num_head, slopes):
        return ops.attention_decode_append(
            qkv, self.k[layer_idx], self.v[layer_idx], num_head, slopes, self.len_t)

    def attend_prefill(self, layer_idx, qkv, num_head, slopes, lens, start):
        return ops.attention_prefill_append(
            qkv, self.k[layer_idx], self.v[layer_idx], num_head, slopes, lens, start)

    def set_len(self, n):
        """An int (every sequence) or a length-B sequence / tensor."""
        if isinstance(n, int):
            self.len_t.fill_(n)
        else:
            self.len_t.copy_(torch.as_tensor(n, dtype=torch.int32))


def _alibi_bias(slopes: torch.Tensor, Tq: int, Tk: int, device, dtype) -> torch.Tensor:
    """Additive (H, Tq, Tk) mask: ALiBi bias + causal -inf.

    For decode (Tq < Tk) the q rows are the LAST Tq positions of the Tk
    context (reference GPT2.py:193-235: decode path uses the last-row mask).
    """
    H = slopes.shape[0]
    qpos = torch.arange(Tk - Tq, Tk, device=device, dtype=torch.float32)
    kpos = torch.arange(Tk, device=device, dtype=torch.float32)
    rel = kpos.view(1, Tk) - qpos.view(Tq, 1)  # j - i
    bias = slopes.to(device).float().view(H, 1, 1) * rel.view(1, Tq, Tk)
    bias = bias.masked_fill(rel.view(1, Tq, Tk) > 0, float("-inf"))
    return bias.to(dtype)


class InferenceAttention(nn.Module):
    def __init__(self, dim: int, heads: int, alibi: bool = True):
        super().__init__()
        self.num_head = heads
        self.head_dim = dim // heads
        self.query = nn.Linear(dim, dim, bias=False)
        self.key = nn.Linear(dim, dim, bias=False)
        self.value = nn.Linear(dim, dim, bias=False)
        self.fc_resid = nn.Linear(dim, dim, bias=False)
        if alibi:
            self.register_buffer("slopes", alibi_slopes(heads), persistent=False)
        else:
            self.slopes = None

    def _load_from_state_dict(self, *args, **kwargs):
        # invalidate the lazily-fused decode qkv weight on checkpoint load
        self._qkv_w = None
        super()._load_from_state_dict(*args, **kwargs)

    def _fused_qkv_w(self, dtype) -> torch.Tensor:
        """The (3C, C) q|k|v weight, materialized lazily."""
        if getattr(self, "_qkv_w", None) is None or self._qkv_w.dtype != dtype:
            self._qkv_w = torch.cat(
                [self.query.weight, self.key.weight, self.value.weight], dim=0
            ).contiguous()
        return self._qkv_w

    def forward(
        self,
        x: torch.Tensor,
        layer_past: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
        use_cache: bool = False,
        static_cache: Optional["StaticKVCache"] = None,
        layer_idx: int = 0,
    ):
        B, T, C = x.shape
        H, D = self.num_head, self.head_dim
        if T == 1 and (x.is_cuda or static_cache is not None):
            # decode: one fused (3C, C) GEMV instead of three launches (the
            # fused weight is materialized lazily; same total weight-stream
            # bytes, 1/3 the kernel launches and a fuller grid)
            qkv = ops.decode_linear(x, self._fused_qkv_w(x.dtype))
            if static_cache is not None:
                # the kernel reads q / k / v straight from the projection
                # row, appends k / v at device position len-1 (len already
                # advanced for this token, per sequence) and attends over
                # the live cache — fully graph-replayable
                out = static_cache.attend_decode(layer_idx, qkv, H, self.slopes)
                return _proj(out, self.fc_resid.weight), None
            q, k, v = qkv.split(C, dim=-1)
            q = q.view(B, T, H, D).transpose(1, 2)
            k = k.view(B, T, H, D).transpose(1, 2)
            v = v.view(B, T, H, D).transpose(1, 2)
        else:
            q = _proj(x, self.query.weight).view(B, T, H, D).transpose(1, 2)
            k = _proj(x, self.key.weight).view(B, T, H, D).transpose(1, 2)
            v = _proj(x, self.value.weight).view(B, T, H, D).transpose(1, 2)
        if static_cache is not None:
            assert isinstance(static_cache, StaticKVCache), \
                "a paged cache is filled through GPT2.prefill"
            kc, vc = static_cache.k[layer_idx], static_cache.v[layer_idx]
            # prefill: fill rows [0, T) and fall through to the SDPA path
            idxs = torch.arange(T, device=x.device)
            kc.index_copy_(2, idxs, k.to(kc.dtype))
            vc.index_copy_(2, idxs, v.to(vc.dtype))
        if layer_past is not None:
            pk, pv = layer_past
            k = torch.cat([pk, k], dim=2)  # concat along seq (GPT2.py:177-182)
            v = torch.cat([pv, v], dim=2)
        present = (k, v) if use_cache else None
        Tk = k.shape[2]
        if (
            T == 1
            and x.is_cuda
            and q.dtype in (torch.bfloat16, torch.float16)
            and D <= 256
        ):
            # MI355X-native decode kernel (ops/csrc/attn_decode.hip) — the
            # torch-SDPA path below stays for prefill / CPU
            out = ops.attention_decode(q.contiguous(), k.contiguous(),
                                       v.contiguous(), self.slopes)
        elif self.slopes is not None:
            mask = _alibi_bias(self.slopes, T, Tk, x.device, q.dtype).unsqueeze(0)
            out = F.scaled_dot_product_attention(q, k, v, attn_mask=mask)
        else:
            if T == Tk:
                out = F.scaled_dot_product_attention(q, k, v, is_causal=True)
            else:
                causal = torch.zeros(T, Tk, device=x.device, dtype=q.dtype)
                rel = torch.arange(Tk, device=x.device).view(1, Tk) - torch.arange(
                    Tk - T, Tk, device=x.device
                ).view(T, 1)
                causal = causal.masked_fill(rel > 0, float("-inf"))
                out = F.scaled_dot_product_attention(q, k, v, attn_mask=causal.view(1, 1, T, Tk))
        out = out.transpose(1, 2).reshape(B, T, C)
        return _proj(out, self.fc_resid.weight), present

    def prefill(self, x: torch.Tensor, cache: "StaticKVCache", layer_idx: int,
                lens: torch.Tensor, start: torch.Tensor) -> torch.Tensor:
        """Prompt rows (or one chunk of them) through the native prefill
        kernel: one fused qkv GEMM, ops.attention_prefill_append (fills cache
        rows start[b]..start[b]+lens[b] and attends over the cache; no mask
        tensor, no index_copy_), the output projection."""
        qkv = F.linear(x, self._fused_qkv_w(x.dtype))
        out = cache.attend_prefill(layer_idx, qkv, self.num_head, self.slopes,
                                   lens, start)
        return F.linear(out, self.fc_resid.weight)


class InferenceMLP(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.fc1 = nn.Linear(dim, 4 * dim, bias=False)
        self.fc_resid = nn.Linear(4 * dim, dim, bias=False)

    def forward(self, x):
        h = _proj(x, self.fc1.weight)
        if x.shape[-2] == 1 and x.is_cuda and not torch.is_grad_enabled():
            # decode: in-house fp16/bf16 gelu kernel (torch's fp16 tanh-gelu
            # pays extra fp32 copy kernels that dominate at (B, 1, 4C) sizes)
            h = ops.gelu(h)
        else:
            h = F.gelu(h, approximate="tanh")
        return _proj(h, self.fc_resid.weight)


class InferenceBlock(nn.Module):
    def __init__(self, dim: int, heads: int, alibi: bool = True):
        super().__init__()
        self.ln1 = nn.LayerNorm(dim, elementwise_affine=True, bias=False, eps=1e-6)
        self.attn = InferenceAttention(dim, heads, alibi)
        self.ln2 = nn.LayerNorm(dim, elementwise_affine=True, bias=False, eps=1e-6)
        self.mlp = InferenceMLP(dim)

    def forward(self, x, layer_past=None, use_cache=False, static_cache=None,
                layer_idx=0):
        a, present = self.attn(self.ln1(x), layer_past, use_cache,
                               static_cache=static_cache, layer_idx=layer_idx)
        x = x + a
        x = x + self.mlp(self.ln2(x))
        return x, present


class GPT2(nn.Module):
    """Inference model (reference torch_compatability/GPT2.py:297-445)."""

    def __init__(self, embedding_dim: int, vocab_size: int, num_head: int,
                 num_ctx: int, N: int, alibi: bool = True):
        super().__init__()
        self.N = N
        self.vocab_size = vocab_size
        self.num_ctx = num_ctx
        self.wte = nn.Embedding(vocab_size, embedding_dim)
        self.blocks = nn.ModuleList(
            [InferenceBlock(embedding_dim, num_head, alibi) for _ in range(N)]
        )
        self.norm = nn.LayerNorm(embedding_dim, elementwise_affine=True, bias=False, eps=1e-6)
        self.lm_head = nn.Linear(embedding_dim, vocab_size, bias=False)
        self.lm_head.weight = self.wte.weight  # tied (GPT2.py:350)

    def forward(
        self,
        idx: torch.Tensor,
        labels: Optional[torch.Tensor] = None,
        use_cache: bool = False,
        past_states: Optional[List] = None,
        static_cache: Optional[StaticKVCache] = None,
    ):
        x = self.wte(idx)
        if (
            idx.shape[1] == 1
            and x.is_cuda
            and static_cache is not None
            and not use_cache
            and labels is None
        ):
            return self._decode_step(x, static_cache)
        presents = [] if use_cache else None
        if past_states is None:
            past_states = [None] * self.N
        for i, (block, past) in enumerate(zip(self.blocks, past_states)):
            x, present = block(x, past, use_cache, static_cache=static_cache,
                               layer_idx=i)
            if use_cache:
                presents.append(present)
        x = self.norm(x)
        logits = _proj(x, self.lm_head.weight)
        if labels is not None:
            tgt = labels[..., 1:].reshape(-1)
            lg = logits[..., :-1, :].reshape(-1, logits.shape[-1])
            loss = F.cross_entropy(lg.float(), tgt)
            return logits, loss
        if use_cache:
            return logits, presents
        return logits

    @torch.no_grad()
    def _decode_step(self, x: torch.Tensor, cache: StaticKVCache) -> torch.Tensor:
        """Single-token decode with fused residual+LayerNorm boundaries:
        each block runs attn(ln1(x)) and mlp(ln2(x+a)) with the add and the
        FOLLOWING LayerNorm in one kernel (ops.add_ln) — the unfused path's
        four ~4.5 us elementwise/LN launches per layer were ~0.45 ms of the
        per-token budget. Identical math, verified against Block.forward by
        the GPU decode parity tests."""
        eps = self.blocks[0].ln1.eps
        ln_x = F.layer_norm(x, x.shape[-1:], weight=self.blocks[0].ln1.weight,
                            eps=eps)
        for i, block in enumerate(self.blocks):
            a, _ = block.attn(ln_x, None, False, static_cache=cache, layer_idx=i)
            x, ln2_x = ops.add_ln(x, a, block.ln2.weight, eps)
            m = block.mlp(ln2_x)
            next_w = (
                self.blocks[i + 1].ln1.weight if i + 1 < self.N else self.norm.weight
            )
            x, ln_x = ops.add_ln(x, m, next_w, eps)
        # ln_x is now norm(x)
        return _proj(ln_x, self.lm_head.weight)

    @torch.no_grad()
    def prefill(
        self,
        idx: torch.Tensor,
        cache: StaticKVCache,
        lens=None,
        chunk: Optional[int] = None,
        start=None,
    ) -> torch.Tensor:
        """Fill `cache` from the prompts and return each sequence's
        last-token logits, (B, V).

        `cache` is a StaticKVCache, or a paged cache or a view of some of its
        slots (models/paged.py). `start` (None: nothing) is the number of rows
        each sequence already has cached, e.g. a shared prefix: idx then holds
        the tokens behind them, and `lens` counts those.

        idx: (B, T) right-padded prompts; lens: one length per sequence (a
        sequence or a (B,) tensor; None: all T). Per layer: one fused qkv
        GEMM, ops.attention_prefill_append, the output projection, the MLP.
        Pad rows are never written to the cache and attend to nothing. Each
        sequence's last hidden row is gathered on device before the final
        norm, so norm and lm_head run on (B, 1, C).

        chunk=P sends the prompt through in slices of P positions (slice c
        holds lens_c = clamp(lens - cP, 0, P) new rows behind
        start_c = min(lens, cP) cached ones), which bounds the activation
        memory of a long prompt; the result is the unchunked one up to
        rounding. `cache.len_t` is left to the caller. A one-token prompt
        goes through the decode step, which appends at row len_t - 1.
        """
        B, T = idx.shape
        if T == 1:
            return self(idx, static_cache=cache)[:, -1]
        dev = idx.device
        if lens is None:
            lens_t = torch.full((B,), T, dtype=torch.int32, device=dev)
        else:
            lens_t = torch.as_tensor(lens, dtype=torch.int32).to(dev)
        start_t = (None if start is None
                   else torch.as_tensor(start, dtype=torch.int32).to(dev))
        P = T if not chunk else max(1, min(int(chunk), T))
        rows = torch.arange(B, device=dev)
        last = None
        for c0 in range(0, T, P):
            x = self.wte(idx[:, c0:c0 + P])
            Pc = x.shape[1]
            lens_c = (lens_t - c0).clamp(0, Pc)
            start_c = lens_t.clamp(max=c0)
            if start_t is not None:
                start_c = start_c + start_t
            for i, block in enumerate(self.blocks):
                x = x + block.attn.prefill(block.ln1(x), cache, i, lens_c, start_c)
                x = x + block.mlp(block.ln2(x))
            # the slice that holds row lens - 1 supplies it (device select)
            pos = lens_t.long() - 1 - c0
            here = (pos >= 0) & (pos < Pc)
            row = x[rows, pos.clamp(0, Pc - 1)]  # (B, C)
            last = row if last is None else torch.where(here.view(B, 1), row, last)
        x = self.norm(last.unsqueeze(1))
        return _proj(x, self.lm_head.weight)[:, 0]

    @torch.no_grad()
    def generate(
        self,
        idx: torch.Tensor,
        max_new_tokens: int,
        temperature: float = 1.0,
        sample: bool = False,
        top_k: Optional[int] = None,
    ) -> torch.Tensor:
        """Simple no-cache generate (reference GPT2.py:354-400, lm-eval path)."""
        for _ in range(max_new_tokens):
            ctx = idx[:, -self.num_ctx:]
            logits = self.forward(ctx)
            logits = logits[:, -1, :] / max(temperature, 1e-5)
            if top_k is not None:
                v, _ = torch.topk(logits, min(top_k, logits.size(-1)))
                logits[logits < v[:, [-1]]] = float("-inf")
            probs = F.softmax(logits.float(), dim=-1)
            nxt = torch.multinomial(probs, 1) if sample else probs.argmax(-1, keepdim=True)
            idx = torch.cat([idx, nxt], dim=1)
        return idx


# Graph warm-up + capture run the decode step this many times, writing
# scratch KV rows len..len+2 of every sequence before the lengths are rewound:
# callers size the static buffers with that headroom (clamped to num_ctx) and
# skip capture when the longest prompt is within 3 rows of the context limit.
GRAPH_SCRATCH_ROWS = 3

# generate_batch asks the device whether every row has finished once per this
# many steps: one host sync per check, at most this many - 1 wasted steps.
FINISHED_CHECK_EVERY = 16


def capture_decode_step(step, cache: StaticKVCache, lens):
    """Warm `step` up on a side stream, capture it in a hipGraph and rewind
    the cache lengths to `lens` (an int or one length per sequence): the
    warm-up and the capture advanced every sequence and wrote 3 fake rows
    behind it, which real tokens overwrite as the lengths re-advance.
    Returns (graph, step's captured output buffer)."""
    warm = torch.cuda.Stream()
    warm.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(warm):
        for _ in range(GRAPH_SCRATCH_ROWS - 1):
            step()
    torch.cuda.current_stream().wait_stream(warm)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    cache.set_len(lens)
    return graph, out


@torch.no_grad()
def generate_fast(
    model: "GPT2",
    idx: torch.Tensor,
    max_new_tokens: int,
    use_graph: bool = True,
    prefill_chunk: Optional[int] = None,
) -> torch.Tensor:
    """Greedy generation with a static KV cache and (optionally) the whole
    per-token decode step captured in a hipGraph — removes the per-layer
    Python/launch overhead that dominates single-token latency. The prompt
    goes through GPT2.prefill, in slices of `prefill_chunk` positions if set.
    """
    B, T0 = idx.shape
    dev = idx.device
    p = next(model.parameters())
    H = model.blocks[0].attn.num_head
    D = model.blocks[0].attn.head_dim
    max_ctx = min(model.num_ctx, T0 + max_new_tokens)
    cache_rows = min(model.num_ctx, max_ctx + GRAPH_SCRATCH_ROWS)
    use_graph = (use_graph and dev.type == "cuda"
                 and cache_rows - T0 >= GRAPH_SCRATCH_ROWS)
    cache = StaticKVCache(model.N, B, H, D, cache_rows, dev, p.dtype)

    # prefill. The length goes first: a one-token prompt prefills through
    # the decode step, which appends at row len - 1 (T0 > 1 never reads it)
    cache.set_len(T0)
    last = model.prefill(idx, cache, chunk=prefill_chunk)
    cur = last.argmax(-1, keepdim=True)  # (B, 1) — static input buffer
    out_tokens = [cur.clone()]

    def step():
        cache.advance(1)
        return model(cur, static_cache=cache)

    graph = None
    if use_graph:
        graph, logits_buf = capture_decode_step(step, cache, T0)

    for i in range(max_new_tokens - 1):
        if T0 + 1 + i >= max_ctx:
            break
        if graph is not None:
            graph.replay()
            nxt = logits_buf[:, -1:].argmax(-1)
        else:
            nxt = step()[:, -1:].argmax(-1)
        cur.copy_(nxt)
        out_tokens.append(nxt.clone())
    return torch.cat([idx] + out_tokens, dim=1)


@torch.no_grad()
def generate_batch(
    model: "GPT2",
    prompts: Sequence[Sequence[int]],
    max_new_tokens: int,
    *,
    eos_token: Optional[int] = None,
    sample: bool = False,
    temperature: float = 1.0,
    top_k: int = 0,
    top_p: float = 1.0,
    repetition_penalty: float = 1.0,
    use_graph: bool = True,
    prefill_chunk: Optional[int] = None,
) -> List[List[int]]:
    """Batched generation for prompts of DIFFERENT lengths (each >= 1 and
    <= model.num_ctx), on the model's device.

    Returns the generated tokens per prompt, without the prompt, cut before
    the first `eos_token`. Row b yields at most
    min(max_new_tokens, num_ctx - len(prompts[b])) tokens — generate_fast's
    rule per sequence.

    One right-padded GPT2.prefill with the per-sequence lengths fills the
    static cache (in slices of `prefill_chunk` positions if set): the pad
    rows attend to nothing and are never written to the cache, and only each
    sequence's last row reaches the lm_head. Decode then runs
    with per-sequence lengths (StaticKVCache.len_t), sampling batched and on
    device (no per-token host sync). Finished rows stop advancing, keep
    being fed their last token and their outputs are discarded.
    """
    from .sampling import sample_batch

    B = len(prompts)
    lens = [len(p) for p in prompts]
    assert B >= 1 and min(lens) >= 1, "generate_batch: every prompt needs >= 1 token"
    assert max(lens) <= model.num_ctx, "generate_batch: prompt longer than num_ctx"
    if max_new_tokens <= 0:
        return [[] for _ in prompts]
    p = next(model.parameters())
    dev = p.device
    H = model.blocks[0].attn.num_head
    D = model.blocks[0].attn.head_dim
    limits = [min(max_new_tokens, model.num_ctx - n) for n in lens]
    max_ctx = max(n + m for n, m in zip(lens, limits))
    cache_rows = min(model.num_ctx, max_ctx + GRAPH_SCRATCH_ROWS)
    use_graph = (use_graph and dev.type == "cuda"
                 and cache_rows - max(lens) >= GRAPH_SCRATCH_ROWS)
    cache = StaticKVCache(model.N, B, H, D, cache_rows, dev, p.dtype)

    idx = torch.zeros(B, max(lens), dtype=torch.long)
    seen = torch.zeros(B, model.vocab_size, dtype=torch.bool)
    for b, pr in enumerate(prompts):
        row = torch.as_tensor(list(pr), dtype=torch.long)
        idx[b, : lens[b]] = row
        seen[b, row] = True
    idx, seen = idx.to(dev), seen.to(dev)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
    limit_t = torch.tensor(limits, device=dev)

    # lengths first: prompts of one token prefill through the decode step
    cache.set_len(lens_t)
    last = model.prefill(idx, cache, lens_t, chunk=prefill_chunk)  # (B, V)

    cur = idx.new_zeros((B, 1))  # static input buffers of the decode step
    active = torch.ones(B, dtype=torch.int32, device=dev)

    def step():
        cache.advance(active)
        return model(cur, static_cache=cache)

    graph = None
    if use_graph:
        graph, logits_buf = capture_decode_step(step, cache, lens_t)

    out = torch.full((B, max_new_tokens), -1, dtype=torch.long, device=dev)
    finished = limit_t <= 0
    for g in range(max_new_tokens):
        nxt = sample_batch(last, seen, temperature, top_k, top_p,
                           repetition_penalty, sample)  # (B,)
        emit = ~finished
        if eos_token is not None:
            emit &= nxt != eos_token
        out[:, g] = torch.where(emit, nxt, -1)
        finished = ~emit | (limit_t <= g + 1)
        if g + 1 == max_new_tokens:
            break
        if (g + 1) % FINISHED_CHECK_EVERY == 0 and bool(finished.all()):
            break
        seen.scatter_(1, nxt.view(B, 1), True)
        cur.copy_(torch.where(finished.view(B, 1), cur, nxt.view(B, 1)))
        active.copy_(~finished)
        if graph is not None:
            graph.replay()
            last = logits_buf[:, -1]
        else:
            last = step()[:, -1]
    res = []
    for row in out.tolist():
        res.append(row[: row.index(-1)] if -1 in row else row)
    return res


def model_getter(
    model_size: str,
    config_path: str = "torch_compatability/model_config.yaml",
    model_checkpoint: Optional[str] = None,
) -> GPT2:
    """Build (and optionally load) an inference model from the YAML zoo
    (reference GPT2.py:448-474)."""
    configs = load_config(config_path)
    assert model_size in configs, "Invalid model size provided"
    c = configs[model_size]
    model = GPT2(
        embedding_dim=c.embedding_dim,
        vocab_size=c.vocab_size,
        num_head=c.num_head,
        num_ctx=c.num_ctx,
        N=c.N,
        alibi=bool(c.get("alibi_attn", True)),
    )
    if model_checkpoint is not None:
        sd = torch.load(model_checkpoint, map_location="cpu", weights_only=True)
        model.load_state_dict(sd)
    return model
