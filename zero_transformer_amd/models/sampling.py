"""Sampling utilities + streaming KV-cached generation
(reference app.py:42-142: repetition penalty, temperature, top-k, nucleus,
greedy, EOS stop, per-token streaming with layer_past cache)."""

from __future__ import annotations

from typing import Iterator, List, Optional

import torch
import torch.nn.functional as F


def apply_repetition_penalty(
    logits: torch.Tensor, generated: List[int], penalty: float
) -> torch.Tensor:
    """CTRL-style repetition penalty (reference app.py:97-108)."""
    if penalty == 1.0 or not generated:
        return logits
    idx = torch.tensor(sorted(set(generated)), device=logits.device)
    sel = logits[..., idx]
    sel = torch.where(sel > 0, sel / penalty, sel * penalty)
    logits[..., idx] = sel
    return logits


def apply_repetition_penalty_batched(
    logits: torch.Tensor, seen: torch.Tensor, penalty: float
) -> torch.Tensor:
    """apply_repetition_penalty for a batch, on device: logits (B, V), seen
    (B, V) bool marking each row's prompt and generated tokens (kept up to
    date with scatter_). Row b gets what apply_repetition_penalty gives it
    alone with the tokens seen[b] marks. Never writes to `logits`: returns a
    new tensor, or `logits` itself when penalty == 1.0."""
    if penalty == 1.0:
        return logits
    pen = torch.where(logits > 0, logits / penalty, logits * penalty)
    return torch.where(seen, pen, logits)


def top_k_filter(logits: torch.Tensor, k: int) -> torch.Tensor:
    """Keep the k highest logits (reference app.py:111-115)."""
    if k <= 0:
        return logits
    v, _ = torch.topk(logits, min(k, logits.size(-1)))
    return logits.masked_fill(logits < v[..., -1, None], float("-inf"))


def top_p_filter(logits: torch.Tensor, p: float) -> torch.Tensor:
    """Nucleus filtering (reference app.py:118-142)."""
    if p >= 1.0:
        return logits
    sorted_logits, sorted_idx = torch.sort(logits, descending=True)
    cum = torch.cumsum(F.softmax(sorted_logits.float(), dim=-1), dim=-1)
    remove = cum > p
    remove[..., 1:] = remove[..., :-1].clone()
    remove[..., 0] = False
    mask = remove.scatter(-1, sorted_idx, remove)
    return logits.masked_fill(mask, float("-inf"))


def _sample_next(logits, generated, temperature, top_k, top_p,
                 repetition_penalty, sample) -> int:
    lg = logits[:, -1, :].clone()
    lg = apply_repetition_penalty(lg, generated, repetition_penalty)
    lg = lg / max(temperature, 1e-5)
    if top_k:
        lg = top_k_filter(lg, top_k)
    if top_p < 1.0:
        lg = top_p_filter(lg, top_p)
    probs = F.softmax(lg.float(), dim=-1)
    return int(torch.multinomial(probs, 1).item()) if sample else int(probs.argmax().item())


def sample_batch(logits, seen, temperature, top_k, top_p,
                 repetition_penalty, sample) -> torch.Tensor:
    """_sample_next for a batch without leaving the device: logits (B, V),
    seen as in apply_repetition_penalty_batched -> (B,) int64 token ids.
    Greedy takes the argmax of the penalised logits directly (temperature
    and the filters keep the maximum where it is)."""
    lg = apply_repetition_penalty_batched(logits, seen, repetition_penalty)
    if not sample:
        return lg.argmax(-1)
    lg = lg / max(temperature, 1e-5)
    if top_k:
        lg = top_k_filter(lg, top_k)
    if top_p < 1.0:
        lg = top_p_filter(lg, top_p)
    probs = F.softmax(lg.float(), dim=-1)
    return torch.multinomial(probs, 1).squeeze(-1)


@torch.no_grad()
def generate_stream(
    model,
    idx: torch.Tensor,
    max_new_tokens: int = 128,
    temperature: float = 1.0,
    top_k: int = 0,
    top_p: float = 1.0,
    repetition_penalty: float = 1.0,
    sample: bool = True,
    eos_token: Optional[int] = None,
    use_graph: bool = True,
    prefill_chunk: Optional[int] = None,
) -> Iterator[int]:
    """Streaming generation with KV cache (reference app.py:42-94).

    On GPU the decode step runs against a static KV cache with the whole
    per-token model call captured in a hipGraph (the generate_fast
    machinery) — sampling stays host-side between replays, so every
    sampler/penalty option streams at graph-replay latency; the prompt goes
    through GPT2.prefill (in slices of `prefill_chunk` positions if set).
    CPU keeps the dynamic layer_past path.
    """
    model.eval()
    assert idx.shape[0] == 1, "generate_stream streams a single prompt (B=1); use inference.generate_batch for batched decoding"
    generated: List[int] = idx[0].tolist()
    kw = (temperature, top_k, top_p, repetition_penalty, sample)

    if idx.is_cuda:
        from .inference import (GRAPH_SCRATCH_ROWS, StaticKVCache,
                                capture_decode_step)

        B, T0 = idx.shape
        dev = idx.device
        H = model.blocks[0].attn.num_head
        D = model.blocks[0].attn.head_dim
        max_ctx = min(model.num_ctx, T0 + max_new_tokens)
        rows = min(model.num_ctx, max_ctx + GRAPH_SCRATCH_ROWS)
        use_graph = use_graph and rows - T0 >= GRAPH_SCRATCH_ROWS
        cache = StaticKVCache(model.N, B, H, D, rows, dev,
                              next(model.parameters()).dtype)
        # length first: a one-token prompt prefills through the decode
        # step, which appends at row len - 1 (T0 > 1 never reads it)
        cache.set_len(T0)
        logits = model.prefill(idx, cache, chunk=prefill_chunk).unsqueeze(1)
        cur = idx.new_zeros((B, 1))

        def step():
            cache.advance(1)
            return model(cur, static_cache=cache)

        graph = None
        if use_graph:
            graph, logits_buf = capture_decode_step(step, cache, T0)

        for i in range(max_new_tokens):
            nxt = _sample_next(logits, generated, *kw)
            if eos_token is not None and nxt == eos_token:
                return
            generated.append(nxt)
            yield nxt
            if T0 + 1 + i >= max_ctx:
                return
            cur.fill_(nxt)
            if graph is not None:
                graph.replay()
                logits = logits_buf
            else:
                logits = step()
        return

    logits, states = model(idx, use_cache=True)
    for _ in range(max_new_tokens):
        nxt = _sample_next(logits, generated, *kw)
        if eos_token is not None and nxt == eos_token:
            return
        generated.append(nxt)
        yield nxt
        cur = torch.tensor([[nxt]], device=idx.device)
        logits, states = model(cur, use_cache=True, past_states=states)
