"""Paged KV cache and a continuous-batching serving engine on top of it.

PagedKVCache replaces StaticKVCache's (B, H, S_alloc, D) buffers by a pool of
pages, (P, H, R, D) per layer, and a per-slot block table: a sequence holds
ceil(rows / R) pages wherever they are free, and two sequences with the same
prompt prefix can point at the same pages. Both attention kernels address the
pool through the table (ops.attention_prefill_paged /
ops.attention_decode_paged, ops/csrc/attn_paged.hip).

ServingEngine keeps a fixed number of slots decoding in one (optionally
hipGraph-captured) step and changes the population between steps: finished
rows are retired and their pages released, waiting requests are admitted into
the free slots and prefilled together, and full prompt pages are shared
between requests through a hash chain of their token blocks.
"""

from __future__ import annotations

import hashlib
import math
from collections import OrderedDict, deque
from typing import Dict, List, Optional, Sequence

import torch

from .. import ops
from .inference import FINISHED_CHECK_EVERY, GPT2


class _PagedAttend:
    """What the attention layers need from a paged cache: per-layer pools
    `k` / `v`, a `block_table` (B, M) and `len_t` (B,) for B sequences."""

    def attend_decode(self, layer_idx, qkv, num_head, slopes):
        return ops.attention_decode_paged(
            qkv, self.k[layer_idx], self.v[layer_idx], num_head, slopes,
            self.block_table, self.len_t)

    def attend_prefill(self, layer_idx, qkv, num_head, slopes, lens, start):
        return ops.attention_prefill_paged(
            qkv, self.k[layer_idx], self.v[layer_idx], num_head, slopes,
            self.block_table, lens, start)


class _SlotView(_PagedAttend):
    """Some slots of a PagedKVCache, for a prefill of just those: the same
    pools (they have no batch dimension) with the slots' table and length
    rows."""

    def __init__(self, cache: "PagedKVCache", slots: Sequence[int], lens):
        sel = torch.as_tensor(list(slots), dtype=torch.long, device=cache.block_table.device)
        self.k, self.v = cache.k, cache.v
        self.block_table = cache.block_table.index_select(0, sel).contiguous()
        self.len_t = torch.as_tensor(lens, dtype=torch.int32).to(sel.device)


class PagedKVCache(_PagedAttend):
    """Per-layer page pools, a device block table and length per slot, and the
    host-side page allocator.

    Page 0 is the parking page: it is never handed out and every unused table
    entry points to it, so a table entry is always a valid page id. A slot
    owns ceil(n_rows / page_rows) table entries from assign() to release().
    Pages carry a reference count (the number of slots whose table names
    them); a page whose count drops to zero goes back to the free list unless
    the caller asks to keep it (`release(slot, keep=...)`: it is then *held*,
    outside the free list with count zero, until it is shared again through
    assign(shared_pages=...) or given up with free_page()). All bookkeeping is
    host-side Python; misuse trips an assert.
    """

    def __init__(self, n_layers: int, slots: int, heads: int, head_dim: int,
                 num_pages: int, page_rows: int, max_pages_per_seq: int,
                 device, dtype):
        assert page_rows > 0 and page_rows % 64 == 0, \
            "page_rows must be a multiple of 64 (the kernels' key tile)"
        assert num_pages >= 2, "page 0 is reserved: at least 2 pages"
        assert slots >= 1 and max_pages_per_seq >= 1
        shape = (num_pages, heads, page_rows, head_dim)
        self.k = [torch.zeros(shape, device=device, dtype=dtype) for _ in range(n_layers)]
        self.v = [torch.zeros(shape, device=device, dtype=dtype) for _ in range(n_layers)]
        self.block_table = torch.zeros(slots, max_pages_per_seq, dtype=torch.int32,
                                       device=device)
        self.len_t = torch.zeros(slots, dtype=torch.int32, device=device)
        self.slots, self.num_pages = slots, num_pages
        self.page_rows, self.max_pages = page_rows, max_pages_per_seq
        self._free = deque(range(1, num_pages))
        self.refcount = [0] * num_pages
        self._held = set()
        self.slot_pages: List[Optional[List[int]]] = [None] * slots

    # ---- allocator (host) ----

    def pages_free(self) -> int:
        return len(self._free)

    def pages_for(self, n_rows: int) -> int:
        return -(-n_rows // self.page_rows)

    def kv_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.k + self.v)

    def assign(self, slot: int, n_rows: int, shared_pages: Sequence[int] = ()) -> List[int]:
        """Give the empty `slot` pages for `n_rows` rows: `shared_pages` (live
        or held pages, in order, for its first rows) plus fresh ones. Writes
        the slot's table row; returns its pages."""
        assert 0 <= slot < self.slots and self.slot_pages[slot] is None, \
            f"assign: slot {slot} is occupied"
        need = self.pages_for(n_rows)
        assert 1 <= need <= self.max_pages, \
            f"assign: {n_rows} rows exceed the per-sequence capacity"
        shared = list(shared_pages)
        assert len(shared) <= need and len(set(shared)) == len(shared)
        for p in shared:
            assert 0 < p < self.num_pages and (self.refcount[p] > 0 or p in self._held), \
                f"assign: page {p} is neither live nor held"
        assert need - len(shared) <= len(self._free), "assign: not enough free pages"
        for p in shared:
            self._held.discard(p)
            self.refcount[p] += 1
        fresh = [self._free.popleft() for _ in range(need - len(shared))]
        for p in fresh:
            assert self.refcount[p] == 0
            self.refcount[p] = 1
        pages = shared + fresh
        self.slot_pages[slot] = pages
        row = torch.zeros(self.max_pages, dtype=torch.int32)
        row[: len(pages)] = torch.tensor(pages, dtype=torch.int32)
        self.block_table[slot].copy_(row)
        return pages

    def release(self, slot: int, keep=()) -> List[int]:
        """Empty `slot`: its table row points to page 0 again, its length is 0.
        A page nobody else references goes to the free list, or, if it is in
        `keep`, becomes held; returns the pages now held."""
        assert 0 <= slot < self.slots and self.slot_pages[slot] is not None, \
            f"release: slot {slot} is empty"
        held = []
        for p in self.slot_pages[slot]:
            assert self.refcount[p] > 0, f"release: page {p} freed twice"
            self.refcount[p] -= 1
            if self.refcount[p] == 0:
                if p in keep:
                    self._held.add(p)
                    held.append(p)
                else:
                    self._free.append(p)
        self.slot_pages[slot] = None
        self.block_table[slot].zero_()
        self.len_t[slot] = 0
        return held

    def free_page(self, page: int) -> None:
        """Give a held page back to the free list."""
        assert page in self._held, f"free_page: page {page} is not held"
        self._held.remove(page)
        self._free.append(page)

    def pages_held(self) -> int:
        return len(self._held)

    # ---- lengths (device) ----

    def set_len(self, n, slots: Optional[Sequence[int]] = None):
        """An int (every slot) or one length per slot; with `slots`, for
        those only."""
        if slots is not None:
            sel = torch.as_tensor(list(slots), dtype=torch.long, device=self.len_t.device)
            self.len_t.index_copy_(
                0, sel, torch.as_tensor(n, dtype=torch.int32).to(self.len_t.device))
        elif isinstance(n, int):
            self.len_t.fill_(n)
        else:
            self.len_t.copy_(torch.as_tensor(n, dtype=torch.int32))

    def advance(self, n=1):
        """As StaticKVCache.advance: an int or a (slots,) int32 device tensor."""
        self.len_t += n

    def view(self, slots: Sequence[int], lens) -> _SlotView:
        """The cache as a prefill of `slots` sees it; `lens` are their lengths
        once it is done."""
        return _SlotView(self, slots, lens)


class _Request:
    __slots__ = ("rid", "prompt", "limit", "slot", "shared", "keys",
                 "temperature", "top_k", "top_p", "penalty", "seed")

    def __init__(self, rid, prompt, limit, temperature, top_k, top_p, penalty, seed):
        self.rid, self.prompt, self.limit = rid, prompt, limit
        self.slot, self.shared, self.keys = None, 0, None
        # temperature 0 is greedy; seed None: the request draws nothing
        self.temperature, self.top_k, self.top_p = temperature, top_k, top_p
        self.penalty, self.seed = penalty, seed


class ServingEngine:
    """Continuous batching over a PagedKVCache: `slots` sequences decode in one
    step, and between steps finished ones leave and waiting ones enter.

        eng = ServingEngine(model, slots=16, num_pages=256)
        a = eng.submit(tokens, 64); b = eng.submit(other, 200)
        results = eng.run()          # {a: [...], b: [...]}

    submit() queues a request and returns its id. step() (1) retires finished
    rows and releases their pages, (2) admits waiting requests into free
    slots, first come first served, and prefills them together in one
    right-padded GPT2.prefill, (3) runs one decode step for all slots. run()
    steps until nothing is queued or running; poll() hands out what has
    finished since the last poll. A request yields at most
    min(max_new_tokens, num_ctx - len(prompt)) tokens, cut before `eos_token`
    - generate_batch's rule.

    Sampling options are per request: submit() takes sample, temperature,
    top_k, top_p, repetition_penalty and seed, and None means the
    constructor's value. They live in per-slot device tensors written at
    admission, and one ops.sample_rows call per step reads them per row.
    Token i of a request is drawn with u = uniform01(seed, i), whoever shares
    the batch, whichever slot it has and however many steps ran before: the
    same prompt, options and seed give the same completion. A sampling
    request without a seed gets one from torch's default CPU generator at
    submit() (a greedy one draws nothing); info[rid]["seed"] holds the seed
    in use. Tokens tied with the nucleus cut are all kept.

    Admission is all-or-nothing: a request enters only when every page it can
    ever need, ceil((len + limit) / page_rows) minus the shared ones, is free
    (evictable prefix pages count as free), and gets them all at once, so its
    table row is written once and it cannot run out of pages in flight.
    Preemption and recompute are out of scope: a request that is admitted
    runs to its end, and the queue is strictly first in, first out (a large
    request at its head holds back smaller ones behind it).

    The decode step is captured once, at construction, with every length 0
    and nothing active: such a step writes nothing. Population changes are
    in-place device writes (block table, lengths, `cur`, `active`, `seen`,
    the sampling options)
    between replays. A slot with active = 0 (finished or empty) has length 0
    in the step, so it neither reads nor writes the pool. The host asks the
    device which rows have finished once per `check_every` steps, and when a
    running request is known to have reached its limit; results do not depend
    on it.

    Prefix reuse (`prefix_cache`): every full page of a prompt is keyed by the
    hash chain of its token blocks (page i covers tokens [0, (i + 1) R)). On
    admission the longest cached chain is shared, at most (len - 1) // R
    pages so that one row at least is prefilled, and only those rows' tokens
    go through the prefill, with start = the shared rows. Pages are keyed
    once their prefill is queued, so a request shares with earlier admission
    rounds only: one whose next page is being filled by a request of the
    same round waits one step (and the queue behind it) and shares it then.
    Decode appends never land in a shared page
    (only full prompt pages are shared). Keyed pages of retired requests stay
    cached until free pages run short, then go least recently used first.
    """

    @torch.no_grad()
    def __init__(self, model: GPT2, slots: int, num_pages: int, page_rows: int = 64, *,
                 eos_token: Optional[int] = None, sample: bool = False,
                 temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                 repetition_penalty: float = 1.0, use_graph: bool = True,
                 prefill_chunk: Optional[int] = None,
                 check_every: int = FINISHED_CHECK_EVERY, prefix_cache: bool = True):
        p = next(model.parameters())
        dev = p.device
        attn = model.blocks[0].attn
        self.model, self.dev = model, dev
        self.cache = PagedKVCache(model.N, slots, attn.num_head, attn.head_dim,
                                  num_pages, page_rows, -(-model.num_ctx // page_rows),
                                  dev, p.dtype)
        self.eos_token = eos_token
        self.sampling = (temperature, top_k, top_p, repetition_penalty, sample)
        self._check_options(temperature, top_k, top_p, repetition_penalty)
        self.prefill_chunk = prefill_chunk
        self.check_every = max(1, int(check_every))
        self.prefix_cache = prefix_cache

        V = model.vocab_size
        self.cur = torch.zeros(slots, 1, dtype=torch.long, device=dev)
        self.active = torch.zeros(slots, dtype=torch.int32, device=dev)
        self.seen = torch.zeros(slots, V, dtype=torch.bool, device=dev)
        self.n_gen = torch.zeros(slots, dtype=torch.long, device=dev)
        self.limit_t = torch.zeros(slots, dtype=torch.long, device=dev)
        # per-slot sampling options (empty slots are greedy: their token is discarded)
        self.temp_t = torch.zeros(slots, dtype=torch.float32, device=dev)
        self.top_k_t = torch.zeros(slots, dtype=torch.int32, device=dev)
        self.top_p_t = torch.ones(slots, dtype=torch.float32, device=dev)
        self.pen_t = torch.ones(slots, dtype=torch.float32, device=dev)
        self.seed_t = torch.zeros(slots, dtype=torch.long, device=dev)
        self.out_buf = torch.zeros(slots, model.num_ctx, dtype=torch.long, device=dev)
        self._rows = torch.arange(slots, device=dev)

        self.waiting: deque = deque()
        self.running: List[Optional[_Request]] = [None] * slots
        self.done: Dict[int, List[int]] = {}
        self.info: Dict[int, dict] = {}  # per request: slot, pages, shared rows
        self._next_id = 0
        self._steps = 0          # decode steps since the last finished check
        self._budget: List[int] = [0] * slots  # steps left until a row's limit
        self.decode_steps = 0
        self.prefill_calls = 0
        # prefix cache: chain key -> page, page -> key, held pages in LRU order
        self._page_of: Dict[bytes, int] = {}
        self._key_of: Dict[int, bytes] = {}
        self._lru: "OrderedDict[int, None]" = OrderedDict()

        self.graph = None
        if use_graph and dev.type == "cuda":
            # all lengths 0, nothing active: the warm-up and the capture write
            # nothing to the pool, so there is nothing to rewind
            warm = torch.cuda.Stream()
            warm.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(warm):
                for _ in range(2):
                    self._decode()
            torch.cuda.current_stream().wait_stream(warm)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self._logits_buf = self._decode()
        self.last = torch.zeros(slots, V, dtype=p.dtype, device=dev)

    # ---- requests ----

    @staticmethod
    def _check_options(temperature, top_k, top_p, penalty) -> None:
        if not (math.isfinite(temperature) and temperature >= 0):
            raise ValueError(f"temperature {temperature}: need a finite value >= 0")
        if top_k < 0:
            raise ValueError(f"top_k {top_k}: need >= 0 (0 turns it off)")
        if not 0 <= top_p <= 1:
            raise ValueError(f"top_p {top_p}: need 0..1")
        if not (math.isfinite(penalty) and penalty > 0):
            raise ValueError(f"repetition_penalty {penalty}: need a finite value > 0")

    def submit(self, prompt_tokens: Sequence[int], max_new_tokens: int, *,
               sample: Optional[bool] = None, temperature: Optional[float] = None,
               top_k: Optional[int] = None, top_p: Optional[float] = None,
               repetition_penalty: Optional[float] = None,
               seed: Optional[int] = None) -> int:
        """Queue a request; None takes the constructor's value of an option.
        Out-of-range options are a ValueError, like a request that can never
        fit. `seed`: any integer (used modulo 2**64)."""
        d_temp, d_k, d_p, d_pen, d_sample = self.sampling
        temperature = float(d_temp if temperature is None else temperature)
        top_k = int(d_k if top_k is None else top_k)
        top_p = float(d_p if top_p is None else top_p)
        penalty = float(d_pen if repetition_penalty is None else repetition_penalty)
        self._check_options(temperature, top_k, top_p, penalty)
        if not (d_sample if sample is None else sample):
            temperature = 0.0
        prompt = [int(t) for t in prompt_tokens]
        n = len(prompt)
        if not 1 <= n <= self.model.num_ctx:
            raise ValueError(f"prompt of {n} tokens: need 1..{self.model.num_ctx}")
        limit = min(int(max_new_tokens), self.model.num_ctx - n)
        c = self.cache
        if limit > 0 and c.pages_for(n + limit) > min(c.max_pages, c.num_pages - 1):
            raise ValueError(
                f"request needs {c.pages_for(n + limit)} pages of {c.page_rows} rows; "
                f"the pool has {c.num_pages - 1}")
        if seed is not None:
            seed = (int(seed) + 2 ** 63) % 2 ** 64 - 2 ** 63  # as a signed 64-bit word
        elif temperature > 0 and limit > 0:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        rid = self._next_id
        self._next_id += 1
        if limit <= 0:
            self.done[rid] = []
        else:
            self.waiting.append(_Request(rid, prompt, limit, temperature,
                                         min(top_k, 2 ** 31 - 1), top_p, penalty, seed))
        return rid

    def idle(self) -> bool:
        return not self.waiting and all(r is None for r in self.running)

    def poll(self) -> Dict[int, List[int]]:
        out, self.done = self.done, {}
        for rid in out:
            self.info.pop(rid, None)
        return out

    def run(self) -> Dict[int, List[int]]:
        out = self.poll()
        while not self.idle():
            self.step()
            out.update(self.poll())
        return out

    # ---- one step ----

    @torch.no_grad()
    def step(self) -> None:
        self._retire()
        self._admit()
        if any(r is not None for r in self.running):
            self._sample_and_decode()

    def _retire(self) -> None:
        occupied = [s for s, r in enumerate(self.running) if r is not None]
        if not occupied:
            return
        due = self._steps >= self.check_every or any(self._budget[s] <= 0 for s in occupied)
        if not due:
            return
        self._steps = 0
        state = torch.stack([self.active.long(), self.n_gen]).tolist()  # one sync
        gone = [s for s in occupied if state[0][s] == 0]
        if not gone:
            return
        toks = self.out_buf[gone].tolist()
        for s, row in zip(gone, toks):
            req = self.running[s]
            self.done[req.rid] = row[: state[1][s]]
            held = self.cache.release(s, keep=self._key_of)
            for p in reversed(held):  # deepest page of a chain goes first
                self._lru[p] = None
            self.running[s] = None

    def _chain_keys(self, prompt: List[int]) -> List[bytes]:
        R = self.cache.page_rows
        keys, h = [], b""
        for i in range(len(prompt) // R):
            blk = ",".join(map(str, prompt[i * R:(i + 1) * R])).encode()
            h = hashlib.sha256(h + blk).digest()
            keys.append(h)
        return keys

    def _evict(self, n: int, spare) -> None:
        """Free `n` held prefix pages, least recently used first, but none of
        `spare` (the pages the request being admitted is about to share)."""
        for p in [p for p in self._lru if p not in spare][:n]:
            del self._lru[p]
            del self._page_of[self._key_of.pop(p)]
            self.cache.free_page(p)

    def _admit(self) -> None:
        c = self.cache
        R = c.page_rows
        batch: List[_Request] = []
        free_slots = [s for s, r in enumerate(self.running) if r is None]
        fresh_keys = set()  # pages this round's prefill is about to fill
        while self.waiting and free_slots:
            req = self.waiting[0]
            n = len(req.prompt)
            shared: List[int] = []
            if req.keys is None:  # once, however long the request waits
                req.keys = self._chain_keys(req.prompt) if self.prefix_cache else []
            for key in req.keys[: (n - 1) // R]:
                if key not in self._page_of:
                    break
                shared.append(self._page_of[key])
            nxt = req.keys[len(shared):(n - 1) // R]
            if nxt and nxt[0] in fresh_keys:
                break  # its prefix is being prefilled: share it next round
            need = c.pages_for(n + req.limit) - len(shared)
            evictable = sum(1 for p in self._lru if p not in shared)
            if need > c.pages_free() + evictable:
                break  # first in, first out: nobody overtakes
            if need > c.pages_free():
                self._evict(need - c.pages_free(), set(shared))
            self.waiting.popleft()
            for p in shared:
                self._lru.pop(p, None)
            req.slot = free_slots.pop(0)
            req.shared = len(shared)
            pages = c.assign(req.slot, n + req.limit, shared)
            self.running[req.slot] = req
            self.info[req.rid] = dict(slot=req.slot, pages=pages, seed=req.seed,
                                      shared_pages=len(shared), start=len(shared) * R)
            batch.append(req)
            fresh_keys.update(k for k in req.keys if k not in self._page_of)
        if batch:
            self._prefill(batch)

    def _prefill(self, batch: List[_Request]) -> None:
        c, dev, R = self.cache, self.dev, self.cache.page_rows
        slots = [r.slot for r in batch]
        start = [r.shared * R for r in batch]
        total = [len(r.prompt) for r in batch]
        new = [n - st for n, st in zip(total, start)]
        idx = torch.zeros(len(batch), max(new), dtype=torch.long)
        seen = torch.zeros(len(batch), self.model.vocab_size, dtype=torch.bool)
        for b, r in enumerate(batch):
            idx[b, : new[b]] = torch.tensor(r.prompt[start[b]:], dtype=torch.long)
            seen[b, torch.tensor(r.prompt, dtype=torch.long)] = True
        sel = torch.tensor(slots, dtype=torch.long, device=dev)
        c.set_len(total, slots)
        last = self.model.prefill(idx.to(dev), c.view(slots, total), new,
                                  chunk=self.prefill_chunk, start=start)
        self.prefill_calls += 1
        self.last.index_copy_(0, sel, last.to(self.last.dtype))
        self.seen.index_copy_(0, sel, seen.to(dev))
        self.active.index_fill_(0, sel, 1)
        self.n_gen.index_fill_(0, sel, 0)
        self.cur.index_fill_(0, sel, 0)
        self.limit_t.index_copy_(0, sel, torch.tensor([r.limit for r in batch], device=dev))
        for dst, vals in ((self.temp_t, [r.temperature for r in batch]),
                          (self.top_k_t, [r.top_k for r in batch]),
                          (self.top_p_t, [r.top_p for r in batch]),
                          (self.pen_t, [r.penalty for r in batch]),
                          (self.seed_t, [r.seed or 0 for r in batch])):
            dst.index_copy_(0, sel, torch.tensor(vals, dtype=dst.dtype).to(dev))
        for r in batch:
            self._budget[r.slot] = r.limit
            # the prompt's full pages are valid for whoever is admitted later
            for key, page in zip(r.keys, self.info[r.rid]["pages"]):
                if key not in self._page_of:
                    self._page_of[key] = page
                    self._key_of[page] = key

    def _decode(self) -> torch.Tensor:
        """The captured part: active rows grow by one, the others drop to
        length 0 (they then neither read nor write the pool), one model step
        -> (slots, 1, V)."""
        self.cache.advance(self.active)
        self.cache.len_t.mul_(self.active)
        return self.model(self.cur, static_cache=self.cache)

    def _sample_and_decode(self) -> None:
        # token i of a request is drawn with u(seed, i): the counter is n_gen
        nxt, _ = ops.sample_rows(self.last, self.seen, self.temp_t, self.top_k_t,
                                 self.top_p_t, self.pen_t, self.seed_t, self.n_gen)
        emit = self.active.bool()
        if self.eos_token is not None:
            emit &= nxt != self.eos_token
        pos = self.n_gen.clamp(max=self.out_buf.shape[1] - 1).view(-1, 1)
        self.out_buf.scatter_(
            1, pos, torch.where(emit.view(-1, 1), nxt.view(-1, 1), self.out_buf.gather(1, pos)))
        self.n_gen += emit
        alive = emit & (self.n_gen < self.limit_t)
        self.seen.scatter_(1, nxt.view(-1, 1), True)
        self.cur.copy_(torch.where(alive.view(-1, 1), nxt.view(-1, 1), self.cur))
        self.active.copy_(alive)
        if self.graph is not None:
            self.graph.replay()
            logits = self._logits_buf
        else:
            logits = self._decode()
        self.last = logits[:, -1]
        self._steps += 1
        self.decode_steps += 1
        for s, r in enumerate(self.running):
            if r is not None:
                self._budget[s] -= 1
