"""Pool <-> contiguous-cache helpers for the paged attention ops, shared by
tests/test_paged.py (CPU) and tests/test_gpu_paged.py. The references and the
checker stay those of tests/_prefill.py and tests/_parity.py: a paged case is
checked on its gathered logical cache."""

from __future__ import annotations

import torch

from . import _parity as P  # noqa: F401  (re-exported for the two test files)
from . import _prefill as PF  # noqa: F401
from ._ragged import make_prompts

R = 64
PROMPT_LENS = (5, 12, 9, 3, 62, 7, 70, 1, 130, 20)
N_NEW = (10, 10, 6, 3, 8, 1, 9, 10, 3, 5)
N_NEW_11 = 7
MIN_GAP = 0.05  # reference top-2 logit gap that makes token equality meaningful
SLOTS, NUM_PAGES = 3, 6  # 5 usable pages: the 130-token prompt alone takes 3
EOS = 372


def scenario():
    """-> (prompts, counts): the ten prompts, then the eleventh, which starts
    with the first full page of prompt 6."""
    prompts = make_prompts(PROMPT_LENS)
    return prompts + [prompts[6][:R] + prompts[0]], N_NEW + (N_NEW_11,)


def make_table(B, M, P_pages, seed, used=None):
    """(B, M) int32 table over a fixed shuffled permutation of pages
    1..P_pages-1, dealt round-robin so that the sequences' pages interleave:
    entry (b, i) is perm[i * B + b]. `used[b]` entries of row b are kept, the
    rest are 0 (None: all M)."""
    assert B * M <= P_pages - 1
    g = torch.Generator().manual_seed(seed)
    perm = (torch.randperm(P_pages - 1, generator=g) + 1).to(torch.int32)
    bt = perm[: B * M].view(M, B).t().contiguous()
    if used is not None:
        for b, u in enumerate(used):
            bt[b, u:] = 0
    return bt


def scatter(pool, bt, cache, used=None):
    """pool (P, H, R, D) <- the logical caches (B, H, M*R, D) under table bt,
    the first used[b] pages of sequence b only (None: all). In place."""
    B, M = bt.shape
    R = pool.shape[2]
    for b in range(B):
        for i in range(M if used is None else used[b]):
            pool[int(bt[b, i])] = cache[b, :, i * R:(i + 1) * R]
    return pool


def gather(pool, bt):
    """The logical caches (B, H, M*R, D) of pool under table bt (a copy)."""
    B, M = bt.shape
    _, H, R, D = pool.shape
    pages = pool[bt.long()]  # (B, M, H, R, D)
    return pages.permute(0, 2, 1, 3, 4).reshape(B, H, M * R, D)


def pages_used(rows, R):
    return [-(-int(n) // R) for n in rows]


def bits(t):
    """Bit patterns (NaN-safe equality) of a 16- or 32-bit float tensor."""
    t = t.contiguous().cpu()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def serve(model, **kw):
    """The scenario through one engine: requests 0..6 first; once request 6
    is in a slot the eleventh is submitted, then 7..9. -> (tokens per request
    in scenario order, engine, what was seen when the eleventh was admitted)."""
    prompts, counts = scenario()
    from zero_transformer_amd.models.paged import ServingEngine

    eng = ServingEngine(model, SLOTS, NUM_PAGES, R, **kw)
    ids = [eng.submit(prompts[i], counts[i]) for i in range(7)]
    out = {}
    while ids[6] not in eng.info:
        eng.step()
        out.update(eng.poll())
    id11 = eng.submit(prompts[10], counts[10])
    ids += [eng.submit(prompts[i], counts[i]) for i in (7, 8, 9)]
    seen = None
    while not eng.idle():
        eng.step()
        if seen is None and id11 in eng.info:
            info = eng.info[id11]
            page = eng.info[ids[6]]["pages"][0] if ids[6] in eng.info else None
            seen = dict(info, page6=page,
                        ref=None if page is None else eng.cache.refcount[page])
        out.update(eng.poll())
    return [out[i] for i in ids + [id11]], eng, seen  # scenario order


def assert_drained(eng):
    c = eng.cache
    assert all(r is None for r in eng.running) and all(p is None for p in c.slot_pages)
    assert not any(c.refcount)
    assert c.pages_held() == len(eng._key_of) == len(eng._lru)
    assert c.pages_free() + c.pages_held() == NUM_PAGES - 1
    assert int(c.block_table.abs().sum()) == 0 and int(c.len_t.abs().sum()) == 0
    assert int(eng.active.sum()) == 0
