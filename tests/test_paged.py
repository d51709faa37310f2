"""Paged KV cache on CPU: the page allocator, the fp32 reference ops against
the contiguous references, the serving engine against generate_batch, and the
/submit endpoint.

ops.attention_prefill_paged / attention_decode_paged route CPU tensors to the
references, so the engine here is the Python the GPU runs with the reference
ops in the kernels' place."""

from __future__ import annotations

import math
import threading

import pytest
import torch

from zero_transformer_amd import ops
from zero_transformer_amd.models.inference import generate_batch
from zero_transformer_amd.models.paged import PagedKVCache, ServingEngine
from zero_transformer_amd.ops import reference

from . import _paged as PG
from . import _parity as P
from . import _prefill as PF
from ._paged import (EOS, MIN_GAP, NUM_PAGES, R, assert_drained, scenario, serve)
from ._ragged import make_model

# ---------------------------------------------------------------------------
# allocator
# ---------------------------------------------------------------------------


def _cache(slots=3, pages=8, M=3):
    return PagedKVCache(1, slots, 2, 8, pages, R, M, "cpu", torch.float32)


def _accounted(c):
    live = sum(1 for n in c.refcount if n > 0)
    return c.pages_free() + c.pages_held() + live


def test_allocator_conserves_pages_and_counts_sharers():
    c = _cache()
    assert c.pages_free() == 7 and c.refcount[0] == 0
    a = c.assign(0, 130)  # 3 pages
    assert len(a) == 3 and 0 not in a and c.pages_free() == 4
    assert c.block_table[0].tolist() == a
    b = c.assign(1, 70, shared_pages=a[:1])  # 2 pages, the first one shared
    assert b[0] == a[0] and c.refcount[a[0]] == 2 and c.pages_free() == 3
    assert c.block_table[1].tolist() == b + [0]
    assert _accounted(c) == 7
    # the shared page survives its first owner; the others come back
    assert c.release(0) == [] and c.refcount[a[0]] == 1 and c.pages_free() == 5
    assert c.block_table[0].tolist() == [0, 0, 0] and int(c.len_t[0]) == 0
    # the last sharer leaves: kept pages are held, not free
    held = c.release(1, keep={a[0]})
    assert held == [a[0]] and c.pages_held() == 1 and c.pages_free() == 6
    assert _accounted(c) == 7
    # a held page can be shared again, or given up
    d = c.assign(2, 64 + 1, shared_pages=held)
    assert d[0] == a[0] and c.pages_held() == 0 and c.refcount[a[0]] == 1
    c.release(2, keep={a[0]})
    c.free_page(a[0])
    assert c.pages_free() == 7 and c.pages_held() == 0 and not any(c.refcount)
    # any order of assign / release conserves the count
    g = torch.Generator().manual_seed(3)
    for _ in range(50):
        s = int(torch.randint(0, 3, (1,), generator=g))
        if c.slot_pages[s] is None:
            rows = int(torch.randint(1, 3 * R + 1, (1,), generator=g))
            if c.pages_for(rows) <= c.pages_free():
                c.assign(s, rows)
        else:
            c.release(s)
        assert _accounted(c) == 7
    assert c.len_t.dtype == torch.int32 and c.block_table.dtype == torch.int32


def test_allocator_asserts_on_misuse():
    c = _cache()
    with pytest.raises(AssertionError):
        c.release(0)  # empty slot
    c.assign(0, 10)
    with pytest.raises(AssertionError):
        c.assign(0, 10)  # occupied
    with pytest.raises(AssertionError):
        c.assign(1, 3 * R + 1)  # over the per-sequence capacity
    with pytest.raises(AssertionError):
        c.assign(1, 10, shared_pages=[5])  # page 5 is free: neither live nor held
    c.release(0)
    with pytest.raises(AssertionError):
        c.release(0)  # double free
    with pytest.raises(AssertionError):
        c.free_page(1)  # not held
    small = _cache(pages=3)
    small.assign(0, 2 * R)
    with pytest.raises(AssertionError):
        small.assign(1, 1)  # no free page left
    with pytest.raises(AssertionError):
        PagedKVCache(1, 1, 2, 8, 4, 48, 2, "cpu", torch.float32)  # R % 64


def test_cache_lengths():
    c = _cache()
    c.set_len([5, 70], slots=[2, 0])
    assert c.len_t.tolist() == [70, 0, 5]
    c.advance(torch.tensor([1, 1, 0], dtype=torch.int32))
    assert c.len_t.tolist() == [71, 1, 5]
    c.set_len(0)
    assert c.len_t.tolist() == [0, 0, 0]


# ---------------------------------------------------------------------------
# reference ops against the contiguous references on the gathered caches
# ---------------------------------------------------------------------------

B, H, D, M, PAGES = 3, 2, 16, 5, 20
PREFILL_CASES = (
    ((200, 1, 65), (0, 0, 0)),
    ((0, 128, 100), (0, 0, 37)),
    ((1, 64, 1), (64, 64, 319)),
    ((205, 9, -3), (0, 318, 7)),  # clamps: lens > T, start + lens > M*R, negative
)


def _pools(seed, bt, k0, v0):
    kp = P.randn((PAGES, H, R, D), P.FP32, seed)
    vp = P.randn((PAGES, H, R, D), P.FP32, seed + 1)
    kp[0] = vp[0] = math.nan
    return PG.scatter(kp, bt, k0), PG.scatter(vp, bt, v0)


@pytest.mark.parametrize("alibi", [True, False])
def test_reference_prefill_paged_equals_contiguous_reference(alibi):
    T = 200
    C = H * D
    slopes = reference.alibi_slopes(H) if alibi else None
    bt = PG.make_table(B, M, PAGES, 5)
    for i, (lens, start) in enumerate(PREFILL_CASES):
        qkv = P.randn((B, T, 3 * C), P.FP32, 40 + i)
        k0 = P.randn((B, H, M * R, D), P.FP32, 50 + i)
        v0 = P.randn((B, H, M * R, D), P.FP32, 60 + i)
        kp, vp = _pools(70 + i, bt, k0, v0)
        kp0, vp0 = kp.clone(), vp.clone()
        lt = torch.tensor(lens, dtype=torch.int32)
        st = torch.tensor(start, dtype=torch.int32)
        want = reference.attention_prefill_append(qkv, k0, v0, H, slopes, lt, st)
        got = ops.attention_prefill_paged(qkv, kp, vp, H, slopes, bt, lt, st)
        assert torch.equal(got, want)
        # the logical caches are the contiguous ones; every page outside the
        # table (page 0 included) is untouched
        assert torch.equal(PG.gather(kp, bt), k0) and torch.equal(PG.gather(vp, bt), v0)
        out = torch.ones(PAGES, dtype=torch.bool)
        out[bt.long().flatten()] = False
        assert torch.equal(PG.bits(kp[out]), PG.bits(kp0[out]))
        assert torch.equal(PG.bits(vp[out]), PG.bits(vp0[out]))
    # lens / start None: every row new, nothing cached
    qkv = P.randn((B, T, 3 * C), P.FP32, 90)
    k0 = torch.zeros(B, H, M * R, D)
    v0 = torch.zeros(B, H, M * R, D)
    kp, vp = _pools(91, bt, k0, v0)
    want = reference.attention_prefill_append(qkv, k0, v0, H, slopes)
    assert torch.equal(ops.attention_prefill_paged(qkv, kp, vp, H, slopes, bt), want)
    assert torch.equal(PG.gather(kp, bt), k0)


@pytest.mark.parametrize("alibi", [True, False])
def test_reference_decode_paged_equals_contiguous_reference(alibi):
    Bn = 6
    lens = (0, 1, 5, 64, 65, 200)
    C = H * D
    Mn = 4
    slopes = reference.alibi_slopes(H) if alibi else None
    bt = PG.make_table(Bn, Mn, 30, 6, used=PG.pages_used(lens, R))
    qkv = P.randn((Bn, 1, 3 * C), P.FP32, 100)
    k0 = P.randn((Bn, H, Mn * R, D), P.FP32, 101)
    v0 = P.randn((Bn, H, Mn * R, D), P.FP32, 102)
    kp = torch.full((30, H, R, D), math.nan)
    vp = torch.full((30, H, R, D), math.nan)
    used = PG.pages_used(lens, R)
    PG.scatter(kp, bt, k0, used)
    PG.scatter(vp, bt, v0, used)
    kp0 = kp.clone()
    lt = torch.tensor(lens, dtype=torch.int32)
    want = reference.attention_decode_append(qkv, k0, v0, H, slopes, lt)
    got = ops.attention_decode_paged(qkv, kp, vp, H, slopes, bt, lt)
    assert torch.equal(got, want) and torch.count_nonzero(got[0]) == 0
    for b, n in enumerate(lens):
        for i in range(used[b]):
            page = int(bt[b, i])
            assert torch.equal(kp[page], k0[b, :, i * R:(i + 1) * R])
            assert torch.equal(vp[page], v0[b, :, i * R:(i + 1) * R])
    # exactly one row per live sequence changed; page 0 stayed NaN
    changed = (PG.bits(kp) != PG.bits(kp0)).any(-1).any(1)  # (P, R)
    assert int(changed.sum()) == sum(1 for n in lens if n)
    assert bool(kp[0].isnan().all())


# ---------------------------------------------------------------------------
# engine against generate_batch
# ---------------------------------------------------------------------------


@pytest.fixture(scope="module")
def model():
    return make_model(num_ctx=192)


@pytest.fixture(scope="module")
def alone(model):
    """Each request alone through generate_batch (greedy), with the top-2
    logit gap of the no-cache forward asserted at every deciding step."""
    prompts, counts = scenario()
    refs = []
    with torch.no_grad():
        for pr, n in zip(prompts, counts):
            toks = generate_batch(model, [pr], n)[0]
            assert len(toks) == n
            full = torch.tensor([pr + toks])
            logits = model(full[:, :-1])[0, len(pr) - 1:]
            top2 = logits.float().topk(2, dim=-1).values
            gap = float((top2[:, 0] - top2[:, 1]).min())
            print(f"[paged] prompt len {len(pr)}: min top-2 gap {gap:.4f}")
            assert gap >= MIN_GAP, f"top-2 gap {gap} under {MIN_GAP}"
            assert logits.argmax(-1).tolist() == toks
            refs.append(toks)
    return refs


def test_engine_equals_generate_batch_and_shares_one_page(model, alone):
    got, eng, seen = serve(model)
    assert got == alone
    assert eng.prefill_calls > 1 and eng.waiting == type(eng.waiting)()
    # the eleventh request shared exactly the first page of request 6, which
    # was still running, and prefilled only the rows behind it
    assert seen is not None and seen["shared_pages"] == 1 and seen["start"] == R
    assert seen["pages"][0] == seen["page6"] and seen["ref"] == 2
    assert_drained(eng)
    assert eng.cache.pages_held() >= 1  # prefix pages stay cached


@pytest.mark.parametrize("kw", [dict(check_every=1), dict(check_every=16, prefix_cache=False),
                                dict(check_every=1, prefill_chunk=48)], ids=str)
def test_engine_result_is_independent_of_check_interval_and_prefix_cache(model, alone, kw):
    """The default run above has check_every=16 and the prefix cache on."""
    got, eng, seen = serve(model, **kw)
    assert got == alone
    if kw.get("prefix_cache") is False:
        assert seen["shared_pages"] == 0 and seen["start"] == 0
        assert eng.cache.pages_held() == 0
    else:
        assert seen["shared_pages"] == 1 and seen["ref"] == 2
    assert_drained(eng)


def test_engine_eos(model, alone):
    assert alone[0][3] == EOS and EOS not in alone[0][:3] and alone[5][0] == EOS, \
        "scenario: eos must be prompt 0's fourth token and prompt 5's first"
    got, eng, _ = serve(model, eos_token=EOS)
    assert got[0] == alone[0][:3] and got[5] == []
    for g, ref in zip(got, alone):
        assert g == (ref[: ref.index(EOS)] if EOS in ref else ref)
    assert_drained(eng)


def test_engine_submit_limits(model):
    eng = ServingEngine(model, 2, 3, R)  # 2 usable pages
    with pytest.raises(ValueError):
        eng.submit([], 4)
    with pytest.raises(ValueError):
        eng.submit([1] * 193, 4)
    with pytest.raises(ValueError):
        eng.submit([1] * 100, 60)  # 160 rows: 3 pages, the pool has 2
    rid = eng.submit([1] * 192, 5)  # no room for a token: done at once
    assert eng.poll() == {rid: []} and eng.idle()
    with pytest.raises(ValueError):
        eng.submit([9], 200)  # capped to 191 tokens: 192 rows, 3 pages
    a = eng.submit([7] * 100, 4)  # 2 pages: fills the pool
    b = eng.submit([9], 3)  # waits for a's pages although a slot is free
    eng.step()
    assert len(eng.waiting) == 1 and eng.cache.pages_free() == 0
    res = eng.run()
    assert len(res[a]) == 4 and len(res[b]) == 3 and eng.idle()


# ---------------------------------------------------------------------------
# app
# ---------------------------------------------------------------------------


@pytest.mark.filterwarnings("ignore::pytest.PytestUnhandledThreadExceptionWarning")
def test_engine_worker_hands_a_failure_to_every_caller():
    """If the engine raises, the worker thread ends: the callers that wait,
    and any later one, get the error and do not hang."""
    from app import EngineWorker

    class Broken:
        def __init__(self):
            self.n = 0

        def submit(self, tokens, n):
            self.n += 1
            return self.n

        def idle(self):
            return self.n == 0

        def step(self):
            raise FloatingPointError("boom")

        def poll(self):
            return {}

    worker = EngineWorker(Broken())
    errors = []

    def ask():
        try:
            worker.submit([1, 2], 3)
        except RuntimeError as e:
            errors.append(str(e))

    threads = [threading.Thread(target=ask) for _ in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=30)
    assert not any(t.is_alive() for t in threads)
    ask()  # after the thread has died
    assert len(errors) == 3 and all("boom" in e for e in errors)
    worker.thread.join(timeout=30)
    assert not worker.thread.is_alive()


def test_submit_endpoint_joins_the_running_batch():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient

    from app import ByteTokenizer, build_app
    from torch_compatability.GPT2 import model_getter

    torch.manual_seed(4)
    model = model_getter("test", config_path="torch_compatability/model_config.yaml").eval()
    tok, dev = ByteTokenizer(), torch.device("cpu")
    eng = ServingEngine(model, 2, 4, R, repetition_penalty=1.2)
    app = build_app(model, tok, dev, eng)
    client = TestClient(app)
    prompts = ["Hi", "Hello, MI355X!"]
    want = client.post("/generate_batch", json={
        "prompts": prompts, "max_new_tokens": 5, "greedy": True,
        "repetition_penalty": 1.2}).json()["completions"]
    got = [None, None]

    def ask(i):
        r = client.post("/submit", json={"prompt": prompts[i], "max_new_tokens": 5})
        got[i] = r.json()["completion"]

    threads = [threading.Thread(target=ask, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert got == want
    assert client.post("/submit", json={"prompt": "x" * 40, "max_new_tokens": 5}
                       ).status_code == 400
    app.state.worker.close()
