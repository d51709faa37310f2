"""ops.sample_rows on the CPU (the float64 oracle, its RNG mirror and the
dispatch), and per-request sampling options through ServingEngine and
POST /submit. The GPU kernel is checked by tests/test_gpu_sampling.py with the
same helpers (tests/_sampling.py)."""

from __future__ import annotations

import pytest
import torch

from zero_transformer_amd import ops
from zero_transformer_amd.models.sampling import sample_batch
from zero_transformer_amd.ops import reference

from . import _sampling as S
from ._ragged import make_model

# ---------------------------------------------------------------------------
# RNG mirror
# ---------------------------------------------------------------------------


def test_uniform01_anchors():
    """Values of csrc/common.h uniform01, computed from its definition."""
    assert reference.uniform01(1234, 5) == 0.14350616931915283
    assert reference.uniform01(S.SEED_U0, 0) == 0.0
    assert reference.uniform01(S.SEED_U1, 0) == 1.0 - 2.0 ** -24
    # 64-bit words: a negative seed is its two's complement
    assert reference.uniform01(-7, 3) == reference.uniform01(2 ** 64 - 7, 3)


def test_uniform01_mean():
    n = 20000
    mean = sum(reference.uniform01(99, i) for i in range(n)) / n
    assert abs(mean - 0.5) < 0.01


# ---------------------------------------------------------------------------
# the oracle on the grid
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("pool_index", range(len(S.VOCABS) * len(S.SCALES)))
def test_reference_passes_the_check(pool_index):
    """Self-consistency of the helper and the oracle, fp16 logits."""
    toks, cuts = S.reference_outputs(pool_index, torch.float16)
    assert toks.dtype == torch.long and cuts.dtype == torch.float32
    for o, t, c in zip(S.oracles(pool_index, torch.float16), toks, cuts):
        o.check(t, c)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_cpu_dispatch_is_the_reference_and_greedy_equals_sample_batch(dtype):
    pool_index = S.VOCABS.index(1000) * len(S.SCALES) + 1
    pool = S.grid()[pool_index]
    args = pool.args(dtype)
    toks, cuts = ops.sample_rows(*args)
    want_t, want_c = reference.sample_rows(*args)
    assert torch.equal(toks, want_t) and torch.equal(cuts, want_c)
    for o, t, c in zip(S.oracles(pool_index, dtype), toks, cuts):
        o.check(t, c)
    greedy = [i for i in range(pool.n) if float(pool.temperature[i]) == 0.0]
    assert any(abs(float(pool.penalty[i]) - 1.3) < 1e-6 for i in greedy)
    for i in greedy:
        lg, seen = args[0][i:i + 1], args[1][i:i + 1]
        want = sample_batch(lg, seen, 1.0, 0, 1.0, float(pool.penalty[i]), False)
        assert int(toks[i]) == int(want)
    with pytest.raises(Exception):
        ops.sample_rows(*args[:-1])  # no counter


def test_logits_and_seen_are_not_written():
    pool = S.grid()[S.VOCABS.index(65) * len(S.SCALES)]
    args = pool.args(torch.float16)
    before = (args[0].clone(), args[1].clone())
    reference.sample_rows(*args)
    assert torch.equal(before[0].view(torch.int16), args[0].view(torch.int16))
    assert torch.equal(before[1], args[1])


def test_rows_are_independent():
    pool_index = S.VOCABS.index(1000) * len(S.SCALES) + 2
    pool = S.grid()[pool_index]
    toks, cuts = S.reference_outputs(pool_index, torch.float16)
    perm = torch.randperm(pool.n, generator=torch.Generator().manual_seed(3))
    pt, pc = reference.sample_rows(*pool.args(torch.float16, perm))
    assert torch.equal(pt, toks[perm]) and torch.equal(pc, cuts[perm])
    # a row alone, and the same row among changed neighbours
    args = list(pool.args(torch.float16, [0, 5, 13]))
    t3, c3 = reference.sample_rows(*args)
    args[0] = args[0].clone()
    args[0][0] += 1.0
    args[2] = args[2].clone()
    args[2][2] = 0.3
    t3b, c3b = reference.sample_rows(*args)
    assert int(t3b[1]) == int(t3[1]) == int(toks[5]) and float(c3b[1]) == float(cuts[5])


def test_out_of_contract_rows_stay_in_range():
    V = 70
    lg = torch.full((3, V), float("-inf"))
    lg[1, 3] = float("nan")
    lg[2] = float("inf")
    f = lambda v, dt: torch.full((3,), v, dtype=dt)
    toks, _ = reference.sample_rows(lg, None, f(0.8, torch.float32), f(5, torch.int32),
                                    f(0.9, torch.float32), f(1.0, torch.float32),
                                    f(1, torch.long), f(0, torch.long))
    assert bool(((toks >= 0) & (toks < V)).all())


# ---------------------------------------------------------------------------
# the engine: per-request options, fp32 test model on the CPU
# ---------------------------------------------------------------------------


@pytest.fixture(scope="module")
def model():
    return make_model(num_ctx=192)


@pytest.fixture(scope="module")
def default_run(model):
    """The scenario through an engine with its default (greedy) options."""
    from . import _paged as PG

    return PG.serve(model)[0]


@pytest.fixture(scope="module")
def mixed_run(model):
    torch.manual_seed(11)
    return S.serve_mixed(model)


def test_engine_greedy_requests_are_unchanged_in_a_mixed_batch(default_run, mixed_run):
    got, seeds = mixed_run
    for i in S.GREEDY_IDS:
        assert got[i] == default_run[i]
        assert seeds[i] is None  # a greedy request draws nothing
    sampled = [i for i in range(len(got)) if i not in S.GREEDY_IDS and i != S.TOP1_ID]
    assert any(got[i] != default_run[i] for i in sampled), "nothing was sampled"
    assert [len(g) for g in got] == [len(g) for g in default_run]


def test_engine_top_k_1_equals_greedy(default_run, mixed_run):
    assert mixed_run[0][S.TOP1_ID] == default_run[S.TOP1_ID]


def test_engine_is_reproducible_from_the_recorded_seeds(model, mixed_run):
    """(b) and (d): the unseeded request's recorded seed replays it, and the
    global generator has no say once every seed is given."""
    got, seeds = mixed_run
    assert isinstance(seeds[S.UNSEEDED], int)
    assert seeds[1] == 101 and seeds[10] == -7  # as a signed 64-bit word
    replay = list(S.MIXED)
    replay[S.UNSEEDED] = dict(S.MIXED[S.UNSEEDED], seed=seeds[S.UNSEEDED])
    torch.manual_seed(12345)
    again, seeds2 = S.serve_mixed(model, replay)
    assert again == got and seeds2[S.UNSEEDED] == seeds[S.UNSEEDED]
    torch.manual_seed(777)
    assert S.serve_mixed(model, replay, check_every=1, prefix_cache=False)[0] == got


def test_engine_unseeded_requests_follow_manual_seed(model):
    from zero_transformer_amd.models.paged import ServingEngine

    def seed_of(manual, **kw):
        torch.manual_seed(manual)
        eng = ServingEngine(model, 2, 4, 64)
        state = torch.get_rng_state()
        rid = eng.submit([5, 6, 7], 4, **kw)
        untouched = torch.equal(state, torch.get_rng_state())
        eng.step()
        return eng.info[rid]["seed"], untouched

    assert seed_of(1, sample=True) == seed_of(1, sample=True)
    assert seed_of(1, sample=True)[0] != seed_of(2, sample=True)[0]
    assert seed_of(1, sample=True)[1] is False
    assert seed_of(1) == (None, True)  # greedy: the global generator is untouched
    assert seed_of(1, sample=True, seed=9) == (9, True)


@pytest.mark.parametrize("bad", [dict(top_k=-1), dict(top_p=1.5), dict(top_p=-0.1),
                                 dict(repetition_penalty=0.0), dict(temperature=-1.0),
                                 dict(temperature=float("nan")),
                                 dict(temperature=float("inf"))])
def test_engine_rejects_out_of_range_options(model, bad):
    from zero_transformer_amd.models.paged import ServingEngine

    eng = ServingEngine(model, 2, 4, 64)
    with pytest.raises(ValueError):
        eng.submit([1, 2, 3], 4, **bad)
    assert eng.idle()


# ---------------------------------------------------------------------------
# the endpoint
# ---------------------------------------------------------------------------


def test_submit_endpoint_takes_the_options():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient

    from app import ByteTokenizer, build_app
    from torch_compatability.GPT2 import model_getter
    from zero_transformer_amd.models.paged import ServingEngine

    torch.manual_seed(4)
    model = model_getter("test", config_path="torch_compatability/model_config.yaml").eval()
    tok, dev = ByteTokenizer(), torch.device("cpu")
    eng = ServingEngine(model, 2, 4, 64, repetition_penalty=1.2)
    app = build_app(model, tok, dev, eng)
    client = TestClient(app)
    try:
        prompt, n = "Hello, MI355X!", 12
        want = client.post("/generate_batch", json={
            "prompts": [prompt], "max_new_tokens": n, "greedy": True}).json()["completions"][0]
        greedy = client.post("/submit", json={
            "prompt": prompt, "max_new_tokens": n, "greedy": True}).json()["completion"]
        assert greedy == want
        # The default-initialised test model echoes its last token with a
        # logit gap of about 35 to the runner-up: at temperature 1.5 alone no
        # seed can leave the greedy text. A repetition penalty of 60 brings a
        # seen token's logit below the unseen ones, so that several tokens
        # carry mass at every step; the greedy text it is compared with has
        # the same penalty.
        body = {"prompt": prompt, "max_new_tokens": n, "temperature": 1.5, "seed": 7,
                "repetition_penalty": 60.0}
        first = client.post("/submit", json=body).json()["completion"]
        second = client.post("/submit", json=body).json()["completion"]
        assert first == second
        greedy_pen = client.post("/submit", json={
            "prompt": prompt, "max_new_tokens": n, "greedy": True,
            "repetition_penalty": 60.0}).json()["completion"]
        assert first != greedy_pen and first != greedy
        other = client.post("/submit", json=dict(body, seed=8)).json()["completion"]
        assert other != first
        for bad in ({"top_p": 1.5}, {"top_k": -2}, {"temperature": -0.5},
                    {"repetition_penalty": 0}):
            r = client.post("/submit", json=dict(prompt=prompt, max_new_tokens=n, **bad))
            assert r.status_code == 400, bad
    finally:
        app.state.worker.close()
