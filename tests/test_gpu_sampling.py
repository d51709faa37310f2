"""The fused sampler kernel (ops/csrc/sample.hip) against the float64
definition, on the grid and with the check of tests/_sampling.py, and the
serving engine with per-request options in fp16 on the GPU."""

from __future__ import annotations

import pytest
import torch

from zero_transformer_amd import ops

from . import _paged as PG
from . import _sampling as S
from ._ragged import make_model

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16, torch.float32]
N_POOLS = len(S.VOCABS) * len(S.SCALES)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _run(pool, dtype, dev, B):
    """The whole pool through the kernel in batches of B rows."""
    toks, cuts = [], []
    for lo in range(0, pool.n, B):
        args = pool.args(dtype, list(range(lo, min(lo + B, pool.n))), dev)
        t, c = ops.sample_rows(*args)
        assert t.shape == c.shape == (args[0].shape[0],)
        assert t.dtype == torch.long and c.dtype == torch.float32 and t.device == dev
        toks.append(t)
        cuts.append(c)
    return torch.cat(toks).cpu(), torch.cat(cuts).cpu()


@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_kernel_passes_the_check_on_the_grid(dev, dtype, B):
    agree = rows = 0
    for pi in range(N_POOLS):
        pool = S.grid()[pi]
        toks, cuts = _run(pool, dtype, dev, B)
        ref_t, ref_c = S.reference_outputs(pi, dtype)
        for i, o in enumerate(S.oracles(pi, dtype)):
            try:
                o.check(toks[i], cuts[i])
            except AssertionError as e:
                raise AssertionError(f"V {pool.V} scale {pool.scale} row {i} B {B}: {e}") from e
            if o.greedy:  # exactly the reference, token and cut
                assert int(toks[i]) == int(ref_t[i]) and float(cuts[i]) == float(ref_c[i])
        agree += int((toks == ref_t).sum())
        rows += pool.n
    print(f"[sampler] {str(dtype)[6:]} B {B}: {agree}/{rows} tokens equal the float64 oracle's")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_kernel_is_deterministic_and_writes_no_input(dev, dtype):
    for V in (1000, 50257, 65536):
        pool = S.grid()[S.VOCABS.index(V) * len(S.SCALES) + 1]
        args = pool.args(dtype, list(range(16)), dev)
        before = (PG.bits(args[0]), args[1].cpu().clone())
        a = ops.sample_rows(*args)
        b = ops.sample_rows(*args)
        assert torch.equal(a[0], b[0])
        assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
        assert torch.equal(PG.bits(args[0]), before[0]) and torch.equal(args[1].cpu(), before[1])
        none = ops.sample_rows(args[0], None, *args[2:])  # seen is optional
        plain = list(args)
        plain[5] = torch.ones_like(args[5])
        want = ops.sample_rows(*plain)
        assert torch.equal(none[0], want[0]) and torch.equal(none[1], want[1])


def test_rows_are_independent(dev):
    pool = S.grid()[S.VOCABS.index(8193) * len(S.SCALES) + 2]
    whole = ops.sample_rows(*pool.args(torch.float16, None, dev))
    perm = torch.randperm(pool.n, generator=torch.Generator().manual_seed(3))
    got = ops.sample_rows(*pool.args(torch.float16, perm, dev))
    assert torch.equal(got[0].cpu(), whole[0].cpu()[perm])
    assert torch.equal(got[1].cpu(), whole[1].cpu()[perm])
    args = list(pool.args(torch.float16, [0, 5, 13], dev))
    args[0] = args[0].clone()
    args[0][0] += 1.0
    args[2] = args[2].clone()
    args[2][2] = 0.3
    t, c = ops.sample_rows(*args)
    assert int(t[1]) == int(whole[0][5]) and float(c[1]) == float(whole[1][5])


def test_misaligned_rows_and_views(dev):
    """Odd V puts every other row off the 16-byte grid; a storage offset
    moves the first one too."""
    pool = S.grid()[S.VOCABS.index(65) * len(S.SCALES) + 1]
    args = list(pool.args(torch.float16, None, dev))
    want = ops.sample_rows(*args)
    flat = torch.zeros(pool.n * pool.V + 3, dtype=torch.float16, device=dev)
    flat[3:] = args[0].reshape(-1)
    args[0] = flat[3:].view(pool.n, pool.V)
    got = ops.sample_rows(*args)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_out_of_contract_rows_stay_in_range(dev):
    V = 1000
    lg = torch.full((4, V), float("-inf"), device=dev, dtype=torch.float16)
    lg[1, 3] = float("nan")
    lg[2] = float("inf")
    lg[3] = float("nan")
    f = lambda v, dt: torch.full((4,), v, dtype=dt, device=dev)
    for T in (0.8, 0.0):
        toks, _ = ops.sample_rows(lg, None, f(T, torch.float32), f(5, torch.int32),
                                  f(0.9, torch.float32), f(1.0, torch.float32),
                                  f(1, torch.long), f(0, torch.long))
        assert bool(((toks >= 0) & (toks < V)).all())


def test_v_beyond_the_kernel_takes_the_reference(dev):
    V = ops.SAMPLE_ROWS_MAX_V + 8
    lg = (torch.randn(1, V, generator=torch.Generator().manual_seed(0)) * 3).half()
    f = lambda v, dt: torch.full((1,), v, dtype=dt)
    opts = (f(0.8, torch.float32), f(40, torch.int32), f(0.9, torch.float32),
            f(1.0, torch.float32), f(5, torch.long), f(2, torch.long))
    want = ops.sample_rows(lg, None, *opts)
    got = ops.sample_rows(lg.to(dev), None, *(o.to(dev) for o in opts))
    assert got[0].device == dev and int(got[0]) == int(want[0]) and float(got[1]) == float(want[1])


def test_graph_replay_reads_the_options_on_the_device(dev):
    pool = S.grid()[S.VOCABS.index(1000) * len(S.SCALES) + 1]
    sets = [pool.args(torch.float16, rows, dev) for rows in ([0, 1, 2], [13, 3, 17], [20, 5, 26])]
    eager = [ops.sample_rows(*a) for a in sets]
    static = [t.clone() for t in sets[0]]
    warm = torch.cuda.Stream()
    warm.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(warm):
        ops.sample_rows(*static)
    torch.cuda.current_stream().wait_stream(warm)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.sample_rows(*static)
    for a, want in zip(sets, eager):
        for dst, src in zip(static, a):
            dst.copy_(src)
        graph.replay()
        assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])


@pytest.fixture(scope="module")
def served(dev):
    """The mixed-option scenario in fp16, with and without the captured
    graph, and each request alone through greedy generate_batch."""
    from zero_transformer_amd.models.inference import generate_batch

    model = make_model(num_ctx=192).to(dev).to(torch.float16)
    prompts, counts = PG.scenario()
    alone = [generate_batch(model, [pr], n)[0] for pr, n in zip(prompts, counts)]
    replay = list(S.MIXED)
    replay[S.UNSEEDED] = dict(S.MIXED[S.UNSEEDED], seed=909)
    return alone, {g: S.serve_mixed(model, replay, use_graph=g)[0] for g in (True, False)}


def test_engine_mixed_options_graph_equals_eager(served):
    alone, runs = served
    assert runs[True] == runs[False]
    sampled = [i for i in range(len(alone)) if i not in S.GREEDY_IDS and i != S.TOP1_ID]
    assert any(runs[True][i] != alone[i] for i in sampled), "nothing was sampled"


@pytest.mark.parametrize("use_graph", [True, False])
def test_engine_greedy_requests_equal_generate_batch(served, use_graph):
    alone, runs = served
    for i in S.GREEDY_IDS + [S.TOP1_ID]:
        assert runs[use_graph][i] == alone[i]
