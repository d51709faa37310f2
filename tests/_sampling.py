"""The validity check, the case grid and the mixed-option serving scenario
shared by tests/test_sampling_rows.py (CPU) and tests/test_gpu_sampling.py.

The check is against the float64 definition of ops.sample_rows and tolerates
rounding at the two places where a decision depends on a floating sum, the
top-p mass and the inclusive CDF of the draw, by TAU on the normalised mass;
everything that only compares values (top-k, greedy, membership) is exact.

TAU: fp32 rounding of the exponent argument a = (y - max) / T is a relative
error of 2^-24 |a| on each weight, and a weight that contributes more than
TAU has |a| below about 11; the fixed-order tree sums add a few 2^-24. 2e-5
is roughly ten times that.
"""

from __future__ import annotations

import torch

from zero_transformer_amd.models.sampling import apply_repetition_penalty_batched
from zero_transformer_amd.ops import reference

from . import _paged as PG

TAU = 2e-5
NEG_INF = float("-inf")

VOCABS = (1, 2, 63, 64, 65, 1000, 8193, 50257, 50304, 65536)
SCALES = (1, 3, 6)
SEED_U0 = 1612200     # uniform01(SEED_U0, 0) == 0: the first kept token
SEED_U1 = 17974134    # uniform01(SEED_U1, 0) == 1 - 2^-24: the last kept token


def combos(V):
    """13 (T, k, p) combinations in which every T of (1.0, 0.8, 0.7, 1.2),
    every k of (0, 1, 5, 40, V, V + 7) and every p of (1.0, 0.99, 0.95, 0.9,
    0.5, 0.3, 0.0) occurs."""
    return [(1.0, 0, 1.0), (0.8, 0, 0.95), (0.7, 40, 0.9), (1.2, 5, 0.5),
            (1.0, 1, 0.99), (0.8, V, 0.3), (0.7, V + 7, 0.0), (1.2, 0, 0.0),
            (1.0, 40, 1.0), (0.8, 5, 0.99), (0.7, 0, 0.5), (1.2, 40, 0.3),
            (1.0, 5, 0.9)]


class Pool:
    """The rows of one (V, scale): logits (N, V) fp16-representable fp32, seen
    (N, V) bool, and the per-row option vectors, all on the CPU."""

    def __init__(self, V, scale, gen):
        rows = []  # (logits row, seen row, T, k, p, penalty, seed, counter)

        def normal():
            return (torch.randn(V, generator=gen) * scale).half().float()

        def seed():
            return int(torch.randint(0, 2 ** 40, (1,), generator=gen))

        none = torch.zeros(V, dtype=torch.bool)
        for i, (T, k, p) in enumerate(combos(V)):
            rows.append((normal(), none, T, k, p, 1.0, seed(), i))
        seen = torch.rand(V, generator=gen) < 0.3
        rows.append((normal(), seen, 0.8, 0, 0.95, 1.3, seed(), 3))   # penalty
        rows.append((normal(), seen, 0.0, 0, 1.0, 1.3, seed(), 0))    # greedy under a penalty
        rows.append((normal(), none, 0.0, 5, 0.5, 1.0, seed(), 1))    # T = 0
        rows.append((normal(), none, 1e-6, 0, 0.9, 1.0, seed(), 2))   # T below the clamp
        quant = lambda: torch.round(torch.randn(V, generator=gen) * scale * 2) / 2
        rows.append((quant(), none, 1.0, 5, 0.9, 1.0, seed(), 4))     # ties on kth and cut
        rows.append((quant(), none, 0.8, 40, 0.5, 1.0, seed(), 5))
        rows.append((quant(), seen, 0.0, 0, 1.0, 1.0, seed(), 6))     # greedy among ties
        rows.append((torch.full((V,), 1.5), none, 1.0, 3, 0.5, 1.0, seed(), 7))  # all equal
        holes = normal()
        holes[torch.rand(V, generator=gen) < 0.5] = NEG_INF
        holes[int(torch.randint(0, V, (1,), generator=gen))] = 0.25   # one finite at least
        rows.append((holes, none, 1.0, 0, 1.0, 1.0, seed(), 8))       # -inf entries
        rows.append((holes.clone(), none, 0.9, 40, 0.95, 1.0, SEED_U1, 0))
        rows.append((normal(), none, 1.0, 0, 1.0, 1.0, SEED_U0, 0))   # u = 0
        rows.append((normal(), none, 1.0, 0, 1.0, 1.0, SEED_U1, 0))   # u = 1 - 2^-24
        rows.append((normal(), none, 0.8, 40, 0.9, 1.0, SEED_U0, 0))
        rows.append((normal(), seen, 0.8, 0, 0.95, 1.1, SEED_U1, 0))
        self.V, self.scale, self.n = V, scale, len(rows)
        self.logits = torch.stack([r[0] for r in rows])
        self.seen = torch.stack([r[1] for r in rows])
        self.temperature = torch.tensor([r[2] for r in rows], dtype=torch.float32)
        self.top_k = torch.tensor([r[3] for r in rows], dtype=torch.int32)
        self.top_p = torch.tensor([r[4] for r in rows], dtype=torch.float32)
        self.penalty = torch.tensor([r[5] for r in rows], dtype=torch.float32)
        self.seed = torch.tensor([r[6] for r in rows], dtype=torch.long)
        self.counter = torch.tensor([r[7] for r in rows], dtype=torch.long)

    def args(self, dtype, rows=None, device="cpu"):
        """The arguments of sample_rows for `rows` (all) in `dtype`."""
        sel = slice(None) if rows is None else torch.as_tensor(rows)
        t = (self.logits.to(dtype), self.seen, self.temperature, self.top_k, self.top_p,
             self.penalty, self.seed, self.counter)
        return tuple(x[sel].contiguous().to(device) for x in t)


_GRID = None


def grid():
    """Every Pool of the grid, built once."""
    global _GRID
    if _GRID is None:
        gen = torch.Generator().manual_seed(2024)
        _GRID = [Pool(V, s, gen) for V in VOCABS for s in SCALES]
    return _GRID


class RowOracle:
    """The float64 quantities of one row that the check needs, computed once
    and left unchanged: the penalised y, kth, K, the weights on K and their
    sum."""

    def __init__(self, logits_row, seen_row, T, k, p, penalty, seed, counter):
        x = logits_row.view(1, -1)
        # the penalised row in the dtype of the logits, as the serving engine had it
        y = torch.where(seen_row.view(1, -1),
                        torch.where(x > 0, x / penalty, x * penalty), x) if penalty != 1.0 else x
        self.y = y[0].double()
        V = self.y.numel()
        self.T, self.k, self.p = float(T), int(k), float(p)
        self.u = reference.uniform01(int(seed), int(counter))
        self.m = float(self.y.max())
        self.greedy = not self.T > 0
        if self.greedy:
            return
        self.kth = float(torch.topk(self.y, self.k).values[-1]) if 0 < self.k < V else NEG_INF
        self.K = self.y >= self.kth
        self.w = torch.exp((self.y - self.m) / max(self.T, 1e-5)) * self.K
        self.Z = float(self.w.sum())

    def check(self, tok, cut):
        """Assert that (tok, cut) is a valid output for this row."""
        tok, cut = int(tok), float(cut)
        y = self.y
        assert 0 <= tok < y.numel()
        if self.greedy:
            assert tok == int(y.argmax()) and cut == self.m, (tok, cut)
            return
        assert cut >= self.kth and float(y[tok]) >= cut, (tok, cut, self.kth)
        if self.p >= 1.0:
            assert cut == self.kth, (cut, self.kth)
        else:
            assert bool(((y == cut) & self.K).any()), f"cut {cut} is no kept value"
            ge = float(self.w[y >= cut].sum()) / self.Z
            gt = float(self.w[y > cut].sum()) / self.Z
            assert ge > self.p - TAU, (ge, self.p)
            assert gt <= self.p + TAU, (gt, self.p)
        ws = self.w * (y >= cut)
        cdf = torch.cumsum(ws, 0) / float(ws.sum())
        before = float(cdf[tok - 1]) if tok > 0 else 0.0  # the CDF at the kept token before tok
        assert before - TAU <= self.u < float(cdf[tok]) + TAU, (before, self.u, float(cdf[tok]))


_ORACLES = {}


def oracles(pool_index, dtype):
    """The RowOracles of grid()[pool_index] in `dtype`, built once."""
    key = (pool_index, dtype)
    if key not in _ORACLES:
        pool = grid()[pool_index]
        a = pool.args(dtype)
        _ORACLES[key] = [RowOracle(a[0][i], a[1][i], *(float(x[i]) for x in a[2:6]),
                                   int(a[6][i]), int(a[7][i])) for i in range(pool.n)]
    return _ORACLES[key]


_REFERENCE = {}


def reference_outputs(pool_index, dtype):
    """reference.sample_rows on the whole pool, computed once."""
    key = (pool_index, dtype)
    if key not in _REFERENCE:
        _REFERENCE[key] = reference.sample_rows(*grid()[pool_index].args(dtype))
    return _REFERENCE[key]


def batched_penalty_rows(logits, seen, penalty):
    """apply_repetition_penalty_batched row by row with each row's penalty."""
    return torch.stack([apply_repetition_penalty_batched(
        logits[b:b + 1], seen[b:b + 1], float(penalty[b]))[0] for b in range(logits.shape[0])])


# ---- the serving scenario of tests/_paged.py with mixed per-request options ----

GREEDY = dict(sample=False)
UNSEEDED = 9
MIXED = [
    GREEDY,
    dict(sample=True, temperature=1.0, seed=101),
    dict(sample=True, temperature=0.8, top_p=0.95, repetition_penalty=1.1, seed=202),
    GREEDY,
    dict(sample=True, temperature=1.5, top_k=1, seed=303),  # top_k = 1: the greedy tokens
    dict(sample=True, temperature=0.7, top_k=40, top_p=0.9, seed=404),
    GREEDY,
    dict(sample=True, temperature=1.2, top_k=5, seed=505),
    GREEDY,
    dict(sample=True, temperature=1.0, top_p=0.5),  # no seed: the engine draws one
    dict(sample=True, temperature=0.9, seed=2 ** 64 - 7),
]
GREEDY_IDS = [i for i, o in enumerate(MIXED) if o is GREEDY]
TOP1_ID = 4


def serve_mixed(model, options=MIXED, **kw):
    """PG.serve with options[i] for request i of the scenario -> (tokens per
    request in scenario order, the seed the engine recorded per request)."""
    from zero_transformer_amd.models.paged import ServingEngine

    prompts, counts = PG.scenario()
    eng = ServingEngine(model, PG.SLOTS, PG.NUM_PAGES, PG.R, **kw)
    out, seeds = {}, {}

    def step():
        eng.step()
        seeds.update({rid: info["seed"] for rid, info in eng.info.items()})
        out.update(eng.poll())

    ids = [eng.submit(prompts[i], counts[i], **options[i]) for i in range(7)]
    while ids[6] not in seeds:
        step()
    id11 = eng.submit(prompts[10], counts[10], **options[10])
    ids += [eng.submit(prompts[i], counts[i], **options[i]) for i in (7, 8, 9)]
    while not eng.idle():
        step()
    PG.assert_drained(eng)
    order = ids + [id11]
    return [out[i] for i in order], [seeds[i] for i in order]

