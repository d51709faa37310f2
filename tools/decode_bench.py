"""KV-cached decode throughput of the inference model (serving evidence).

    python tools/decode_bench.py --model-size 1_3b --tokens 128 --batch 1
    python tools/decode_bench.py --model-size 1_3b --batch 16 --fast --ragged
    python tools/decode_bench.py --model-size 1_3b --prefill --prompt-len 1024
    python tools/decode_bench.py --model-size 1_3b --batch 16 --fast --paged
    python tools/decode_bench.py --model-size 1_3b --batch 16 --stream 64
    python tools/decode_bench.py --model-size 1_3b --batch 16 --stream 64 --prefix-len 512
    python tools/decode_bench.py --model-size 1_3b --batch 16 --stream 64 --sample
    python tools/decode_bench.py --sampler

--paged runs the same workload through the paged KV cache (models/paged.py):
--fast [--ragged] through a ServingEngine with --batch slots, --prefill through
GPT2.prefill on a PagedKVCache. --stream N is the serving scenario: N seeded
requests (prompts of 54..119 tokens, 16..256 new tokens each) through an
engine with --batch slots, against generate_batch over the same requests in
arrival-order groups of --batch; with --sample both sides sample at the
server defaults (temperature 0.8, top-p 0.95, penalty 1.1), the engine with
one seed per request. --sampler times the sampler alone, no model: the torch
chain sampling.sample_batch against the fused ops.sample_rows kernel.
"""

import argparse
import gc
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from zero_transformer_amd.models.inference import model_getter
from zero_transformer_amd.utils import gemm_tune


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model-size", default="1_3b")
    p.add_argument("--batch", type=int, default=1)
    p.add_argument("--prompt-len", type=int, default=128)
    p.add_argument("--tokens", type=int, default=128)
    p.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    p.add_argument("--fast", action="store_true",
                   help="static KV cache + hipGraph-captured decode step")
    p.add_argument("--ragged", action="store_true",
                   help="with --fast: prompt lengths seeded-uniform in "
                   "[prompt_len // 4, prompt_len], through generate_batch "
                   "(greedy, no EOS)")
    p.add_argument("--sequential", action="store_true",
                   help="with --ragged: the same prompts one at a time "
                   "(batch-1 generate_batch calls) instead of one batch")
    p.add_argument("--prefill", action="store_true",
                   help="time the prompt pass alone (no decode): GPT2.prefill "
                   "and the SDPA static-cache forward it replaced, alternating, "
                   "median of --runs; with --ragged the --ragged lengths, "
                   "right-padded")
    p.add_argument("--paged", action="store_true",
                   help="with --fast / --prefill: the paged KV cache instead of "
                   "the static one (pages of 64 rows)")
    p.add_argument("--step", action="store_true",
                   help="time the captured decode step alone, static cache against "
                   "paged cache, alternating in one process: --tokens replays from "
                   "--prompt-len cached rows, median of --runs rounds")
    p.add_argument("--stream", type=int, default=0,
                   help="serving scenario with this many requests: engine with "
                   "--batch slots against generate_batch in groups of --batch")
    p.add_argument("--prefix-len", type=int, default=0,
                   help="with --stream: every prompt starts with the same "
                   "this-many tokens; the engine runs with and without prefix reuse")
    p.add_argument("--sample", action="store_true",
                   help="with --stream: sample at the server defaults instead of greedy")
    p.add_argument("--sampler", action="store_true",
                   help="time sample_batch against ops.sample_rows on fp16 "
                   "(B, 50304) logits drawn from N(0, 3^2), B = 1 and 16, greedy "
                   "and the server defaults; median of --runs rounds")
    p.add_argument("--kv-pages", type=int, default=0,
                   help="pages in the pool (0: what --batch full-length requests need)")
    p.add_argument("--prefill-chunk", type=int, default=None)
    p.add_argument("--runs", type=int, default=15)
    args = p.parse_args()
    if args.sampler:
        return bench_sampler(args)
    args.fast = args.fast or args.prefill or bool(args.stream) or args.step
    assert args.fast or not args.ragged, "--ragged goes with --fast"
    assert args.ragged or not args.sequential, "--sequential goes with --ragged"
    assert args.fast or not args.paged, "--paged goes with --fast, --prefill or --stream"
    gemm_tune.enable()  # committed hipBLASLt tunings (incl. decode shapes)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = model_getter(args.model_size).to(dev)
    model = (model.half() if args.dtype == "fp16" else model.to(torch.bfloat16)).eval()

    idx = torch.randint(0, model.vocab_size, (args.batch, args.prompt_len), device=dev)

    @torch.no_grad()
    def run():
        logits, presents = model(idx, use_cache=True)
        nxt = logits[:, -1:].argmax(-1)
        t0 = None
        for i in range(args.tokens):
            if i == 8:  # warm
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            logits, presents = model(nxt, use_cache=True, past_states=presents)
            nxt = logits[:, -1:].argmax(-1)
        torch.cuda.synchronize()
        return (args.tokens - 8) / (time.perf_counter() - t0)

    if args.fast:
        from zero_transformer_amd.models.inference import generate_fast

        @torch.no_grad()
        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            generate_fast(model, idx, args.tokens)
            torch.cuda.synchronize()
            return args.tokens / (time.perf_counter() - t0)

    if args.ragged:
        from zero_transformer_amd.models.inference import generate_batch

        g = torch.Generator().manual_seed(0)
        lens = torch.randint(args.prompt_len // 4, args.prompt_len + 1,
                             (args.batch,), generator=g).tolist()
        prompts = [idx[b, :n].tolist() for b, n in enumerate(lens)]
        groups = [[pr] for pr in prompts] if args.sequential else [prompts]

        @torch.no_grad()
        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = sum(len(r) for grp in groups
                    for r in generate_batch(model, grp, args.tokens))
            torch.cuda.synchronize()
            # per-sequence rate, like the other modes: x batch below
            return n / args.batch / (time.perf_counter() - t0)

    if args.stream:
        return bench_stream(args, model)
    if args.step:
        return bench_step(args, model)

    if args.paged:
        from zero_transformer_amd.models.paged import ServingEngine

        if not args.ragged:
            prompts = idx.tolist()
        rows = max(len(pr) for pr in prompts) + args.tokens
        pages = args.kv_pages or args.batch * -(-min(rows, model.num_ctx) // 64) + 1
        reuse = []

        @torch.no_grad()
        def run():
            # like generate_fast / generate_batch, a call pays for its cache
            # and its graph capture; the second figure reuses the engine
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng = ServingEngine(model, args.batch, pages, prefix_cache=False)
            for pr in prompts:
                eng.submit(pr, args.tokens)
            n = sum(len(r) for r in eng.run().values())
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for pr in prompts:
                eng.submit(pr, args.tokens)
            n2 = sum(len(r) for r in eng.run().values())
            torch.cuda.synchronize()
            reuse.append(n2 / (time.perf_counter() - t1))
            return n / args.batch / (t1 - t0)

    if args.prefill:
        return bench_prefill(args, model, idx, lens if args.ragged else None)

    run()  # warmup pass
    tps = run()
    mode = "fast(graph)" if args.fast else "dynamic"
    if args.ragged:
        mode = (f"ragged {min(lens)}..{max(lens)} "
                + ("sequential" if args.sequential else "batched"))
    if args.paged:
        mode = "paged " + mode.replace("fast(graph)", "engine(graph)")
    print(f"{args.model_size} {args.dtype} batch {args.batch} {mode}: "
          f"{tps * args.batch:.1f} tokens/s ({1e3 / tps:.2f} ms/token)"
          + (f"; engine reused {reuse[-1]:.1f} tokens/s" if args.paged else ""))


SERVER_DEFAULTS = dict(temperature=0.8, top_k=0, top_p=0.95, repetition_penalty=1.1)


@torch.no_grad()
def bench_sampler(args):
    """One sampling call of the serving step, the torch chain against the
    fused kernel, on the same logits: fp16 (B, 50304) drawn from N(0, 3^2)
    (no checkpoint), 5 % of each row marked seen. A timing is 200 calls
    between two device syncs; 2 warm-up rounds, then --runs rounds that
    alternate the two; median, min and max per call."""
    from zero_transformer_amd import ops
    from zero_transformer_amd.models.sampling import sample_batch

    dev = torch.device("cuda", 0)
    V, calls = 50304, 200
    g = torch.Generator().manual_seed(0)
    d = SERVER_DEFAULTS
    for B in (1, 16):
        logits = (torch.randn(B, V, generator=g) * 3).half().to(dev)
        seen = (torch.rand(B, V, generator=g) < 0.05).to(dev)
        vec = lambda v, dt: torch.full((B,), v, dtype=dt, device=dev)
        seed = torch.arange(B, dtype=torch.long, device=dev)
        counter = torch.zeros(B, dtype=torch.long, device=dev)
        for name, sample in (("greedy", False), ("server defaults", True)):
            rows = (logits, seen, vec(d["temperature"] if sample else 0.0, torch.float32),
                    vec(d["top_k"], torch.int32), vec(d["top_p"], torch.float32),
                    vec(d["repetition_penalty"], torch.float32), seed, counter)
            fns = {"sample_batch": lambda: sample_batch(logits, seen, sample=sample, **d),
                   "sample_rows": lambda: ops.sample_rows(*rows)}
            times = {k: [] for k in fns}
            for r in range(2 + args.runs):
                for k, f in fns.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        f()
                    torch.cuda.synchronize()
                    if r >= 2:
                        times[k].append((time.perf_counter() - t0) / calls * 1e6)
            med = {k: statistics.median(v) for k, v in times.items()}
            print(f"sampler fp16 B {B} V {V} N(0, 3^2) {name}: "
                  + ", ".join(f"{k} {med[k]:.1f} us (min {min(times[k]):.1f}, "
                              f"max {max(times[k]):.1f})" for k in med)
                  + f", sample_batch / sample_rows {med['sample_batch'] / med['sample_rows']:.2f}x")


@torch.no_grad()
def bench_step(args, model):
    """The captured decode step alone (no sampling, no prefill, no capture in
    the timed window): every sequence starts at --prompt-len cached rows and
    grows by one per replay, --tokens replays per round."""
    from zero_transformer_amd.models.inference import (GRAPH_SCRATCH_ROWS, StaticKVCache,
                                                       capture_decode_step)
    from zero_transformer_amd.models.paged import PagedKVCache

    B, T0, n = args.batch, args.prompt_len, args.tokens
    dev = next(model.parameters()).device
    attn = model.blocks[0].attn
    rows = T0 + n + GRAPH_SCRATCH_ROWS
    per = -(-rows // 64)
    geom = (model.N, B, attn.num_head, attn.head_dim)
    dtype = next(model.parameters()).dtype
    caches = {"contiguous": StaticKVCache(*geom, rows, dev, dtype),
              "paged": PagedKVCache(*geom, B * per + 1, 64, per, dev, dtype)}
    for b in range(B):
        caches["paged"].assign(b, rows)
    cur = torch.zeros(B, 1, dtype=torch.long, device=dev)
    one = torch.ones(B, dtype=torch.int32, device=dev)
    graphs = {}
    for name, cache in caches.items():
        cache.set_len(T0)

        def step(cache=cache):
            cache.advance(one)
            return model(cur, static_cache=cache)

        graphs[name], _ = capture_decode_step(step, cache, T0)
    times = {name: [] for name in graphs}
    for r in range(2 + args.runs):
        for name, graph in graphs.items():
            caches[name].set_len(T0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                graph.replay()
            torch.cuda.synchronize()
            if r >= 2:
                times[name].append((time.perf_counter() - t0) / n * 1e6)
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f"{args.model_size} {args.dtype} decode step batch {B}, rows {T0}..{T0 + n}: "
          + ", ".join(f"{k} {med[k]:.1f} us (min {min(times[k]):.1f}, max {max(times[k]):.1f})"
                      for k in med)
          + f", paged / contiguous {med['paged'] / med['contiguous']:.4f}")


@torch.no_grad()
def bench_stream(args, model):
    """The serving scenario; no EOS, so both sides emit exactly the requested
    tokens and only those are counted. Greedy, or with --sample at the server
    defaults (the two sides then draw differently: token equality says
    nothing)."""
    from zero_transformer_amd.models.inference import GRAPH_SCRATCH_ROWS, generate_batch
    from zero_transformer_amd.models.paged import ServingEngine

    g = torch.Generator().manual_seed(0)
    N, S = args.stream, args.batch
    lens = torch.randint(54, 120, (N,), generator=g).tolist()
    news = torch.randint(16, 257, (N,), generator=g).tolist()
    prefix = torch.randint(0, model.vocab_size, (args.prefix_len,), generator=g).tolist()
    prompts = [prefix + torch.randint(0, model.vocab_size, (n,), generator=g).tolist()
               for n in lens]
    limits = [min(m, model.num_ctx - len(p)) for p, m in zip(prompts, news)]
    total = sum(limits)
    attn = model.blocks[0].attn
    row_bytes = 2 * model.N * attn.num_head * attn.head_dim * 2  # k + v, 16-bit
    full = -(-min(model.num_ctx, max(len(p) + m for p, m in zip(prompts, limits))) // 64)
    pages = args.kv_pages or S * full + 1
    sampling = dict(SERVER_DEFAULTS, sample=True) if args.sample else {}

    class TimedEngine(ServingEngine):
        """Adds up the prefill time (a device sync on either side). A
        subclass, not a wrapper stored on the instance: that would put the
        engine, and its hipGraph, in a reference cycle, and a graph must not
        be destroyed by the cycle collector while another one is captured."""
        prefill_s = 0.0

        def _prefill(self, batch):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            super()._prefill(batch)
            torch.cuda.synchronize()
            self.prefill_s += time.perf_counter() - t0

    def sync_time(f):
        gc.collect()  # never inside a capture (see TimedEngine)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def static():
        out, rows = [], 0
        for i in range(0, N, S):
            grp, lim = prompts[i:i + S], limits[i:i + S]
            res = generate_batch(model, grp, max(lim), **sampling)
            out += [r[:m] for r, m in zip(res, lim)]
            rows = max(rows, len(grp) * min(
                model.num_ctx, max(len(p) + min(max(lim), model.num_ctx - len(p))
                                   for p in grp) + GRAPH_SCRATCH_ROWS))
        return out, rows

    def engine(prefix_cache):
        eng = TimedEngine(model, S, pages, prefix_cache=prefix_cache, **sampling)
        peak = 0
        ids = [eng.submit(p, m, seed=i if args.sample else None)
               for i, (p, m) in enumerate(zip(prompts, news))]
        res = {}
        while not eng.idle():
            eng.step()
            c = eng.cache
            peak = max(peak, c.num_pages - 1 - c.pages_free() - c.pages_held())
            res.update(eng.poll())
        return [res[i] for i in ids], eng, peak

    static()  # warm-up of both paths (GEMM tunings, allocator)
    engine(True)
    for _ in range(2):  # alternating, twice
        dt, (out_s, rows) = sync_time(static)
        assert sum(len(r) for r in out_s) == total
        print(f"{args.model_size} {args.dtype} stream {N} x {S} "
              f"{'sampled' if args.sample else 'greedy'} static groups: "
              f"{total / dt:.1f} tokens/s ({dt:.2f} s), KV {rows * row_bytes / 2**20:.0f} MiB")
        for pc in ((True, False) if args.prefix_len else (True,)):
            dt, (out_e, eng, peak) = sync_time(lambda: engine(pc))
            assert sum(len(r) for r in out_e) == total
            agree = sum(a == b for a, b in zip(out_e, out_s))
            print(f"{args.model_size} {args.dtype} stream {N} x {S} engine "
                  f"prefix_cache={pc}: {total / dt:.1f} tokens/s ({dt:.2f} s), "
                  f"KV pool {eng.cache.kv_bytes() / 2**20:.0f} MiB ({pages} pages), "
                  f"peak live pages {peak}, prefill {eng.prefill_s * 1e3:.0f} ms in "
                  f"{eng.prefill_calls} calls, {eng.decode_steps} decode steps, "
                  f"{agree}/{N} requests token-equal to static")


@torch.no_grad()
def bench_prefill(args, model, idx, lens):
    """Time-to-first-logits of the prompt pass, both paths on the same
    inputs: a device sync on either side of each call, 3 warm-up rounds, then
    --runs rounds alternating the two; medians. Both leave each sequence's
    last-token logits, (B, V)."""
    from zero_transformer_amd.models.inference import StaticKVCache

    B, T = idx.shape
    if lens is None:
        lens = [T] * B
    T = max(lens)
    idx = idx[:, :T].contiguous()
    dev = idx.device
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
    attn = model.blocks[0].attn
    cache = StaticKVCache(model.N, B, attn.num_head, attn.head_dim, T, dev,
                          next(model.parameters()).dtype)
    rows = torch.arange(B, device=dev)

    def native():
        return model.prefill(idx, cache, lens_t, chunk=args.prefill_chunk)

    if args.paged:
        from zero_transformer_amd.models.paged import PagedKVCache

        per = -(-T // 64)
        pcache = PagedKVCache(model.N, B, attn.num_head, attn.head_dim, B * per + 1, 64,
                              per, dev, next(model.parameters()).dtype)
        for b in range(B):
            pcache.assign(b, T)

        def paged():
            return model.prefill(idx, pcache, lens_t, chunk=args.prefill_chunk)

    def sdpa():
        return model(idx, static_cache=cache)[rows, lens_t.long() - 1]

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    other = ("paged", paged) if args.paged else ("sdpa", sdpa)
    times = {"native": [], other[0]: []}
    for r in range(3 + args.runs):
        for name, f in (("native", native), other):
            ms, out = timed(f)
            if r >= 3:
                times[name].append(ms)
            if r == 0:
                first = out if name == "native" else first
                diff = float((out.float() - first.float()).abs().max())
    med = {k: statistics.median(v) for k, v in times.items()}
    if args.paged:
        print(f"{args.model_size} {args.dtype} prefill batch {B} lens {min(lens)}..{max(lens)}"
              f" chunk {args.prefill_chunk}: contiguous {med['native']:.2f} ms "
              f"(min {min(times['native']):.2f}), paged {med['paged']:.2f} ms "
              f"(min {min(times['paged']):.2f}), ratio {med['paged'] / med['native']:.3f}x; "
              f"max |logit diff| {diff:.3f}")
        return
    print(f"{args.model_size} {args.dtype} prefill batch {B} lens {min(lens)}..{max(lens)}"
          f" chunk {args.prefill_chunk}: native {med['native']:.2f} ms "
          f"(min {min(times['native']):.2f}), sdpa forward {med['sdpa']:.2f} ms "
          f"(min {min(times['sdpa']):.2f}), ratio {med['sdpa'] / med['native']:.2f}x; "
          f"max |logit diff| {diff:.3f} (logit std {float(first.float().std()):.2f})")


if __name__ == "__main__":
    main()
