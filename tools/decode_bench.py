"""KV-cached decode throughput of the inference model (serving evidence).

    python tools/decode_bench.py --model-size 1_3b --tokens 128 --batch 1
    python tools/decode_bench.py --model-size 1_3b --batch 16 --fast --ragged
    python tools/decode_bench.py --model-size 1_3b --prefill --prompt-len 1024
"""

import argparse
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
    p.add_argument("--prefill-chunk", type=int, default=None)
    p.add_argument("--runs", type=int, default=15)
    args = p.parse_args()
    args.fast = args.fast or args.prefill
    assert args.fast or not args.ragged, "--ragged goes with --fast"
    assert args.ragged or not args.sequential, "--sequential goes with --ragged"
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

    if args.prefill:
        return bench_prefill(args, model, idx, lens if args.ragged else None)

    run()  # warmup pass
    tps = run()
    mode = "fast(graph)" if args.fast else "dynamic"
    if args.ragged:
        mode = (f"ragged {min(lens)}..{max(lens)} "
                + ("sequential" if args.sequential else "batched"))
    print(f"{args.model_size} {args.dtype} batch {args.batch} {mode}: "
          f"{tps * args.batch:.1f} tokens/s ({1e3 / tps:.2f} ms/token)")


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

    def sdpa():
        return model(idx, static_cache=cache)[rows, lens_t.long() - 1]

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    times = {"native": [], "sdpa": []}
    for r in range(3 + args.runs):
        for name, f in (("native", native), ("sdpa", sdpa)):
            ms, out = timed(f)
            if r >= 3:
                times[name].append(ms)
            if r == 0:
                first = out if name == "native" else first
                diff = float((out.float() - first.float()).abs().max())
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f"{args.model_size} {args.dtype} prefill batch {B} lens {min(lens)}..{max(lens)}"
          f" chunk {args.prefill_chunk}: native {med['native']:.2f} ms "
          f"(min {min(times['native']):.2f}), sdpa forward {med['sdpa']:.2f} ms "
          f"(min {min(times['sdpa']):.2f}), ratio {med['sdpa'] / med['native']:.2f}x; "
          f"max |logit diff| {diff:.3f} (logit std {float(first.float().std()):.2f})")


if __name__ == "__main__":
    main()
