"""KV-cached decode throughput of the inference model (serving evidence).

    python tools/decode_bench.py --model-size 1_3b --tokens 128 --batch 1
    python tools/decode_bench.py --model-size 1_3b --batch 16 --fast --ragged
"""

import argparse
import os
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
    args = p.parse_args()
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

    run()  # warmup pass
    tps = run()
    mode = "fast(graph)" if args.fast else "dynamic"
    if args.ragged:
        mode = (f"ragged {min(lens)}..{max(lens)} "
                + ("sequential" if args.sequential else "batched"))
    print(f"{args.model_size} {args.dtype} batch {args.batch} {mode}: "
          f"{tps * args.batch:.1f} tokens/s ({1e3 / tps:.2f} ms/token)")


if __name__ == "__main__":
    main()
