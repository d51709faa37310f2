"""Speculative verify: the split-S attention op and generate_speculative
against what they replace (profiles/PERF.md "Speculative verify").

    python tools/verify_bench.py --op     # attention ops alone, 1.3B head shape
    python tools/verify_bench.py --e2e    # generate_speculative vs generate_fast
    python tools/verify_bench.py --op8    # the int8 cache's verify, per layer call

--op: H 16, D 128, fp16, pages of 64 rows; per (B, T, S) the median over --runs
rounds of --iters calls each (device events around the batch of calls), the
three ops alternating inside a round: attention_verify_paged,
attention_prefill_paged on the same inputs, and T calls of
attention_decode_paged. KV GB/s = 2 * B * H * S * D * 2 bytes / verify time.
--op8: the same head shape, fp16 and bf16, T rows behind S cached ones in an
int8 paged cache; attention_verify_paged_q8, the staged route it replaces
(kv8_quantize_paged, kv8_load_paged of the S cached rows into a 16-bit staging
pair, attention_verify_append there) and the 16-bit attention_verify_paged,
alternating as in --op. Code GB/s = 2 * B * H * S * (D + 4) bytes / int8 time.
--e2e: random-weight --model-size model, batch 1, --tokens new tokens behind a
prompt of 128 and 1024, graphs on: generate_fast, generate_speculative with an
oracle draft (generate_fast's own continuation: every draft accepted, the
upper bound) and with prompt lookup on a prompt that repeats a 16-token
pattern. ms/step and tokens/s are the difference between calls of --tokens
and half as many tokens, so the prompt pass and the graph capture cancel. The
weights are random: acceptance says nothing about real text.
"""

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from zero_transformer_amd import ops
from zero_transformer_amd.ops import reference


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per call


def bench_op(args):
    dev = torch.device("cuda", 0)
    H, D, R = 16, 128, 64
    C = H * D
    sl = reference.alibi_slopes(H).to(dev)
    print("| B | T | S | verify us | prefill us | T x decode us | KV GB/s (verify) |")
    print("|---|---|---|---|---|---|---|")
    for B in (1, 4):
        for S in (128, 1024, 2048):
            M = (S + 16 + R - 1) // R
            kp = torch.randn(B * M + 1, H, R, D, device=dev).half()
            vp = torch.randn(B * M + 1, H, R, D, device=dev).half()
            bt = (torch.arange(B * M, dtype=torch.int32, device=dev) + 1).view(B, M)
            for T in (2, 5, 9, 16):
                qkv = torch.randn(B, T, 3 * C, device=dev).half()
                lens = torch.full((B,), T, dtype=torch.int32, device=dev)
                start = torch.full((B,), S - T, dtype=torch.int32, device=dev)
                dl = [torch.full((B,), S - T + i + 1, dtype=torch.int32, device=dev)
                      for i in range(T)]
                rows = [qkv[:, i:i + 1].contiguous() for i in range(T)]

                def verify():
                    ops.attention_verify_paged(qkv, kp, vp, H, sl, bt, lens, start)

                def prefill():
                    ops.attention_prefill_paged(qkv, kp, vp, H, sl, bt, lens, start)

                def decode():
                    for i in range(T):
                        ops.attention_decode_paged(rows[i], kp, vp, H, sl, bt, dl[i])

                fns = (verify, prefill, decode)
                for f in fns:
                    timed(f, 5)
                res = [[], [], []]
                for _ in range(args.runs):
                    for i, f in enumerate(fns):
                        res[i].append(timed(f, args.iters))
                v, p, d = (statistics.median(r) for r in res)
                gbs = 2 * B * H * S * D * 2 / (v * 1e-6) / 1e9
                print(f"| {B} | {T} | {S} | {v:.1f} | {p:.1f} | {d:.1f} | {gbs:.0f} |", flush=True)


def bench_op8(args):
    dev = torch.device("cuda", 0)
    H, D, R = 16, 128, 64
    C = H * D
    sl = reference.alibi_slopes(H).to(dev)
    print("| dtype | B | T | S | int8 verify us | staged us | 16-bit verify us | "
          "int8 / staged | code GB/s |")
    print("|---|---|---|---|---|---|---|---|---|")
    for dtype in (torch.float16, torch.bfloat16):
        for B in (1, 4):
            for S in (1024, 2048, 4096):
                M = (S + 16 + R - 1) // R
                P = B * M + 1
                bt = (torch.arange(B * M, dtype=torch.int32, device=dev) + 1).view(B, M)
                kp, vp = (torch.randn(P, H, R, D, device=dev).to(dtype) for _ in range(2))
                q8 = [reference.quantize_kv_rows(t) for t in (kp, vp)]
                pools = [q8[0][0], q8[1][0], q8[0][1], q8[1][1]]
                stage = [torch.zeros(B, H, M * R, D, device=dev, dtype=dtype) for _ in range(2)]
                start = torch.full((B,), S, dtype=torch.int32, device=dev)
                for T in (5, 16):
                    qkv = torch.randn(B, T, 3 * C, device=dev).to(dtype)
                    lens = torch.full((B,), T, dtype=torch.int32, device=dev)

                    def native():
                        ops.attention_verify_paged_q8(qkv, *pools, H, sl, bt, lens, start)

                    def staged():
                        ops.kv8_quantize_paged(qkv, *pools, bt, lens, start)
                        ops.kv8_load_paged(*pools, bt, start, *stage)
                        ops.attention_verify_append(qkv, *stage, H, sl, lens, start)

                    def wide():
                        ops.attention_verify_paged(qkv, kp, vp, H, sl, bt, lens, start)

                    fns = (native, staged, wide)
                    for f in fns:
                        timed(f, 5)
                    res = [[], [], []]
                    for _ in range(args.runs):
                        for i, f in enumerate(fns):
                            res[i].append(timed(f, args.iters))
                    n, s, w = (statistics.median(r) for r in res)
                    gbs = 2 * B * H * S * (D + 4) / (n * 1e-6) / 1e9
                    print(f"| {str(dtype)[6:]} | {B} | {T} | {S} | {n:.1f} | {s:.1f} | {w:.1f} | "
                          f"{n / s:.2f} | {gbs:.0f} |", flush=True)


def bench_e2e(args):
    from zero_transformer_amd.models.inference import (
        generate_fast, generate_speculative, model_getter)

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = model_getter(args.model_size).to(dev).half().eval()
    n, K = args.tokens, args.draft_len
    print("| prompt | path | whole call ms | steps | ms/step | accepted/step | tokens/s |")
    print("|---|---|---|---|---|---|---|")
    for T0 in (128, 1024):
        g = torch.Generator().manual_seed(T0)
        rand = torch.randint(1, model.vocab_size, (1, T0), generator=g).to(dev)
        rep = rand[:, :16].repeat(1, T0 // 16)
        want = generate_fast(model, rand, n)[0].tolist()

        def oracle(tokens):
            return [want[len(t):len(t) + K] for t in tokens]

        runs = (
            ("generate_fast", lambda m: (generate_fast(model, rand, m), m - 1, 0)),
            ("speculative, oracle draft",
             lambda m: generate_speculative(model, rand, m, draft_len=K, draft_fn=oracle)),
            ("generate_fast, repetitive prompt",
             lambda m: (generate_fast(model, rep, m), m - 1, 0)),
            ("speculative, prompt lookup, repetitive prompt",
             lambda m: generate_speculative(model, rep, m, draft_len=K)),
        )
        for name, fn in runs:
            # whole calls (prompt pass and graph capture included) of n and
            # n / 2 tokens: the difference is steps alone
            res = {}
            for m in (n // 2, n):
                fn(m)
                ts = []
                for _ in range(args.runs):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    _, steps, acc = fn(m)
                    torch.cuda.synchronize()
                    ts.append(time.perf_counter() - t0)
                res[m] = (statistics.median(ts), steps, acc)
            (t1, s1, _), (t2, s2, acc) = res[n // 2], res[n]
            print(f"| {T0} | {name} | {t2 * 1e3:.1f} | {s2} | "
                  f"{(t2 - t1) * 1e3 / max(s2 - s1, 1):.2f} | {acc / max(s2, 1):.2f} | "
                  f"{(n - n // 2) / (t2 - t1):.0f} |", flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--op", action="store_true")
    p.add_argument("--op8", action="store_true")
    p.add_argument("--e2e", action="store_true")
    p.add_argument("--model-size", default="1_3b_2048")
    p.add_argument("--tokens", type=int, default=128)
    p.add_argument("--draft-len", type=int, default=4)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--iters", type=int, default=50)
    args = p.parse_args()
    assert torch.cuda.is_available(), "verify_bench needs the GPU"
    if args.op:
        bench_op(args)
    if args.op8:
        bench_op8(args)
    if args.e2e:
        bench_e2e(args)


if __name__ == "__main__":
    main()
