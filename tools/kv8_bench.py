"""ops.attention_decode_paged_q8 against ops.attention_decode_paged at the 1.3B
head shape (H 16, D 128, pages of 64 rows), fp16 and bf16, batch 1 / 16 / 64
with 128 / 1024 / 2040 cached rows.

    python tools/kv8_bench.py

The two ops alternate in 4 rounds of 300 calls each (device events around the
300); a call takes the next of several pool sets, at least 1 GiB of 16-bit
pools together, so that no call finds its cache in the last-level cache. The
figure is the mean of the two middle rounds, us per call (append, split and
merge kernels)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zero_transformer_amd import ops
from zero_transformer_amd.ops import reference

dev = torch.device("cuda", 0)
H, D, R, M = 16, 128, 64, 32
C = H * D


def bench(fn, sets, iters):
    for i in range(10):
        fn(sets[i % len(sets)])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(sets[i % len(sets)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us


for dtype in (torch.float16, torch.bfloat16):
    for B in (1, 16, 64):
        for rows in (128, 1024, 2040):
            P = B * M + 1
            set16 = P * H * R * D * 2 * 2
            nsets = max(2, min(24, -(-(1 << 30) // set16)))
            bt = (torch.arange(B * M, dtype=torch.int32).view(B, M) + 1).to(dev)
            lens = torch.full((B,), rows, dtype=torch.int32, device=dev)
            qkv = torch.randn(B, 1, 3 * C, device=dev).to(dtype)
            slopes = reference.alibi_slopes(H).to(dev)
            s16, s8 = [], []
            for _ in range(nsets):
                k = torch.randn(P, H, R, D, device=dev).to(dtype)
                v = torch.randn(P, H, R, D, device=dev).to(dtype)
                s16.append((k, v))
                ku = torch.randint(1, 256, (P, H, R, D), device=dev, dtype=torch.uint8)
                vu = torch.randint(1, 256, (P, H, R, D), device=dev, dtype=torch.uint8)
                s8.append((ku, vu, torch.rand(P, H, R, device=dev) * 0.02,
                           torch.rand(P, H, R, device=dev) * 0.02))
            f16 = lambda s: ops.attention_decode_paged(qkv, s[0], s[1], H, slopes, bt, lens)
            f8 = lambda s: ops.attention_decode_paged_q8(qkv, *s, H, slopes, bt, lens)
            iters = 300
            t = [[], []]
            for rnd in range(4):
                t[0].append(bench(f16, s16, iters))
                t[1].append(bench(f8, s8, iters))
            a, b = sorted(t[0])[1:3], sorted(t[1])[1:3]
            m16, m8 = sum(a) / 2, sum(b) / 2
            print(f"{str(dtype)[6:]} B={B} rows={rows} sets={nsets}: 16-bit {m16:.1f} us "
                  f"(min {min(t[0]):.1f} max {max(t[0]):.1f}), int8 {m8:.1f} us "
                  f"(min {min(t[1]):.1f} max {max(t[1]):.1f}), ratio {m8 / m16:.3f}", flush=True)
            del s16, s8
            torch.cuda.empty_cache()
