"""Decode-GEMV microbenchmark: GB/s on the weight stream per shape.

    python tools/gemv_bench.py [--dtype fp16] [--iters 200]
    python tools/gemv_bench.py --w8 [--batches 1 2 3 4 8 16] [--rounds 5]
    python tools/gemv_bench.py --w4 [--batches 1 2 3 4 8 16] [--ksplit 2 4]
    python tools/gemv_bench.py --rows --batches 17 32 48 64 [--ksplit 1 2 8]

Compares ops/csrc/gemv.hip against torch F.linear (hipBLASLt) on the 1.3B
decode shapes. The weight stream is the bound (profiles/PERF.md): report
bytes(W)/time.
"""

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

SHAPES = [  # (N, K) torch Linear (out, in) — 1.3B decode projections
    (2048, 2048),    # q/k/v/out
    (8192, 2048),    # fc1
    (2048, 8192),    # fc_resid
    (50304, 2048),   # lm_head
]


def bench(fn, iters):
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    # graph capture to remove launch overhead from the measurement
    g = torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters // 10):
        g.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (iters // 10) / 10


W8_SHAPES = [(6144, 2048), (2048, 2048), (8192, 2048), (2048, 8192)]  # 1.3B blocks


def bench_w8(args, dt, dev):
    """Both bodies of ops/csrc/gemv_w8.hip next to what ops.decode_linear runs
    for the same shape in 16 bits, the sides alternating over --rounds; the
    median per side, in us and in weight bytes over time."""
    from zero_transformer_amd import ops
    from zero_transformer_amd.ops.reference import quantize_rows_w8

    ext = ops.hip_ops()
    print(f"W8A16 vs 16-bit decode_linear ({args.dtype}); us | TB/s of weight bytes")
    for N, K in W8_SHAPES:
        w = torch.randn(N, K, device=dev, dtype=dt) * 0.02
        q, scale = quantize_rows_w8(w)
        for B in args.batches:
            x = torch.randn(B, K, device=dev, dtype=dt)
            sides = {"w16": lambda: ops.decode_linear(x, w),
                     "w8_gemm": lambda: ext.w8_gemm(x, q, scale)}
            if B <= 4:
                sides["w8_gemv"] = lambda: ext.w8_gemv(x, q, scale)
            for ks in (k for k in args.ksplit if k <= K // 512):
                sides[f"w8_gemm/ks{ks}"] = lambda ks=ks: ext.w8_gemm(x, q, scale, ks)
            times = {k: [] for k in sides}
            for _ in range(args.rounds):
                for k, fn in sides.items():
                    times[k].append(bench(fn, args.iters))
            cells = []
            for k, ts in times.items():
                t = sorted(ts)[len(ts) // 2]
                nbytes = N * K * (2 if k == "w16" else 1)
                cells.append(f"{k} {t*1e6:7.2f} us {nbytes/t/1e12:5.2f}")
            print(f"N={N:5d} K={K:5d} rows={B:2d}: " + " | ".join(cells), flush=True)


def bench_w4(args, dt, dev):
    """bench_w8 with the bodies of ops/csrc/gemv_w4.hip and the dequant +
    F.linear route of ops.linear_w4 added: per shape and row count W4, W8
    and the 16-bit path from the same call, the sides alternating over
    --rounds; the median per side, in us and in weight bytes over time (W4:
    packed codes plus scales)."""
    from zero_transformer_amd import ops
    from zero_transformer_amd.ops.reference import quantize_rows_w4, quantize_rows_w8

    ext = ops.hip_ops()
    torch.set_grad_enabled(False)  # linear_w8 routes to its kernels at inference only
    print(f"W4A16 vs W8A16 vs 16-bit decode_linear ({args.dtype}); us | TB/s of weight bytes")
    for N, K in W8_SHAPES:
        w = torch.randn(N, K, device=dev, dtype=dt) * 0.02
        q, scale = quantize_rows_w8(w)
        p4, s4 = quantize_rows_w4(w)
        nbytes = {"w16": N * K * 2, "w8": N * K, "w4": N * K // 2 + N * K // 128 * 4}
        for B in args.batches:
            x = torch.randn(B, K, device=dev, dtype=dt)
            sides = {"w16": lambda: ops.decode_linear(x, w),
                     "w8": lambda: ops.linear_w8(x, q, scale),
                     "w4_gemm": lambda: ext.w4_gemm(x, p4, s4),
                     "w4_dequant+linear": lambda: torch.nn.functional.linear(
                         x, ext.dequant_w4(p4, s4, dt == torch.bfloat16))}
            if B <= 4:
                sides["w4_gemv"] = lambda: ext.w4_gemv(x, p4, s4)
            for ks in (k for k in args.ksplit if k <= K // 512):
                sides[f"w4_gemm/ks{ks}"] = lambda ks=ks: ext.w4_gemm(x, p4, s4, ks)
            times = {k: [] for k in sides}
            for _ in range(args.rounds):
                for k, fn in sides.items():
                    times[k].append(bench(fn, args.iters))
            cells = []
            for k, ts in times.items():
                t = sorted(ts)[len(ts) // 2]
                cells.append(f"{k} {t*1e6:7.2f} us {nbytes[k.split('_')[0]]/t/1e12:5.2f}")
            print(f"N={N:5d} K={K:5d} rows={B:2d}: " + " | ".join(cells), flush=True)


def bench_rows(args, dt, dev):
    """The 17..64-row body of ops/csrc/gemm_wq_rows.hip, both formats, next to
    the dequant + F.linear route the same call took before it (linear_w8 /
    linear_w4 with grad enabled still take it) and to 16-bit decode_linear,
    the sides alternating over --rounds; the median per side in us."""
    from zero_transformer_amd import ops
    from zero_transformer_amd.ops.reference import quantize_rows_w4, quantize_rows_w8

    ext = ops.hip_ops()
    print(f"quantized rows 17-64 ({args.dtype}); median us")
    for N, K in W8_SHAPES:
        w = torch.randn(N, K, device=dev, dtype=dt) * 0.02
        q, scale = quantize_rows_w8(w)
        p4, s4 = quantize_rows_w4(w)
        for B in args.batches:
            x = torch.randn(B, K, device=dev, dtype=dt)

            def library(fn, *a):
                with torch.enable_grad():
                    return fn(x, *a)

            sides = {"w16": lambda: ops.decode_linear(x, w),
                     "w8_dequant+linear": lambda: library(ops.linear_w8, q, scale),
                     "w8_rows": lambda: ext.w8_gemm_rows(x, q, scale),
                     "w4_dequant+linear": lambda: library(ops.linear_w4, p4, s4),
                     "w4_rows": lambda: ext.w4_gemm_rows(x, p4, s4)}
            for ks in (k for k in args.ksplit if k <= K // 512):
                sides[f"w8_rows/ks{ks}"] = lambda ks=ks: ext.w8_gemm_rows(x, q, scale, ks)
                sides[f"w4_rows/ks{ks}"] = lambda ks=ks: ext.w4_gemm_rows(x, p4, s4, ks)
            times = {k: [] for k in sides}
            for _ in range(args.rounds):
                for k, fn in sides.items():
                    times[k].append(bench(fn, args.iters))
            cells = [f"{k} {sorted(ts)[len(ts) // 2]*1e6:6.2f}" for k, ts in times.items()]
            print(f"N={N:5d} K={K:5d} rows={B:2d}: " + " | ".join(cells), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", action="store_true",
                   help="time ops/csrc/gemm_wq_rows.hip (--batches 17..64) next to the "
                        "dequant + F.linear route and the 16-bit path")
    p.add_argument("--w8", action="store_true",
                   help="time ops/csrc/gemv_w8.hip next to the 16-bit decode paths")
    p.add_argument("--w4", action="store_true",
                   help="time ops/csrc/gemv_w4.hip next to W8 and the 16-bit decode paths")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--ksplit", type=int, nargs="*", default=[],
                   help="--w8 / --w4: also time the MFMA body with these workgroup K splits")
    p.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--batches", type=int, nargs="*", default=[1, 8, 16])
    args = p.parse_args()
    dt = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    dev = torch.device("cuda", 0)
    from zero_transformer_amd import ops

    if args.rows:
        return bench_rows(args, dt, dev)
    if args.w4:
        return bench_w4(args, dt, dev)
    if args.w8:
        return bench_w8(args, dt, dev)
    for B in args.batches:
        print(f"--- batch {B} ({args.dtype}) ---")
        for N, K in SHAPES:
            w = torch.randn(N, K, device=dev, dtype=dt) * 0.02
            x = torch.randn(B, K, device=dev, dtype=dt)
            wbytes = N * K * 2
            ref = x.float() @ w.float().t()
            if B <= 16:
                y = ops.hip_ops().gemv(x, w)
                ok = torch.allclose(y.float(), ref, atol=0.1, rtol=5e-2)
                t = bench(lambda: ops.hip_ops().gemv(x, w), args.iters)
                print(f"gemv   N={N:6d} K={K:5d}: {t*1e6:8.2f} us  "
                      f"{wbytes/t/1e12:6.2f} TB/s  ok={ok}")
            t = bench(lambda: torch.nn.functional.linear(x, w), args.iters)
            print(f"linear N={N:6d} K={K:5d}: {t*1e6:8.2f} us  "
                  f"{wbytes/t/1e12:6.2f} TB/s")


if __name__ == "__main__":
    main()
