"""Flagship training-step benchmark (driver contract).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

Measures the whole-job training throughput (tokens/s over all N GPUs) of the
headline config: GPT-1.3B, ZeRO-1, bf16, ALiBi, block_size 2048, synthetic
data, random-init weights (BASELINE.json). Weak scaling: per-GPU batch is
fixed as N grows. For N > 1 the driver launches this script under
torch.distributed.run with one rank per GPU over RCCL.

A plain run sets up, warms up, times K steps and prints one JSON result line.
--dump-outputs DIR additionally writes what the last timed step produced
(see dump_outputs). --full is where any measurement beyond the headline
figure belongs; there is none today, so it changes nothing.
"""

from __future__ import annotations

import argparse
import json
import os
import time

import numpy as np
import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.abspath(__file__))

BASELINE_TOKS = 131000.0  # reference TPU v3-32 pod-level tokens/s (BASELINE.md, 760M derived)


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--model", default="1_3b_2048")
    p.add_argument("--batch", type=int, default=16, help="per-GPU sequences per step")
    p.add_argument("--accum", type=int, default=1)
    p.add_argument("--bucket-mb", type=float, default=100.0)
    p.add_argument("--train-ctx", type=int, default=0,
                   help="curriculum context (reshape max_ctx rows; 0 = max_ctx)")
    p.add_argument(
        "--ref-batch",
        action="store_true",
        help="reference-shaped headline config: 0.5M-token global batch "
        "(batch 256 x ctx-2048 packing / world), accum 4, train_context 1024 "
        "curriculum active (reference conf/config.yaml:3,22, main_zero.py:481-493); "
        "fixed global batch => strong scaling",
    )
    p.add_argument(
        "--dump-outputs",
        metavar="DIR",
        default=None,
        help="after the timed steps, write the last step's outputs as DIR/<name>.npy",
    )
    p.add_argument(
        "--full",
        action="store_true",
        help="also run every secondary measurement (none exist yet: the "
        "headline figure is all this benchmark measures)",
    )
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be >= 1")
    if args.warmup < 0:
        p.error("--warmup must be >= 0")
    return args


DUMP_SAMPLE_PER_PARAM = 4096  # elements sampled from each parameter tensor


@torch.no_grad()
def dump_outputs(out_dir, metrics, model):
    """Write what the last timed train_step handed back, one .npy per name.

    A caller of TrainEngine.train_step receives the metrics dict and the
    model updated in place: each metric goes out as a 1-element float64
    array, and the updated (bf16 working) parameters as a fixed, seeded
    sample of DUMP_SAMPLE_PER_PARAM elements per tensor, concatenated in
    named_parameters() order, float32 (~0.5M values for the 1.3B model; the
    full set would be 5 GB).
    """
    os.makedirs(out_dir, exist_ok=True)
    for k in ("train/loss", "train/grad_norm", "lr"):
        name = k.split("/")[-1]
        np.save(os.path.join(out_dir, f"{name}.npy"), np.array([metrics[k]], dtype=np.float64))
    gen = torch.Generator(device="cpu").manual_seed(4321)
    parts = []
    for _, p in model.named_parameters():
        flat = p.detach().reshape(-1)
        n = min(DUMP_SAMPLE_PER_PARAM, flat.numel())
        idx = torch.randint(0, flat.numel(), (n,), generator=gen).to(flat.device)
        parts.append(flat[idx].float().cpu())
    np.save(os.path.join(out_dir, "params_sample.npy"), torch.cat(parts).numpy())


def main():
    args = parse()
    world = int(os.environ.get("WORLD_SIZE", 1))
    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", rank))
    assert torch.cuda.is_available(), "bench.py requires MI355X GPUs"
    if world > 1:
        dist.init_process_group("nccl", rank=rank, world_size=world)
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)

    from zero_transformer_amd.models import model_getter
    from zero_transformer_amd.parallel.zero import ZeRO1Optimizer
    from zero_transformer_amd.training.trainer import TrainEngine
    from zero_transformer_amd.utils import gemm_tune
    from zero_transformer_amd.utils.lr import warmup_cosine

    gemm_tune.enable()  # committed hipBLASLt tunings (no-op if absent)

    torch.manual_seed(1234)  # identical replica init on every rank (DP)
    # repo-root-relative config so the bench runs from any cwd (rocprofv3
    # sessions run from /tmp)
    model, mcfg = model_getter(
        args.model, config_path=os.path.join(REPO, "conf", "model_config.yaml"),
        return_cfg=True,
    )
    model = model.to(device)
    n_params = model.num_params()
    seq = int(mcfg.block_size)
    if args.ref_batch:
        assert 256 % world == 0
        args.batch = 256 // world
        # Grad-accum splits the fixed 0.5M-token global batch into micro
        # batches of ~32k tokens (16 micro-steps at world=1, 2 at world=8).
        # The reference's accum=4 is quoted at 32 TPU cores (micro = 2
        # rows); keeping micro ~32k tokens here is the same memory policy:
        # saved activations for a 131k-token micro are ~180 GB on a 1.3B
        # model and thrash the 288 GB allocator (measured: 10.5 s/step of
        # alloc-retry idle, profiles/PERF.md round 2).
        args.accum = max(1, (args.batch * seq) // 32768)
        args.train_ctx = 1024
    train_ctx = args.train_ctx or seq
    opt = ZeRO1Optimizer(
        list(model.named_parameters()),
        lr=warmup_cosine(3e-4, 2000, 143000, 3e-5),
        betas=(0.9, 0.95),
        weight_decay=0.1,
        clip_value=1.0,
        bucket_mb=args.bucket_mb,
        param_dtype=torch.bfloat16,
        accum_steps=args.accum,
    )
    engine = TrainEngine(model, opt, args.accum, train_ctx, device)

    # per-rank RNG stream for dropout seeds (model init above was identical)
    torch.manual_seed(1234 + rank * 7919 + 1)
    # synthetic data, device-resident (BASELINE: synthetic / random-init)
    gen = torch.Generator(device="cpu").manual_seed(99 + rank)
    batches = [
        torch.randint(0, mcfg.vocab_size, (args.batch, seq), generator=gen).to(device)
        for _ in range(2)
    ]

    for i in range(args.warmup):
        engine.train_step(batches[i % 2])
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        metrics = engine.train_step(batches[i % 2])
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    # max over ranks
    if world > 1:
        t = torch.tensor([elapsed], device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, metrics, model)

    ms_per_step = elapsed / args.steps * 1000.0
    tokens_per_step = args.batch * seq * world  # whole-job
    value = tokens_per_step / (elapsed / args.steps)
    if rank == 0:
        print(
            json.dumps(
                {
                    "metric": "training throughput (tokens/s, whole job)",
                    "value": round(value, 1),
                    "unit": "tokens/s",
                    "n_gpus": world,
                    "steps": args.steps,
                    "warmup": args.warmup,
                    "ms_per_step": round(ms_per_step, 2),
                    "higher_is_better": True,
                    "scaling": "strong" if args.ref_batch else "weak",
                    "vs_baseline": round(value / BASELINE_TOKS, 3),
                    "dtype": "bf16",
                    "data": "synthetic",
                    "config": {
                        "model": f"GPT-{args.model} ({n_params/1e9:.2f}B params)",
                        "global_batch": args.batch * world,
                        "global_batch_tokens": args.batch * world * seq,
                        "seq_len": seq,
                        "train_context": train_ctx,
                        "parallelism": f"dp{world}+zero1",
                        "grad_accum": args.accum,
                        "dropout": float(mcfg.dropout),
                        "peak_mem_gb": round(
                            torch.cuda.max_memory_allocated(device) / 2**30, 1
                        ),
                    },
                }
            )
        )
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
