"""On-hardware distributed-path validation within a 1-GPU lease.

RCCL refuses two ranks on one device ("Duplicate GPU detected", measured —
tools/probes/rccl_world2_probe.py) and this pool's MI355X rejects CPX
compute partitioning (amd-smi: AMDSMI_STATUS_UNKNOWN_ERROR), so a true
multi-rank RCCL run needs the driver's 8-GPU node. What CAN be executed on
one GPU, and is here:

  * the real RCCL communicator + reduce-scatter/all-gather kernels at
    world_size=1, launched from a side HIP stream exactly like the ZeRO
    engine's comm stream (test_rccl_world1_collectives);
  * the full ZeRO-1 world_size=2 step on CUDA tensors over gloo — every
    bucket view, backward hook, comm-stream wait and the sharded AdamW
    run on the GPU; only the wire transport is gloo
    (test_zero1_world2_gpu_matches_single) — numerically against a
    single-process GPU run of the combined batch.
"""

import os
import pickle
import socket
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from zero_transformer_amd.models import GPT
from zero_transformer_amd.parallel.zero import ZeRO1Optimizer
from zero_transformer_amd.training.trainer import TrainEngine
from zero_transformer_amd.utils.config import DotDict

# head_dim 64 so the HIP flash-attention path (not eager fallback) runs
CFG = DotDict(
    embedding_dim=256, vocab_size=512, num_head=4, block_size=64,
    dropout=0.0, N=2, alibi_attn=True,
)
STEPS = 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_rccl_world1_collectives():
    """Real RCCL reduce-scatter / all-gather / all-reduce kernels issued
    from a non-default HIP stream (the ZeRO comm-stream pattern)."""
    assert torch.cuda.is_available()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(_free_port()))
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        flat = torch.randn(1 << 20, device=dev)
        shard = torch.empty(1 << 20, device=dev)
        gathered = torch.empty(1 << 20, device=dev)
        comm_stream = torch.cuda.Stream(device=dev)
        comm_stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(comm_stream):
            dist.reduce_scatter_tensor(shard, flat, op=dist.ReduceOp.AVG)
            dist.all_gather_into_tensor(gathered, shard)
            loss = torch.ones(1, device=dev)
            dist.all_reduce(loss)
        torch.cuda.current_stream(dev).wait_stream(comm_stream)
        torch.cuda.synchronize(dev)
        assert torch.equal(shard, flat)
        assert torch.equal(gathered, flat)
        assert loss.item() == 1.0
    finally:
        dist.destroy_process_group()


def _gpu_batches():
    rng = np.random.default_rng(31)
    return [rng.integers(0, 512, size=(4, 64)) for _ in range(STEPS)]


def _build_gpu(dev):
    torch.manual_seed(17)
    model = GPT(CFG).to(dev)
    opt = ZeRO1Optimizer(
        list(model.named_parameters()), lr=0.01, accum_steps=2,
        weight_decay=0.1, bucket_mb=0.5, param_dtype=torch.bfloat16,
    )
    return model, opt, TrainEngine(model, opt, 2, 64, dev)


def _gpu_worker(rank, world, tmpdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    dist.init_process_group(
        "gloo", init_method=f"file://{tmpdir}/store", rank=rank, world_size=world
    )
    try:
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        model, opt, eng = _build_gpu(dev)
        assert opt.overlap_comm, "comm stream must be active (cuda, world>1)"
        losses = [
            eng.train_step(b[rank * 2 : rank * 2 + 2])["train/loss"]
            for b in _gpu_batches()
        ]
        sd = opt.full_param_state_dict()
        if rank == 0:
            with open(os.path.join(tmpdir, "result.pkl"), "wb") as f:
                pickle.dump((losses, sd), f)
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_zero1_world2_gpu_matches_single():
    dev = torch.device("cuda", 0)
    model, opt, eng = _build_gpu(dev)
    ref_losses = [eng.train_step(b)["train/loss"] for b in _gpu_batches()]
    ref_sd = opt.full_param_state_dict()

    with tempfile.TemporaryDirectory() as tmpdir:
        ctx = mp.get_context("spawn")
        procs = [ctx.Process(target=_gpu_worker, args=(r, 2, tmpdir)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(560)
            assert p.exitcode == 0, f"worker failed with {p.exitcode}"
        with open(os.path.join(tmpdir, "result.pkl"), "rb") as f:
            losses, sd = pickle.load(f)

    for la, lb in zip(ref_losses, losses):
        assert abs(la - lb) < 5e-3, f"loss diverged: {la} vs {lb}"
    # bf16 buckets + different grad-accumulation groupings (micro rows 2 vs
    # 1 per rank) put per-element Adam noise at step 1-2 around 1e-3; a few
    # near-zero-grad elements land ~3e-2. Mechanism check, not bit parity:
    # bound the max and the mean.
    for n, p in ref_sd.items():
        d = (p - sd[n]).abs()
        assert float(d.max()) < 0.1, f"{n} diverged (max {float(d.max()):.4f})"
        assert float(d.mean()) < 5e-3, f"{n} diverged (mean {float(d.mean()):.5f})"
