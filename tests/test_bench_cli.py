"""bench.py command line and --dump-outputs writer (CPU; the timed path
itself needs a GPU and is covered by running the benchmark)."""

import sys

import numpy as np
import pytest
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_parse_defaults_and_new_options(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = _parse(monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert a.full is True and a.dump_outputs == "somewhere"


def test_parse_rejects_zero_steps(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def test_dump_outputs_files_dtypes_and_fixed_sample(tmp_path):
    torch.manual_seed(0)
    model = torch.nn.Sequential(
        torch.nn.Linear(100, 100, bias=False), torch.nn.Linear(100, 3)
    ).to(torch.bfloat16)
    metrics = {"train/loss": 2.5, "train/ppl": 12.2, "train/grad_norm": 0.75, "lr": 1e-4}
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), metrics, model)
    bench.dump_outputs(str(b), metrics, model)

    assert sorted(p.name for p in a.iterdir()) == [
        "grad_norm.npy", "loss.npy", "lr.npy", "params_sample.npy",
    ]
    for name, want in (("loss", 2.5), ("grad_norm", 0.75), ("lr", 1e-4)):
        v = np.load(a / f"{name}.npy")
        assert v.dtype == np.float64 and v.shape == (1,) and v[0] == want

    s = np.load(a / "params_sample.npy")
    assert s.dtype == np.float32
    # 10000-element weight is sampled, the small tensors contribute
    # min(numel, cap) draws each
    cap = bench.DUMP_SAMPLE_PER_PARAM
    assert s.shape == (min(cap, 10000) + min(cap, 300) + min(cap, 3),)
    assert np.array_equal(s, np.load(b / "params_sample.npy"))
    # every sampled value is a value of the model
    allv = torch.cat([p.detach().float().reshape(-1) for p in model.parameters()]).numpy()
    assert np.isin(s, allv).all()
