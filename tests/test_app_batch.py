"""Batched serving surface: POST /generate_batch and repeated --prompt go
through inference.generate_batch and give each prompt what /generate gives it
alone (greedy, so deterministic)."""

import sys

import pytest
import torch

import app as app_module
from app import ByteTokenizer, build_app, generate_text, generate_texts
from torch_compatability.GPT2 import model_getter

PROMPTS = ["Hi", "Hello, MI355X!", "ragged"]
OPTS = {"max_new_tokens": 5, "greedy": True, "repetition_penalty": 1.2}


@pytest.fixture(scope="module")
def served():
    torch.manual_seed(4)
    model = model_getter("test", config_path="torch_compatability/model_config.yaml").eval()
    return model, ByteTokenizer(), torch.device("cpu")


def test_generate_batch_endpoint_matches_single_prompt_endpoint(served):
    pytest.importorskip("fastapi")  # the server only; the CLI test needs none
    from fastapi.testclient import TestClient

    client = TestClient(build_app(*served))
    r = client.post("/generate_batch", json={"prompts": PROMPTS, **OPTS})
    assert r.status_code == 200
    got = r.json()["completions"]
    assert len(got) == len(PROMPTS)
    for prompt, text in zip(PROMPTS, got):
        one = client.post("/generate", json={"prompt": prompt, **OPTS}).json()["completion"]
        assert text == one


def test_cli_prompts(served, monkeypatch, capsys):
    model, tok, dev = served
    monkeypatch.setattr(app_module, "model_creator", lambda *a: model)
    monkeypatch.setattr(app_module, "load_tokenizer", lambda: tok)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    kw = dict(max_new_tokens=4, sample=False, repetition_penalty=1.0, temperature=0.8,
              top_k=0, top_p=0.95)
    base = ["app.py", "--greedy", "--max-new-tokens", "4", "--repetition-penalty", "1.0"]

    monkeypatch.setattr(sys, "argv", base + ["--prompt", "Hi"])
    app_module.main()
    assert capsys.readouterr().out == "Hi" + generate_text(model, tok, dev, "Hi", **kw) + "\n"

    monkeypatch.setattr(sys, "argv", base + ["--prompt", "Hi", "--prompt", "Hello"])
    app_module.main()
    lines = capsys.readouterr().out.splitlines()
    texts = generate_texts(model, tok, ["Hi", "Hello"], **kw)
    assert lines == [(p + t).replace("\n", "\\n") for p, t in zip(["Hi", "Hello"], texts)]
    assert texts == [generate_text(model, tok, dev, p, **kw) for p in ["Hi", "Hello"]]
