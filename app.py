"""Interactive inference app (the reference app.py role, MI355X-native).

Two modes:
  CLI:    python app.py --model-size 760m --checkpoint torch_760m.pth \
              --prompt "Hello" --max-new-tokens 64 --top-p 0.95
  Server: python app.py --model-size 760m --checkpoint ... --serve --port 7860
          POST /generate {"prompt": ..., "max_new_tokens": ..., ...}
          (FastAPI + uvicorn instead of the reference's Gradio UI — same
          streaming KV-cached generation + samplers, reference app.py:42-142.)
          POST /generate_batch {"prompts": [...], ...same options...,
                                "prefill_chunk": P (optional)}
            -> {"completions": [...]}: prompts of any lengths, one batch
  Several --prompt flags on the CLI go through the same batched path and
  print one completion per line.
  Paged:  python app.py ... --serve --paged --slots 16 --kv-pages 512
          POST /submit {"prompt": ..., "max_new_tokens": ..., ...same options...,
                        "seed": S (optional)} -> {"completion": ...}
          One engine thread (models/paged.py ServingEngine: paged KV cache,
          continuous batching, prefix reuse) serves every /submit: a request
          joins the running batch and its call returns when it is done. The
          sampling options are the request's, with the defaults of /generate;
          a body that names none of them takes the server's (the command
          line's). The same prompt, options and "seed" give the same
          completion, whatever else is in the batch.

Tokenizer: GPT-NeoX-20B via transformers when its assets are cached locally
(reference app.py:27); otherwise a byte-level fallback so the app works on
network-less boxes and with the 256-vocab test model.
"""

from __future__ import annotations

import argparse

import torch

from torch_compatability.GPT2 import model_getter
from zero_transformer_amd.models.inference import generate_batch
from zero_transformer_amd.models.sampling import generate_stream


class ByteTokenizer:
    eos_token_id = None

    def encode(self, s: str):
        return list(s.encode("utf-8", errors="replace"))

    def decode(self, ids):
        return bytes(int(i) % 256 for i in ids).decode("utf-8", errors="replace")


def load_tokenizer():
    try:
        from transformers import AutoTokenizer

        return AutoTokenizer.from_pretrained("EleutherAI/gpt-neox-20b", local_files_only=True)
    except Exception:
        return ByteTokenizer()


def model_creator(size: str, checkpoint: str | None, device: torch.device):
    """reference app.py:30-39: build -> device -> half -> eval."""
    if device.type == "cuda":
        from zero_transformer_amd.utils import gemm_tune

        gemm_tune.enable()
    model = model_getter(size, model_checkpoint=checkpoint)
    model = model.to(device)
    if device.type == "cuda":
        model = model.half()
    return model.eval()


def generate_text(model, tok, device, prompt: str, **kw) -> str:
    ids = tok.encode(prompt)
    idx = torch.tensor([ids], dtype=torch.long, device=device)
    out = list(generate_stream(model, idx, eos_token=getattr(tok, "eos_token_id", None), **kw))
    return tok.decode(out)


def generate_texts(model, tok, prompts, **kw) -> list:
    """Completions for several prompts of any lengths in one ragged batch
    (inference.generate_batch: per-sequence KV lengths, batched sampling)."""
    outs = generate_batch(model, [tok.encode(s) for s in prompts],
                          kw.pop("max_new_tokens"),
                          eos_token=getattr(tok, "eos_token_id", None), **kw)
    return [tok.decode(o) for o in outs]


class EngineWorker:
    """One thread that owns a ServingEngine: submit() may be called from any
    thread, queues the request and blocks until its tokens are ready. The
    thread sleeps on the queue while the engine is idle."""

    def __init__(self, engine):
        import queue
        import threading

        self.engine = engine
        self.inbox = queue.Queue()
        self.pending = {}  # request id -> (event, result holder)
        self.failed = None  # what ended the thread, if anything did
        self.thread = threading.Thread(target=self._loop, daemon=True)
        self.thread.start()

    def submit(self, tokens, max_new_tokens: int, **options) -> list:
        """`options`: ServingEngine.submit's sampling options and seed."""
        import threading

        done, box = threading.Event(), {}
        self.inbox.put((tokens, max_new_tokens, done, box, options))
        # a timed wait: a request queued after the thread has died is caught
        # here, not by the thread's own clean-up
        while not done.wait(0.5):
            if self.failed is not None:
                self._fail(self.failed)
        if "error" in box:
            raise box["error"]
        return box["tokens"]

    def _take(self, item) -> None:
        tokens, n, done, box, options = item
        try:
            self.pending[self.engine.submit(tokens, n, **options)] = (done, box)
        except ValueError as e:  # a request that can never fit, or a bad option
            box["error"] = e
            done.set()

    def _loop(self) -> None:
        try:
            self._serve()
        except BaseException as e:  # the engine is gone: nobody may wait for it
            self.failed = e
            self._fail(e)
            raise

    def _fail(self, err) -> None:
        """Hand `err` to every caller that waits or is queued."""
        import queue

        waiting = list(self.pending.values())
        self.pending.clear()
        try:
            while True:
                item = self.inbox.get_nowait()
                if item is not None:
                    waiting.append(item[2:4])
        except queue.Empty:
            pass
        for done, box in waiting:
            box["error"] = RuntimeError(f"the serving engine stopped: {err!r}")
            done.set()

    def _serve(self) -> None:
        import queue

        while True:
            if self.engine.idle() and not self.pending:
                item = self.inbox.get()
                if item is None:
                    return
                self._take(item)
            try:
                while True:
                    item = self.inbox.get_nowait()
                    if item is None:
                        return
                    self._take(item)
            except queue.Empty:
                pass
            if not self.engine.idle():
                self.engine.step()
            for rid, toks in self.engine.poll().items():
                done, box = self.pending.pop(rid)
                box["tokens"] = toks
                done.set()

    def close(self) -> None:
        self.inbox.put(None)
        self.thread.join()


def _options(req: dict) -> dict:
    """Sampling options of a request body, with the server defaults."""
    return dict(
        max_new_tokens=int(req.get("max_new_tokens", 128)),
        temperature=float(req.get("temperature", 0.8)),
        top_k=int(req.get("top_k", 0)),
        top_p=float(req.get("top_p", 0.95)),
        repetition_penalty=float(req.get("repetition_penalty", 1.1)),
        sample=not bool(req.get("greedy", False)),
        prefill_chunk=(int(req["prefill_chunk"])
                       if req.get("prefill_chunk") is not None else None),
    )


SAMPLING_FIELDS = ("temperature", "top_k", "top_p", "repetition_penalty", "greedy")


def _submit_options(req: dict) -> dict:
    """The options of a /submit body for ServingEngine.submit: those of
    _options if the body names a sampling field, else none of them (the
    engine's own defaults); "seed" whenever it is given."""
    out = {}
    if any(k in req for k in SAMPLING_FIELDS):
        o = _options(req)
        out = {k: o[k] for k in ("temperature", "top_k", "top_p",
                                 "repetition_penalty", "sample")}
    if req.get("seed") is not None:
        out["seed"] = int(req["seed"])
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model-size", default="test")
    p.add_argument("--checkpoint", default=None)
    p.add_argument("--prompt", action="append", default=None,
                   help="repeat for several prompts: they run as one batch "
                   "and print one completion per line")
    p.add_argument("--max-new-tokens", type=int, default=128)
    p.add_argument("--temperature", type=float, default=0.8)
    p.add_argument("--top-k", type=int, default=0)
    p.add_argument("--top-p", type=float, default=0.95)
    p.add_argument("--repetition-penalty", type=float, default=1.1)
    p.add_argument("--greedy", action="store_true")
    p.add_argument("--prefill-chunk", type=int, default=None,
                   help="send the prompt through the prefill in slices of this "
                   "many positions (bounds activation memory of long prompts)")
    p.add_argument("--paged", action="store_true",
                   help="with --serve: POST /submit through one continuous-"
                   "batching engine over a paged KV cache")
    p.add_argument("--slots", type=int, default=16,
                   help="--paged: sequences decoded per step")
    p.add_argument("--kv-pages", type=int, default=256,
                   help="--paged: pages of 64 rows in the KV pool (page 0 is reserved)")
    p.add_argument("--serve", action="store_true")
    p.add_argument("--port", type=int, default=7860)
    p.add_argument(
        "--host",
        default="127.0.0.1",
        help="bind address for --serve (loopback by default; pass 0.0.0.0 to "
        "expose the unauthenticated endpoint to the network explicitly)",
    )
    args = p.parse_args()

    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    model = model_creator(args.model_size, args.checkpoint, device)
    tok = load_tokenizer()
    kw = dict(
        max_new_tokens=args.max_new_tokens,
        temperature=args.temperature,
        top_k=args.top_k,
        top_p=args.top_p,
        repetition_penalty=args.repetition_penalty,
        sample=not args.greedy,
        prefill_chunk=args.prefill_chunk,
    )

    if args.serve:
        import uvicorn

        engine = None
        if args.paged:
            from zero_transformer_amd.models.paged import ServingEngine

            opts = {k: v for k, v in kw.items() if k != "max_new_tokens"}
            engine = ServingEngine(model, args.slots, args.kv_pages,
                                   eos_token=getattr(tok, "eos_token_id", None), **opts)
        app = build_app(model, tok, device, engine)
        uvicorn.run(app, host=args.host, port=args.port)
    else:
        prompts = args.prompt or ["Hello"]
        if len(prompts) == 1:
            print(prompts[0] + generate_text(model, tok, device, prompts[0], **kw))
        else:
            for prompt, text in zip(prompts, generate_texts(model, tok, prompts, **kw)):
                print((prompt + text).replace("\n", "\\n"))


def build_app(model, tok, device, engine=None):
    """FastAPI app over a loaded model (split out of main() so the server
    surface is unit-testable with fastapi.testclient). With a ServingEngine,
    POST /submit is served by one engine thread."""
    from fastapi import Body, FastAPI, HTTPException

    app = FastAPI(title="zero_transformer_amd inference")

    if engine is not None:
        worker = EngineWorker(engine)
        app.state.worker = worker

        @app.post("/submit")
        def submit(req: dict = Body(...)):
            # a sync endpoint: each call waits in its own server thread
            try:
                toks = worker.submit(tok.encode(str(req["prompt"])),
                                     int(req.get("max_new_tokens", 128)),
                                     **_submit_options(req))
            except ValueError as e:
                raise HTTPException(status_code=400, detail=str(e))
            except RuntimeError as e:
                raise HTTPException(status_code=503, detail=str(e))
            return {"completion": tok.decode(toks)}

    @app.post("/generate")
    def generate(req: dict = Body(...)):
        text = generate_text(model, tok, device, str(req["prompt"]), **_options(req))
        return {"completion": text}

    @app.post("/generate_batch")
    def generate_batch_(req: dict = Body(...)):
        prompts = [str(s) for s in req["prompts"]]
        return {"completions": generate_texts(model, tok, prompts, **_options(req))}

    @app.get("/")
    def index():
        # minimal demo page (the reference's Gradio UI role)
        from fastapi.responses import HTMLResponse

        return HTMLResponse(
            """<!doctype html><title>zero_transformer_amd</title>
<h2>zero_transformer_amd inference</h2>
<textarea id=p rows=6 cols=80>Hello</textarea><br>
max new tokens <input id=n value=128 size=4>
temperature <input id=t value=0.8 size=4>
top-p <input id=tp value=0.95 size=4>
<button onclick="go()">Generate</button>
<pre id=out></pre>
<script>
async function go(){
  const r = await fetch('/generate', {method:'POST',
    headers:{'Content-Type':'application/json'},
    body: JSON.stringify({prompt: p.value, max_new_tokens: +n.value,
                          temperature: +t.value, top_p: +tp.value})});
  out.textContent = (await r.json()).completion;
}
</script>"""
        )

    return app


if __name__ == "__main__":
    main()
