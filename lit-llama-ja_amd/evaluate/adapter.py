"""Perplexity of a LLaMA-Adapter fine-tuned model over fixed windows on the MI355X path -- drop-in for the
reference's evaluate/adapter.py (flags 52-62, the module constant 25; argparse, as evaluate/full.py).

The model is built as generate/adapter.py builds it: lit_llama.adapter.LLaMA of the size
llama_model_lookup finds, the pretrained checkpoint and the adapter checkpoint loaded one after the other
with strict=False. The text is wrapped in the Alpaca prompt (see `instruction_text`), encoded with BOS and
no EOS, trimmed to 256 * block_size tokens, cut into windows of 2048 tokens and scored by
evaluate/full.py's `perplexity`: one no-cache forward per window (the adapter prefix term included) and
the device NLL kernel over its logits (LLaMA.window_nll).

The reference fetches wikitext / ptb / c4 with `datasets` (evaluate/adapter.py:28-49); without a network
the text comes from files (`--text_path`, one or more, comma separated), as in evaluate/full.py.
--quantize llm.int8 | gptq.int4 | gptq.int8 all run (the adapter prefix term does not touch the Linears).
"""
from __future__ import annotations

import argparse
import builtins
import importlib.util
import sys
import time
from pathlib import Path
from typing import Optional

import torch

wd = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(wd))

from evaluate.full import perplexity  # noqa: E402
from lit_llama.checkpoint import read_checkpoint  # noqa: E402
from lit_llama.utils import EmptyInitOnDevice, llama_model_lookup  # noqa: E402

# reference evaluate/adapter.py:25. True: the whole text is scored inside the Alpaca prompt the model was
# fine-tuned against; False: the raw text is scored.
instruction_tuning = True


def generate_cli(name: str):
    """This package's generate/<name>.py, loaded from its file: `generate` on sys.path is generate.py (a
    module, not a package), so the script cannot be imported by name."""
    spec = importlib.util.spec_from_file_location(f"llj_generate_{name}", wd / "generate" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def instruction_text(text: str, enabled: Optional[bool] = None) -> str:
    """The string the reference tokenises (evaluate/adapter.py:117-119, evaluate/lora.py:128-130):
        sample = {"instruction": test_string, "input": input}
        test_string = generate_prompt(sample)
    `input` there is no variable of the script but the Python builtin function. It is truthy, so the
    prompt takes its "with input" form, and its input section reads "<built-in function input>". The
    perplexities are comparable with the reference's only if the token stream is the same, so the quirk
    is reproduced: the builtin itself goes into the sample. `enabled` None = this module's
    `instruction_tuning`; False returns the text as it is."""
    if not (instruction_tuning if enabled is None else enabled):
        return text
    return generate_cli("adapter").generate_prompt({"instruction": text, "input": builtins.input})


def check_dtype(dtype: str) -> torch.dtype:
    dt = getattr(torch, dtype, None)
    if not isinstance(dt, torch.dtype):  # reference evaluate/adapter.py:84-87
        raise ValueError(f"{dtype} is not a valid dtype.")
    return dt


def score(model, tokenizer_path: Path, text_path: str, wrap: Optional[bool] = None) -> dict:
    """The reference's loop over its datasets (evaluate/adapter.py:111-149) over text files:
    {path: perplexity}, printing what the reference prints."""
    from quantize.gptq import tokenizer_for

    tokenizer = tokenizer_for(tokenizer_path)
    out, total_toks = {}, 0
    t0 = time.perf_counter()
    for path in text_path.split(","):
        text = instruction_text(Path(path).read_text(encoding="utf-8"), wrap)
        enc = tokenizer.encode(text, bos=True, eos=False, device=torch.device("cuda"))
        enc = enc[None, :256 * model.config.block_size]  # add the batch dimension, trim as GPTQ's evaluation does
        ppl, _, toks = perplexity(model, enc)
        print(f"Perplexity on {path}: {ppl:.2f}")
        out[path] = ppl
        total_toks += toks
    t = time.perf_counter() - t0
    print(f"\n\nTime for inference: {t:.02f} sec total, {total_toks / t:.02f} tokens/sec", file=sys.stderr)
    print(f"Memory used: {torch.cuda.max_memory_reserved() / 1e9:.02f} GB", file=sys.stderr)
    return out


def load_model(pretrained: dict, adapter: dict, quantize: Optional[str] = None, dtype=torch.float32):
    """The adapter model of two state dicts on the GPU, in eval mode (generate/adapter.py:61-68)."""
    from lit_llama.adapter import LLaMA

    name = llama_model_lookup(pretrained)
    with EmptyInitOnDevice(device=torch.device("cuda"), dtype=dtype, quantization_mode=quantize):
        model = LLaMA.from_name(name)
    model.load_state_dict(pretrained, strict=False)  # 1. the pretrained weights
    model.load_state_dict(adapter, strict=False)     # 2. the fine-tuned adapter weights
    return model.eval()


def main(text_path: str, *, adapter_path: Path = Path("out/adapter/alpaca/lit-llama-adapter-finetuned.pth"),
         checkpoint_path: Path = Path("checkpoints/lit-llama/7B/lit-llama.pth"),
         tokenizer_path: Path = Path("checkpoints/lit-llama/tokenizer.model"), dtype: str = "float32",
         quantize: Optional[str] = None) -> dict:
    """reference evaluate/adapter.py:51-160 (same flags and defaults; dtype float32 as there)."""
    dt = check_dtype(dtype)
    assert adapter_path.is_file(), adapter_path
    assert checkpoint_path.is_file(), checkpoint_path
    assert tokenizer_path.is_file(), tokenizer_path
    if not torch.cuda.is_available():
        raise SystemExit("evaluate/adapter.py runs on a ROCm GPU (MI355X) only")
    print("Loading model ...", file=sys.stderr)
    t0 = time.time()
    model = load_model(read_checkpoint(checkpoint_path), read_checkpoint(adapter_path), quantize, dt)
    print(f"Time to load model: {time.time() - t0:.02f} seconds.", file=sys.stderr)
    return score(model, tokenizer_path, text_path)


def parser(description: str, path_flag: str, default_path: str, quantize_choices) -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=description)
    ap.add_argument("--text_path", required=True, help="UTF-8 text files to score, comma separated")
    ap.add_argument(path_flag, type=Path, default=Path(default_path))
    ap.add_argument("--checkpoint_path", type=Path, default=Path("checkpoints/lit-llama/7B/lit-llama.pth"))
    ap.add_argument("--tokenizer_path", type=Path, default=Path("checkpoints/lit-llama/tokenizer.model"))
    ap.add_argument("--dtype", default="float32")
    ap.add_argument("--quantize", default=None, choices=quantize_choices)
    return ap


def cli() -> argparse.ArgumentParser:
    return parser("Perplexity of a LLaMA-Adapter fine-tuned model (reference evaluate/adapter.py).", "--adapter_path",
                  "out/adapter/alpaca/lit-llama-adapter-finetuned.pth", [None, "llm.int8", "gptq.int4", "gptq.int8"])


if __name__ == "__main__":
    a = cli().parse_args()
    main(a.text_path, adapter_path=a.adapter_path, checkpoint_path=a.checkpoint_path, tokenizer_path=a.tokenizer_path,
         dtype=a.dtype, quantize=a.quantize)
