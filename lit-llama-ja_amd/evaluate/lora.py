"""Perplexity of a LoRA fine-tuned model over fixed windows on the MI355X path -- drop-in for the
reference's evaluate/lora.py (flags 53-63, the module constants 24-27; argparse, as evaluate/full.py).

The model is built by generate/lora.py's `load_model`: lit_llama.LLaMA inside lit_llama.lora.lora(r,
alpha, dropout), the pretrained checkpoint and the LoRA checkpoint loaded one after the other with
strict=False, then eval() (dense weights: the update merged into c_attn, so every window runs the base
model's launches). The wrap in the Alpaca prompt, the windows and the scoring are evaluate/adapter.py's.

--quantize gptq.int4 | gptq.int8 is this package's extension: the reference's evaluate/lora.py refuses
every --quantize (NotImplementedError, evaluate/lora.py:85-86); here the pretrained checkpoint may be a
GPTQ-quantized one, and c_attn runs the unmerged form beside the quantized weight (generate/lora.py).
--quantize llm.int8 raises NotImplementedError before anything is loaded. The text comes from files
(`--text_path`).
"""
from __future__ import annotations

import sys
import time
from pathlib import Path
from typing import Optional

import torch

wd = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(wd))

from evaluate import adapter as _v1  # noqa: E402
from lit_llama.checkpoint import read_checkpoint  # noqa: E402

instruction_tuning = True  # reference evaluate/lora.py:24; see evaluate/adapter.py's `instruction_text`
lora_r = 8
lora_alpha = 16
lora_dropout = 0.05


def main(text_path: str, *, lora_path: Path = Path("out/lora/alpaca/lit-llama-lora-finetuned.pth"),
         checkpoint_path: Path = Path("checkpoints/lit-llama/7B/lit-llama.pth"),
         tokenizer_path: Path = Path("checkpoints/lit-llama/tokenizer.model"), dtype: str = "float32",
         quantize: Optional[str] = None) -> dict:
    """reference evaluate/lora.py:52-165 (same flags and defaults; dtype float32 as there)."""
    if quantize == "llm.int8":
        raise NotImplementedError("LoRA on LLM.int8 Linears is not supported (use no quantization, gptq.int4 or "
                                  "gptq.int8)")
    dt = _v1.check_dtype(dtype)
    assert lora_path.is_file(), lora_path
    assert checkpoint_path.is_file(), checkpoint_path
    assert tokenizer_path.is_file(), tokenizer_path
    if not torch.cuda.is_available():
        raise SystemExit("evaluate/lora.py runs on a ROCm GPU (MI355X) only")
    print("Loading model ...", file=sys.stderr)
    t0 = time.time()
    model = _v1.generate_cli("lora").load_model(read_checkpoint(checkpoint_path), read_checkpoint(lora_path), quantize,
                                                r=lora_r, alpha=lora_alpha, dropout=lora_dropout, dtype=dt)
    print(f"Time to load model: {time.time() - t0:.02f} seconds.", file=sys.stderr)
    return _v1.score(model, tokenizer_path, text_path, instruction_tuning)


def cli():
    return _v1.parser("Perplexity of a LoRA fine-tuned model (reference evaluate/lora.py).", "--lora_path",
                      "out/lora/alpaca/lit-llama-lora-finetuned.pth", [None, "llm.int8", "gptq.int4", "gptq.int8"])


if __name__ == "__main__":
    a = cli().parse_args()
    main(a.text_path, lora_path=a.lora_path, checkpoint_path=a.checkpoint_path, tokenizer_path=a.tokenizer_path,
         dtype=a.dtype, quantize=a.quantize)
