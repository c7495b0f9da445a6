"""Instruction-following generation with a LoRA fine-tuned model on the MI355X path -- drop-in for the
reference's generate/lora.py (flags 25-35, the module constants 20-22; argparse, as generate.py).

The model is lit_llama.LLaMA built inside lit_llama.lora.lora(r, alpha, dropout), so c_attn carries
lora_A / lora_B; the pretrained checkpoint and the LoRA checkpoint (what lora_state_dict selects) are
loaded one after the other with strict=False, then eval(). The instruction is wrapped in the Alpaca
prompt the model was trained against and the text after "### Response:" is printed.

Dense weights (no --quantize): eval() merges the update into c_attn's weight (llj_lora_merge, the
reference's rounding points), so decoding runs the base model's launches -- the reference's only form.
--quantize gptq.int4 | gptq.int8 is this package's extension (the reference raises NotImplementedError for
any --quantize, generate/lora.py:59-60): the pretrained checkpoint is a GPTQ-quantized one, the update
stays beside the quantized weight and c_attn runs the unmerged form, the low-rank term in the epilogue
of its own launch plus one small down-projection launch per layer. --quantize llm.int8 raises
NotImplementedError.
"""
from __future__ import annotations

import argparse
import importlib.util
import sys
import time
from pathlib import Path
from typing import Optional

import torch

wd = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(wd))

from generate import generate  # noqa: E402  (generate.py next to this directory)
from lit_llama import HFTokenizer, LLaMA, Tokenizer  # noqa: E402
from lit_llama.checkpoint import read_checkpoint  # noqa: E402
from lit_llama.lora import lora  # noqa: E402
from lit_llama.utils import EmptyInitOnDevice, llama_model_lookup  # noqa: E402

lora_r = 8
lora_alpha = 16
lora_dropout = 0.05


def _v1_cli():
    """This package's generate/adapter.py, loaded from its file (for the Alpaca prompt): `generate` on
    sys.path is generate.py (a module, not a package), so the sibling script cannot be imported by name."""
    spec = importlib.util.spec_from_file_location("llj_generate_adapter", Path(__file__).with_name("adapter.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_V1 = _v1_cli()
RESPONSE_MARK, generate_prompt = _V1.RESPONSE_MARK, _V1.generate_prompt


def load_model(pretrained: dict, lora_checkpoint: dict, quantize: Optional[str] = None, r: int = lora_r,
               alpha: int = lora_alpha, dropout: float = lora_dropout, dtype=torch.bfloat16) -> LLaMA:
    """The LoRA model of two state dicts on the GPU, in eval mode: merged when dense, unmerged on a
    gptq.int4 / gptq.int8 base."""
    if quantize == "llm.int8":
        raise NotImplementedError("LoRA on LLM.int8 Linears is not supported (use no quantization, gptq.int4 or "
                                  "gptq.int8)")
    name = llama_model_lookup(pretrained)
    with EmptyInitOnDevice(device=torch.device("cuda"), dtype=dtype, quantization_mode=quantize), \
            lora(r=r, alpha=alpha, dropout=dropout, enabled=True):
        model = LLaMA.from_name(name)
    model.load_state_dict(pretrained, strict=False)       # 1. the pretrained weights
    model.load_state_dict(lora_checkpoint, strict=False)  # 2. the fine-tuned LoRA weights
    return model.eval()


def main(prompt: str = "What food do lamas eat?", input: str = "",
         lora_path: Path = Path("out/lora/alpaca/lit-llama-lora-finetuned.pth"),
         pretrained_path: Path = Path("checkpoints/lit-llama/7B/lit-llama.pth"),
         tokenizer_path: Path = Path("checkpoints/lit-llama/tokenizer.model"), quantize: Optional[str] = None,
         max_new_tokens: int = 100, top_k: int = 200, temperature: float = 0.8) -> None:
    """Generates a response to an instruction and an optional input (reference generate/lora.py:25-106)."""
    model, tokenizer = load(lora_path, pretrained_path, tokenizer_path, quantize)
    text = generate_prompt({"instruction": prompt, "input": input})
    encoded = tokenizer.encode(text, bos=True, eos=False, device=torch.device("cuda"))
    prompt_length = encoded.size(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    y = generate(model, encoded, max_new_tokens, temperature=temperature, top_k=top_k, eos_id=tokenizer.eos_id)
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    model.reset_cache()
    print(tokenizer.decode(y).split(RESPONSE_MARK)[1].strip())
    tokens_generated = y.size(0) - prompt_length
    print(f"\n\nTime for inference: {t:.02f} sec total, {tokens_generated / t:.02f} tokens/sec", file=sys.stderr)
    print(f"Memory used: {torch.cuda.max_memory_reserved() / 1e9:.02f} GB", file=sys.stderr)


def main_prompts_file(prompts_file: Path, lora_path: Path = Path("out/lora/alpaca/lit-llama-lora-finetuned.pth"),
                      pretrained_path: Path = Path("checkpoints/lit-llama/7B/lit-llama.pth"),
                      tokenizer_path: Path = Path("checkpoints/lit-llama/tokenizer.model"),
                      quantize: Optional[str] = None, max_new_tokens: int = 100, top_k: int = 200,
                      temperature: float = 0.8, packed_prefill: bool = False) -> None:
    """--prompts_file (main keeps the reference's signature): one instruction per non-empty line instead of --prompt /
    --input, all generated as one batch as generate/adapter.py does it; packed_prefill: prefilled as one packed batch
    as well. An unmerged LoRA on a quantized base has no batched route: generate_prompts runs its prompts one after
    the other."""
    model, tokenizer = load(lora_path, pretrained_path, tokenizer_path, quantize)
    _V1.run_prompts_file(model, tokenizer, prompts_file, max_new_tokens, top_k, temperature, packed_prefill)


def load(lora_path: Path, pretrained_path: Path, tokenizer_path: Path, quantize: Optional[str]):
    """(model, tokenizer) of the two checkpoints (load_model), on the GPU in eval mode."""
    assert lora_path.is_file(), lora_path
    assert pretrained_path.is_file(), pretrained_path
    assert tokenizer_path.is_file(), tokenizer_path
    if quantize == "llm.int8":
        raise NotImplementedError("LoRA on LLM.int8 Linears is not supported (use no quantization, gptq.int4 or "
                                  "gptq.int8)")
    if not torch.cuda.is_available():
        raise SystemExit("generate/lora.py runs on a ROCm GPU (MI355X) only")
    print("Loading model ...", file=sys.stderr)
    t0 = time.time()
    model = load_model(read_checkpoint(pretrained_path), read_checkpoint(lora_path), quantize)
    print(f"Time to load model: {time.time() - t0:.02f} seconds.", file=sys.stderr)
    tokenizer = HFTokenizer(tokenizer_path) if tokenizer_path.suffix == ".json" else Tokenizer(tokenizer_path)
    return model, tokenizer


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="Generates a response to an instruction with a LoRA fine-tuned model.")
    ap.add_argument("--prompt", default="What food do lamas eat?", help="the instruction (Alpaca style)")
    ap.add_argument("--input", default="", help="optional input (Alpaca style)")
    ap.add_argument("--lora_path", type=Path, default=Path("out/lora/alpaca/lit-llama-lora-finetuned.pth"))
    ap.add_argument("--pretrained_path", type=Path, default=Path("checkpoints/lit-llama/7B/lit-llama.pth"))
    ap.add_argument("--tokenizer_path", type=Path, default=Path("checkpoints/lit-llama/tokenizer.model"))
    ap.add_argument("--quantize", default=None, choices=[None, "llm.int8", "gptq.int4", "gptq.int8"])
    ap.add_argument("--max_new_tokens", type=int, default=100)
    ap.add_argument("--top_k", type=int, default=200)
    ap.add_argument("--temperature", type=float, default=0.8)
    ap.add_argument("--prompts_file", type=Path, default=None,
                    help="a file with one instruction per non-empty line, replacing --prompt / --input: all are "
                         "generated as one batch and each response printed in file order")
    ap.add_argument("--packed_prefill", action="store_true",
                    help="with --prompts_file: prefill all prompts as one packed batch, every weight streamed once, "
                         "instead of one prompt after the other")
    a = ap.parse_args()
    if a.prompts_file is not None:
        main_prompts_file(a.prompts_file, a.lora_path, a.pretrained_path, a.tokenizer_path, a.quantize,
                          a.max_new_tokens, a.top_k, a.temperature, a.packed_prefill)
    else:
        main(a.prompt, a.input, a.lora_path, a.pretrained_path, a.tokenizer_path, a.quantize, a.max_new_tokens,
             a.top_k, a.temperature)
