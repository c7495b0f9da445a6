"""Instruction-following generation with a LLaMA-Adapter fine-tuned model on the MI355X path --
drop-in for the reference's generate/adapter.py (flags 21-31; argparse, as generate.py).

The pretrained checkpoint and the adapter checkpoint (adapter_wte / gating_factor tensors only, what
the reference's finetune/adapter.py saves) are loaded one after the other with strict=False, the
instruction is wrapped in the Alpaca prompt the adapter was trained against, and the text after
"### Response:" is printed. Decoding is generate.generate: captured-graph decode steps with the
adapter prefix term inside the decode attention launch.
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path
from typing import Optional

import torch

wd = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(wd))

from generate import generate, generate_prompts, read_prompts_file  # noqa: E402  (generate.py next to this directory)
from lit_llama import HFTokenizer, Tokenizer  # noqa: E402
from lit_llama.adapter import LLaMA  # noqa: E402
from lit_llama.checkpoint import read_checkpoint  # noqa: E402
from lit_llama.utils import EmptyInitOnDevice, llama_model_lookup  # noqa: E402

RESPONSE_MARK = "### Response:"


def generate_prompt(example: dict) -> str:
    """The Alpaca prompt of one sample {"instruction", "input"}: a preamble, the instruction, the
    input section only when there is an input, and the open response section."""
    has_input = bool(example.get("input"))
    preamble = "Below is an instruction that describes a task"
    preamble += ", paired with an input that provides further context. " if has_input else ". "
    preamble += "Write a response that appropriately completes the request."
    sections = [preamble, f"### Instruction:\n{example['instruction']}"]
    if has_input:
        sections.append(f"### Input:\n{example['input']}")
    sections.append(RESPONSE_MARK)
    return "\n\n".join(sections)


def run_prompts_file(model, tokenizer, prompts_file: Path, max_new_tokens: int, top_k: int, temperature: float,
                     packed_prefill: bool = False) -> None:
    """--prompts_file of the instruction CLIs (this one, generate/adapter_v2.py, generate/lora.py): every non-empty
    line as an instruction in the Alpaca prompt, all generated as one batch (generate.generate_prompts, which runs
    them one after the other where the model has no batched route), each response printed in file order."""
    dev = torch.device("cuda")
    enc = [tokenizer.encode(generate_prompt({"instruction": line, "input": ""}), bos=True, eos=False, device=dev)
           for line in read_prompts_file(prompts_file)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ys = generate_prompts(model, enc, max_new_tokens, temperature=temperature, top_k=top_k,
                          eos_id=tokenizer.eos_id, packed_prefill=packed_prefill)
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    model.reset_cache()
    for y in ys:
        print(tokenizer.decode(y).split(RESPONSE_MARK)[1].strip())
    tokens_generated = sum(y.size(0) - e.size(0) for y, e in zip(ys, enc))
    print(f"\n\nTime for inference of {len(enc)} instructions: {t:.02f} sec total, "
          f"{tokens_generated / t:.02f} tokens/sec", file=sys.stderr)
    print(f"Memory used: {torch.cuda.max_memory_reserved() / 1e9:.02f} GB", file=sys.stderr)


def main(prompt: str = "What food do lamas eat?", input: str = "",
         adapter_path: Path = Path("out/adapter/alpaca/lit-llama-adapter-finetuned.pth"),
         pretrained_path: Path = Path("checkpoints/lit-llama/7B/lit-llama.pth"),
         tokenizer_path: Path = Path("checkpoints/lit-llama/tokenizer.model"), quantize: Optional[str] = None,
         max_new_tokens: int = 100, top_k: int = 200, temperature: float = 0.8,
         prompts_file: Optional[Path] = None, packed_prefill: bool = False) -> None:
    """Generates a response to an instruction and an optional input (reference generate/adapter.py:21-94).
    prompts_file: one instruction per non-empty line instead of `prompt` / `input`, each wrapped in the Alpaca
    prompt, all generated as one batch (generate.generate_prompts) and each response printed in file order;
    packed_prefill: their prompts prefilled as one packed batch as well (it means nothing without prompts_file)."""
    assert adapter_path.is_file(), adapter_path
    assert pretrained_path.is_file(), pretrained_path
    assert tokenizer_path.is_file(), tokenizer_path
    if not torch.cuda.is_available():
        raise SystemExit("generate/adapter.py runs on a ROCm GPU (MI355X) only")
    print("Loading model ...", file=sys.stderr)
    t0 = time.time()
    pretrained = read_checkpoint(pretrained_path)
    adapter = read_checkpoint(adapter_path)
    name = llama_model_lookup(pretrained)
    with EmptyInitOnDevice(device=torch.device("cuda"), dtype=torch.bfloat16, quantization_mode=quantize):
        model = LLaMA.from_name(name)
    model.load_state_dict(pretrained, strict=False)  # 1. the pretrained weights
    model.load_state_dict(adapter, strict=False)     # 2. the fine-tuned adapter weights
    del pretrained, adapter
    print(f"Time to load model: {time.time() - t0:.02f} seconds.", file=sys.stderr)
    model.eval()
    tokenizer = HFTokenizer(tokenizer_path) if tokenizer_path.suffix == ".json" else Tokenizer(tokenizer_path)
    if prompts_file is not None:
        run_prompts_file(model, tokenizer, prompts_file, max_new_tokens, top_k, temperature, packed_prefill)
        return
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


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="Generates a response to an instruction with a LLaMA-Adapter model.")
    ap.add_argument("--prompt", default="What food do lamas eat?", help="the instruction (Alpaca style)")
    ap.add_argument("--input", default="", help="optional input (Alpaca style)")
    ap.add_argument("--adapter_path", type=Path, default=Path("out/adapter/alpaca/lit-llama-adapter-finetuned.pth"))
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
    main(a.prompt, a.input, a.adapter_path, a.pretrained_path, a.tokenizer_path, a.quantize, a.max_new_tokens,
         a.top_k, a.temperature, a.prompts_file, a.packed_prefill)
