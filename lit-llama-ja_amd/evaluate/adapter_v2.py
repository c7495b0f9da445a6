"""Perplexity of a LLaMA-Adapter v2 fine-tuned model over fixed windows on the MI355X path -- drop-in for
the reference's evaluate/adapter_v2.py (flags 51-59; argparse, as evaluate/full.py).

The model is built as generate/adapter_v2.py builds it: lit_llama.adapter.LLaMA with
add_adapter_v2_parameters_to_linear_layers applied inside the quantization mode, the pretrained
checkpoint and the adapter checkpoint loaded one after the other with strict=False. The wrap in the
Alpaca prompt, the windows and the scoring are evaluate/adapter.py's (the reference's v2 script always
wraps, evaluate/adapter_v2.py:117-118; here the module constant `instruction_tuning` decides, True as
there).

--quantize gptq.int4 | gptq.int8 is this package's extension (the scale and bias run in the epilogue of
each quantized Linear's own launch); --quantize llm.int8 raises NotImplementedError before anything is
loaded, as lit_llama/adapter_v2.py does at the first forward. The text comes from files (`--text_path`).
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
from lit_llama.utils import EmptyInitOnDevice, llama_model_lookup  # noqa: E402

instruction_tuning = True  # evaluate/adapter.py's constant: see its `instruction_text`


def load_model(pretrained: dict, adapter: dict, quantize: Optional[str] = None, dtype=torch.float32):
    """The adapter v2 model of two state dicts on the GPU, in eval mode (generate/adapter_v2.py:66-74)."""
    from lit_llama.adapter import LLaMA
    from lit_llama.adapter_v2 import add_adapter_v2_parameters_to_linear_layers

    name = llama_model_lookup(pretrained)
    with EmptyInitOnDevice(device=torch.device("cuda"), dtype=dtype, quantization_mode=quantize):
        model = LLaMA.from_name(name)
        add_adapter_v2_parameters_to_linear_layers(model)
    model.load_state_dict(pretrained, strict=False)  # 1. the pretrained weights
    model.load_state_dict(adapter, strict=False)     # 2. the fine-tuned adapter weights
    return model.eval()


def main(text_path: str, *, adapter_path: Path = Path("out/adapter_v2/alpaca/lit-llama-adapter-finetuned.pth"),
         checkpoint_path: Path = Path("checkpoints/lit-llama/7B/lit-llama.pth"),
         tokenizer_path: Path = Path("checkpoints/lit-llama/tokenizer.model"), dtype: str = "float32",
         quantize: Optional[str] = None) -> dict:
    """reference evaluate/adapter_v2.py:50-158 (same flags and defaults; dtype float32 as there)."""
    if quantize == "llm.int8":
        raise NotImplementedError("adapter v2 parameters on LLM.int8 Linears are not supported (use no "
                                  "quantization, gptq.int4 or gptq.int8)")
    dt = _v1.check_dtype(dtype)
    assert adapter_path.is_file(), adapter_path
    assert checkpoint_path.is_file(), checkpoint_path
    assert tokenizer_path.is_file(), tokenizer_path
    if not torch.cuda.is_available():
        raise SystemExit("evaluate/adapter_v2.py runs on a ROCm GPU (MI355X) only")
    print("Loading model ...", file=sys.stderr)
    t0 = time.time()
    model = load_model(read_checkpoint(checkpoint_path), read_checkpoint(adapter_path), quantize, dt)
    print(f"Time to load model: {time.time() - t0:.02f} seconds.", file=sys.stderr)
    return _v1.score(model, tokenizer_path, text_path, instruction_tuning)


def cli():
    return _v1.parser("Perplexity of a LLaMA-Adapter v2 fine-tuned model (reference evaluate/adapter_v2.py).",
                      "--adapter_path", "out/adapter_v2/alpaca/lit-llama-adapter-finetuned.pth",
                      [None, "llm.int8", "gptq.int4", "gptq.int8"])


if __name__ == "__main__":
    a = cli().parse_args()
    main(a.text_path, adapter_path=a.adapter_path, checkpoint_path=a.checkpoint_path, tokenizer_path=a.tokenizer_path,
         dtype=a.dtype, quantize=a.quantize)
