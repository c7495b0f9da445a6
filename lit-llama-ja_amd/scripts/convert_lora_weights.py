"""Merge a LoRA checkpoint into the pretrained weights and save a plain LLaMA checkpoint -- drop-in for the
reference's scripts/convert_lora_weights.py (flags 33-38; argparse, as generate.py).

The LoRA rank is read from `transformer.h.0.attn.c_attn.lora_B`; the model is built under
lora(r=rank, alpha=16, dropout=0.05), both checkpoints are loaded with strict=False, eval() merges
(llj_lora_merge on the GPU, the reference's rounding points in `dtype`), the lora_ keys are dropped and
the state dict is saved next to the LoRA checkpoint as <stem>-lora-merged-weights.pth. The merge runs
on the GPU: --accelerator is accepted for the reference's command lines and must be auto, cuda or gpu.
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path
from typing import Optional

import torch
import torch.nn as nn

wd = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(wd))

from lit_llama import LLaMA  # noqa: E402
from lit_llama.checkpoint import read_checkpoint  # noqa: E402
from lit_llama.lora import lora  # noqa: E402
from lit_llama.utils import EmptyInitOnDevice, llama_model_lookup  # noqa: E402


def del_lora_state_dict(model: nn.Module) -> dict:
    """The model's state dict without the lora_ entries (reference convert_lora_weights.py:18-23)."""
    return {k: v for k, v in model.state_dict().items() if "lora_" not in k}


def lora_model_lookup(checkpoint: dict) -> int:
    """The LoRA rank of a LoRA checkpoint (reference convert_lora_weights.py:26-30)."""
    return checkpoint["transformer.h.0.attn.c_attn.lora_B"].shape[1]


def main(accelerator: str = "auto", lora_path: Optional[Path] = None, checkpoint_path: Optional[Path] = None,
         dtype: str = "bfloat16") -> Path:
    """Merges LoRA weights into the base model (reference convert_lora_weights.py:33-89); returns the path
    of the saved checkpoint."""
    lora_path = Path(lora_path) if lora_path else Path("out/lora/alpaca/lit-llama-lora-finetuned.pth")
    checkpoint_path = Path(checkpoint_path) if checkpoint_path else Path("./checkpoints/lit-llama/7B/lit-llama.pth")
    assert lora_path.is_file(), lora_path
    assert checkpoint_path.is_file(), checkpoint_path
    if accelerator not in ("auto", "cuda", "gpu"):
        raise ValueError(f"accelerator {accelerator!r}: the merge runs on a ROCm GPU (auto, cuda or gpu)")
    dt = getattr(torch, dtype, None)
    if not isinstance(dt, torch.dtype):
        raise ValueError(f"{dtype} is not a valid dtype.")
    if dt not in (torch.bfloat16, torch.float32):
        raise ValueError(f"{dtype}: the merge computes in bfloat16 or float32")
    if not torch.cuda.is_available():
        raise SystemExit("scripts/convert_lora_weights.py runs on a ROCm GPU (MI355X) only")
    print("Loading model ...", file=sys.stderr)
    t0 = time.time()
    pretrained, lora_checkpoint = read_checkpoint(checkpoint_path), read_checkpoint(lora_path)
    name = llama_model_lookup(pretrained)
    rank = lora_model_lookup(lora_checkpoint)
    with EmptyInitOnDevice(device=torch.device("cuda"), dtype=dt), lora(r=rank, alpha=16, dropout=0.05, enabled=True):
        model = LLaMA.from_name(name)
    model.load_state_dict(pretrained, strict=False)       # 1. the pretrained weights
    model.load_state_dict(lora_checkpoint, strict=False)  # 2. the fine-tuned LoRA weights
    print(f"Time to load model: {time.time() - t0:.02f} seconds.", file=sys.stderr)
    model.eval()
    torch.cuda.synchronize()
    base_model_dict = {k: v.cpu() for k, v in del_lora_state_dict(model).items()}
    save_path = lora_path.with_name(f"{lora_path.stem}-lora-merged-weights{lora_path.suffix}")
    print("Saving LoRA to base model weights ...")
    torch.save(base_model_dict, save_path)
    print(f"Model saved at {save_path}")
    return save_path


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="Merges LoRA weights into the base model.")
    ap.add_argument("--accelerator", default="auto")
    ap.add_argument("--lora_path", type=Path, default=None)
    ap.add_argument("--checkpoint_path", type=Path, default=None)
    ap.add_argument("--dtype", default="bfloat16")
    a = ap.parse_args()
    main(a.accelerator, a.lora_path, a.checkpoint_path, a.dtype)
