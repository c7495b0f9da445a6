"""A/B timing of LLaMA-Adapter decode on the bench workload (synthetic 7B gptq.int4, 16-token prompt,
S = 144, batch 1 and 8), by tools/ab_decode.py's method: one process, the arms interleaved
(rounds x batch x arm) so clock and box drift cancel, bench.time_decode per measurement.

Arms:
  base      lit_llama.LLaMA (bench.build_model): no adapter
  fused     lit_llama.adapter.LLaMA, ADAPTER_FUSED = 1: the prefix term inside the decode attention
            launch of the 30 adapted layers (llj_attention_adapter)
  unfused   the same model, ADAPTER_FUSED = 0: llj_attention + llj_adapter_prefix_add, 30 more
            launches per step
The adapter model is bench.build_model's synthetic model built from the adapter class (same
shapes and weight distributions; adapter_wte ~ N(0, 0.02) like every embedding) with gates +-1.
Prints one JSON line per (arm, batch).

  python tools/adapter_decode_ab.py > profiles/adapter_decode_ab.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "lit-llama-ja_amd"))

import bench  # noqa: E402
import lit_llama  # noqa: E402
from lit_llama import adapter as AD  # noqa: E402


def build_adapter_model(name: str, mode):
    """bench.build_model with the adapter class in place of lit_llama.LLaMA, gates set to +-1."""
    base_cls = lit_llama.LLaMA
    lit_llama.LLaMA = AD.LLaMA
    try:
        model = bench.build_model(name, mode)
    finally:
        lit_llama.LLaMA = base_cls
    assert isinstance(model, AD.LLaMA)
    with torch.no_grad():
        for blk in model.transformer.h[model.config.adapter_start_layer:]:
            g = blk.attn.gating_factor
            g.copy_(torch.where(torch.arange(g.numel(), device=g.device) % 2 == 0, 1.0, -1.0).view_as(g))
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", nargs="+", type=int, default=[1, 8])
    ap.add_argument("--model", default="7B")
    ap.add_argument("--quantize", default="gptq.int4")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-seq-length", type=int, default=144)
    args = ap.parse_args()
    mode = None if args.quantize == "none" else args.quantize
    base = bench.build_model(args.model, mode)
    adp = build_adapter_model(args.model, mode)
    arms = [("base", base, None), ("fused", adp, 1), ("unfused", adp, 0)]
    default = AD.ADAPTER_FUSED
    res = {(n, b): [] for n, _, _ in arms for b in args.batch}
    for r in range(args.rounds):
        for b in args.batch:
            for name, model, fused in arms:
                AD.ADAPTER_FUSED = default if fused is None else fused
                t = bench.time_decode(model, b, 16, args.max_seq_length, 5, args.steps, 1)
                ms = t["gpu_seconds"] / args.steps * 1e3
                res[(name, b)].append(ms)
                print(f"[adapter ab] round {r} {name} bs={b}: {ms:.4f} ms/step", file=sys.stderr, flush=True)
                del t
    AD.ADAPTER_FUSED = default
    for (name, b), v in res.items():
        med = statistics.median(v)
        print(json.dumps({"variant": name, "batch": b, "ms_per_step": round(med, 4), "all": [round(x, 4) for x in v],
                          "tokens_per_s": round(b / med * 1e3, 1), "model": args.model, "quantize": args.quantize,
                          "steps": args.steps, "rounds": args.rounds, "max_seq_length": args.max_seq_length}),
              flush=True)


if __name__ == "__main__":
    main()
