"""A/B timing of LLaMA-Adapter v2 decode on the bench workload (synthetic 7B gptq.int4, 16-token prompt,
S = 144, batch 1 and 8), by tools/adapter_decode_ab.py's method: one process, the arms interleaved
(rounds x batch x arm) so clock and box drift cancel, bench.time_decode per measurement.

Arms:
  base  lit_llama.LLaMA (bench.build_model): no adapter
  v1    lit_llama.adapter.LLaMA: the prefix term inside the decode attention launch of the 30 adapted
        layers (tools/adapter_decode_ab.py's `fused` arm)
  v2    the same model + add_adapter_v2_parameters_to_linear_layers: every Linear's scale and bias in
        the epilogue of its own launch (the llj_*_v2 entry points) -- the same number of launches as v1,
        (scale, bias) vectors of 2 x 2 bytes per output column more traffic per step
The v2 vectors are adapter_scale = +-U(0.5, 1.5), adapter_bias ~ N(0, 0.02) per column (their values do
not change the work). Prints one JSON line per (arm, batch), the v2 lines with the v2 / v1 ratio.

  python tools/adapter_v2_decode_ab.py > profiles/adapter_v2_decode_ab.json
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
sys.path.insert(0, str(REPO / "tools"))

import bench  # noqa: E402
from adapter_decode_ab import build_adapter_model  # noqa: E402
from lit_llama.adapter_v2 import add_adapter_v2_parameters_to_linear_layers  # noqa: E402


def build_v2_model(name: str, mode):
    model = build_adapter_model(name, mode)
    add_adapter_v2_parameters_to_linear_layers(model)
    dt = model.act_dtype()
    gen = torch.Generator(device="cpu").manual_seed(4321)
    with torch.no_grad():
        for mod in model.modules():
            if hasattr(mod, "adapter_scale"):
                n = mod.adapter_scale.numel()
                sc = (torch.rand(n, generator=gen) + 0.5) * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1)
                mod.adapter_scale.data = sc.to(device=mod.adapter_scale.device, dtype=dt)
                mod.adapter_bias.data = (0.02 * torch.randn(n, generator=gen)).to(device=mod.adapter_bias.device, dtype=dt)
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
    arms = [("base", bench.build_model(args.model, mode)), ("v1", build_adapter_model(args.model, mode)),
            ("v2", build_v2_model(args.model, mode))]
    res = {(n, b): [] for n, _ in arms for b in args.batch}
    for r in range(args.rounds):
        for b in args.batch:
            for name, model in arms:
                t = bench.time_decode(model, b, 16, args.max_seq_length, 5, args.steps, 1)
                ms = t["gpu_seconds"] / args.steps * 1e3
                res[(name, b)].append(ms)
                print(f"[adapter v2 ab] round {r} {name} bs={b}: {ms:.4f} ms/step", file=sys.stderr, flush=True)
                del t
    med = {k: statistics.median(v) for k, v in res.items()}
    for (name, b), v in res.items():
        row = {"variant": name, "batch": b, "ms_per_step": round(med[(name, b)], 4), "all": [round(x, 4) for x in v],
               "tokens_per_s": round(b / med[(name, b)] * 1e3, 1), "model": args.model, "quantize": args.quantize,
               "steps": args.steps, "rounds": args.rounds, "max_seq_length": args.max_seq_length}
        if name == "v2":
            row["ms_ratio_v2_over_v1"] = round(med[("v2", b)] / med[("v1", b)], 4)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
