"""A/B timing of unmerged LoRA decode on the bench workload (synthetic 7B gptq.int4, 16-token prompt,
S = 144, batch 1 and 8), by tools/adapter_v2_decode_ab.py's method: one process, the arms interleaved
(rounds x batch x arm) so clock and box drift cancel, bench.time_decode per measurement.

Arms:
  base       lit_llama.LLaMA (bench.build_model): no LoRA
  lora       the same model built under lora(r=8, alpha=16): c_attn = ColBlockQuantizedLinear + lora_A / lora_B,
             unmerged -- per layer one down-projection launch (llj_norm_linear, 16 columns) and the low-rank
             term in the epilogue of the QKV launch (llj_norm_qkv_rope_lora)
  lora_epi   ablation (results are wrong: t is never written): the lora arm with the down-projection launches
             left out of the step, so lora - lora_epi is what the 32 extra launches cost and lora_epi - base
             what the epilogue term costs
lora_A ~ N(0, 1 / n_embd), lora_B ~ N(0, 0.02) (their values do not change the work). Prints one JSON line
per (arm, batch), the lora lines with the differences to the other arms in ms per step and us per layer.

  python tools/lora_decode_ab.py > profiles/lora_decode_ab.json
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
from lit_llama import _hip  # noqa: E402
from lit_llama.lora import lora  # noqa: E402


def build_lora_model(name: str, mode, r: int = 8, alpha: int = 16):
    with lora(r=r, alpha=alpha, dropout=0.0, enabled=True):
        model = bench.build_model(name, mode)
    gen = torch.Generator(device="cpu").manual_seed(4321)
    with torch.no_grad():
        for blk in model.transformer.h:
            c = blk.attn.c_attn
            c.lora_A.copy_(torch.randn(c.lora_A.shape, generator=gen) / c.lora_A.shape[1] ** 0.5)
            c.lora_B.copy_(0.02 * torch.randn(c.lora_B.shape, generator=gen))
    return model.eval()


class no_down_projection:
    """While active, the down-projection launches (llj_norm_linear into at most 128 columns) are dropped."""

    def __enter__(self):
        self.orig = _hip.call

        def call(name, *a):
            if name == "llj_norm_linear" and a[9] <= 128:  # (N: the lm_head call has the vocabulary's)
                return
            return self.orig(name, *a)

        _hip.call = call

    def __exit__(self, *exc):
        _hip.call = self.orig


class nothing:
    def __enter__(self):
        pass

    def __exit__(self, *exc):
        pass


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
    lo = build_lora_model(args.model, mode)
    arms = [("base", bench.build_model(args.model, mode), nothing), ("lora", lo, nothing),
            ("lora_epi", lo, no_down_projection)]
    n_layer = lo.config.n_layer
    res = {(n, b): [] for n, _, _ in arms for b in args.batch}
    for r in range(args.rounds):
        for b in args.batch:
            for name, model, ctx in arms:
                with ctx():
                    t = bench.time_decode(model, b, 16, args.max_seq_length, 5, args.steps, 1)
                ms = t["gpu_seconds"] / args.steps * 1e3
                res[(name, b)].append(ms)
                print(f"[lora ab] round {r} {name} bs={b}: {ms:.4f} ms/step", file=sys.stderr, flush=True)
                del t
    med = {k: statistics.median(v) for k, v in res.items()}
    for (name, b), v in res.items():
        row = {"variant": name, "batch": b, "ms_per_step": round(med[(name, b)], 4), "all": [round(x, 4) for x in v],
               "tokens_per_s": round(b / med[(name, b)] * 1e3, 1), "model": args.model, "quantize": args.quantize,
               "steps": args.steps, "rounds": args.rounds, "max_seq_length": args.max_seq_length}
        if name == "lora":
            down = med[("lora", b)] - med[("lora_epi", b)]
            epi = med[("lora_epi", b)] - med[("base", b)]
            row.update(ms_ratio_lora_over_base=round(med[("lora", b)] / med[("base", b)], 4),
                       down_projection_ms_per_step=round(down, 4),
                       down_projection_us_per_layer=round(down / n_layer * 1e3, 2),
                       epilogue_ms_per_step=round(epi, 4), epilogue_us_per_layer=round(epi / n_layer * 1e3, 2))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
