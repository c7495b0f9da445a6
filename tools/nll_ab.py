"""A/B timing of the scoring step of evaluate/*.py at the 7B window's shape: (2047, 32000) bf16 logits
(synthetic, N(0, 4^2)) scored against 2047 targets, by tools/ab_decode.py's method: one process, the arms
interleaved round by round so clock and box drift cancel, medians over the rounds after a warm-up.

Arms (each timed over `--iters` windows per round, host clock between two device synchronisations):
  torch   the expression evaluate/full.py used before: F.cross_entropy(logits.float(), targets,
          reduction="sum") and .item() after every window
  hip     llj_nll with a device (sum, count) accumulator (LLaMA.window_nll's call), read back once per round
Also reported per arm: torch.cuda.max_memory_allocated above the resident logits and targets, and for the
hip arm the achieved read rate of the 131 MB of logits (the kernel's floor is one read of them).
Prints one JSON line per arm.

  python tools/nll_ab.py > profiles/nll_ab.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "lit-llama-ja_amd"))

from lit_llama import _hip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2047)
    ap.add_argument("--vocab", type=int, default=32000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    M, V = args.rows, args.vocab
    gen = torch.Generator(device="cuda").manual_seed(0)
    logits = (4.0 * torch.randn(M, V, device="cuda", generator=gen)).to(torch.bfloat16)
    tgt = torch.randint(0, V, (M,), device="cuda", generator=gen)
    tgt32 = tgt.to(torch.int32)
    row_nll = torch.empty(M, dtype=torch.float32, device="cuda")
    total = torch.zeros(2, dtype=torch.float64, device="cuda")
    st = _hip.stream()

    def arm_torch():
        s = 0.0
        for _ in range(args.iters):
            s += torch.nn.functional.cross_entropy(logits.float(), tgt, reduction="sum").item()
        return s

    def arm_hip():
        total.zero_()
        for _ in range(args.iters):
            _hip.call("llj_nll", logits.data_ptr(), V, M, V, tgt32.data_ptr(), row_nll.data_ptr(), total.data_ptr(), st)
        return total.tolist()[0]

    arms = {"torch": arm_torch, "hip": arm_hip}
    ms = {n: [] for n in arms}
    peak, value = {}, {}
    resident = torch.cuda.memory_allocated()
    for r in range(args.warmup + args.rounds):
        for name, f in arms.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            value[name] = f()
            torch.cuda.synchronize()
            t = (time.perf_counter() - t0) / args.iters * 1e3
            peak[name] = max(peak.get(name, 0), torch.cuda.max_memory_allocated() - resident)
            if r >= args.warmup:
                ms[name].append(t)
            print(f"[nll ab] round {r} {name}: {t:.4f} ms/window", file=sys.stderr, flush=True)
    rel = abs(value["hip"] - value["torch"]) / abs(value["torch"])
    for name in arms:
        med = statistics.median(ms[name])
        rec = {"arm": name, "ms_per_window": round(med, 4), "all": [round(x, 4) for x in ms[name]],
               "peak_extra_bytes": int(peak[name]), "rows": M, "vocab": V, "iters": args.iters, "rounds": args.rounds,
               "summed_nll": value[name], "rel_diff_of_sums": rel}
        if name == "hip":
            rec["logits_read_GBps"] = round(M * V * 2 / (med * 1e-3) / 1e9, 1)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
