"""A/B timing of the prefill of prompts of different lengths: one after the other (prefill_ragged(packed=False), the
default) against one packed batch (packed=True). Synthetic 7B gptq.int4, S = 2048, greedy.

Three prompt sets:
  spread   8 prompts of 64 .. 1024 tokens (the set of tools/ragged_decode_ab.py)
  equal    8 x 544 tokens (the same token count, equal lengths)
  short    32 x 48 tokens (a file of short instructions: the per-prompt prefill streams every weight 32 times)

Without --set this script only drives: each set runs in a child process of its own (`timeout -k 10 LIMIT python
tools/packed_prefill_ab.py --set NAME`), one after the other, and the first child that fails (or hits its limit) ends
the run with its status; nothing further is started on the GPU after it.

A child (--set NAME) is one process: both routes alternated inside every round so clock and box drift cancel,
warm-up of both routes before anything is timed, wall time between device synchronisations. Order inside a round:
loop, packed, loop -- the loop route is measured twice per round, and the spread (max - min) of all its measurements
is the run-to-run noise a difference has to exceed. Per route:
  prefill_ms     a fresh DecodeSession's prefill_ragged alone (cache allocation, the prefill launches, the choice of
                 the first tokens)
  tokens_per_s   the whole generate_prompts call (prefill, graph capture, `new` tokens per prompt)
One JSON line per (set, route) and one "verdict" line per set.

  python tools/packed_prefill_ab.py > profiles/packed_prefill_ab.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "lit-llama-ja_amd"))

SETS = {
    "spread": lambda: [round(64 + (1024 - 64) * i / 7) for i in range(8)],
    "equal": lambda: [544] * 8,
    "short": lambda: [48] * 32,
}
ORDER = ("loop", "packed", "loop")


def drive(args) -> int:
    """Each set in its own child under a time limit; stops at the first failure."""
    for name in SETS:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, str(Path(__file__).resolve()), "--set", name,
               "--model", args.model, "--quantize", args.quantize, "--new-tokens", str(args.new_tokens),
               "--max-seq-length", str(args.max_seq_length), "--rounds", str(args.rounds)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"[packed prefill ab] set {name} ended with status {rc}: stopping", file=sys.stderr, flush=True)
            return rc
    return 0


def child(args) -> None:
    import torch

    import bench
    import generate as G
    from lit_llama.engine import DecodeSession

    mode = None if args.quantize == "none" else args.quantize
    new, S = args.new_tokens, args.max_seq_length
    lens = SETS[args.set]()
    model = bench.build_model(args.model, mode)
    M = sum(lens)
    assert model.packed_prefill_support(M) is None, model.packed_prefill_support(M)
    gen = torch.Generator().manual_seed(1)
    prompts = [torch.randint(3, model.config.vocab_size, (t,), generator=gen).cuda() for t in lens]
    tmax, n = max(lens), len(lens)

    def prefill_ms(packed):
        sess = DecodeSession(model, n, S, tmax + new)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sess.prefill_ragged(prompts, packed=packed)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        assert sess.packed_prefill is packed
        del sess
        model.reset_cache()
        return t * 1e3

    def whole_call(packed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        G.generate_prompts(model, prompts, new, max_seq_length=S, top_k=1, packed_prefill=packed)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        model.reset_cache()
        return t

    for packed in (False, True):  # warm-up: both routes once, untimed (allocator, code objects)
        prefill_ms(packed)
        whole_call(packed)
    res = {r: {"ms": [], "s": []} for r in ("loop", "packed")}
    for rnd in range(args.rounds):
        for r in ORDER:
            prefill_ms(r == "packed")  # warm-up before every timed span
            ms = prefill_ms(r == "packed")
            s = whole_call(r == "packed")
            res[r]["ms"].append(ms)
            res[r]["s"].append(s)
            print(f"[packed prefill ab] {args.set} round {rnd} {r}: prefill {ms:.2f} ms, whole call {n * new / s:.1f} tok/s",
                  file=sys.stderr, flush=True)
    common = {"set": args.set, "model": args.model, "quantize": args.quantize, "prompt_lens": lens, "packed_rows": M,
              "new_tokens": new, "max_seq_length": S, "rounds": args.rounds}
    for r, v in res.items():
        print(json.dumps({"route": r, "prefill_ms": round(statistics.median(v["ms"]), 3),
                          "tokens_per_s": round(n * new / statistics.median(v["s"]), 1),
                          "all_prefill_ms": [round(x, 3) for x in v["ms"]],
                          "all_tokens_per_s": [round(n * new / x, 1) for x in v["s"]], **common}), flush=True)
    ms = {r: statistics.median(res[r]["ms"]) for r in res}
    tps = {r: [n * new / x for x in res[r]["s"]] for r in res}
    ms_spread = max(res["loop"]["ms"]) - min(res["loop"]["ms"])
    tps_spread = max(tps["loop"]) - min(tps["loop"])
    d_ms = ms["loop"] - ms["packed"]
    d_tps = statistics.median(tps["packed"]) - statistics.median(tps["loop"])
    verdict = ("packed prefill is faster" if d_ms > ms_spread else
               "packed prefill is slower" if -d_ms > ms_spread else "no difference beyond the spread")
    print(json.dumps({"set": args.set, "verdict": verdict, "loop_prefill_ms": round(ms["loop"], 3),
                      "packed_prefill_ms": round(ms["packed"], 3), "saved_ms": round(d_ms, 3),
                      "loop_spread_ms": round(ms_spread, 3), "prefill_ratio": round(ms["loop"] / ms["packed"], 3),
                      "loop_tokens_per_s": round(statistics.median(tps["loop"]), 1),
                      "packed_tokens_per_s": round(statistics.median(tps["packed"]), 1),
                      "gain_tokens_per_s": round(d_tps, 1), "loop_spread_tokens_per_s": round(tps_spread, 1)}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", choices=sorted(SETS), default=None, help="run this prompt set in this process")
    ap.add_argument("--model", default="7B")
    ap.add_argument("--quantize", default="gptq.int4")
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--max-seq-length", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds each set's process may take")
    args = ap.parse_args()
    if args.set is None:
        sys.exit(drive(args))
    child(args)


if __name__ == "__main__":
    main()
