"""A/B timing of continuing 8 prompts of different lengths (synthetic 7B gptq.int4, S = 2048, 128 new tokens each,
greedy): one process, the routes alternated inside every round so clock and box drift cancel, warm-up before every
timed span, device-synchronised timing.

Routes:
  loop          the 8 prompts (lengths spread over 64 .. 1024) through generate() one after the other: 8 prefills,
                batch-1 decode. What a file of prompts cost before generate_prompts existed
  ragged        the same prompts through generate_prompts: 8 one-row prefills, then one decode step for all rows
                (c_attn's plain store + llj_attention_ragged). Measured twice per round: the spread of all its
                measurements is the run-to-run noise a difference has to exceed
  equal-fused   8 prompts of one length (the mean of the spread) through generate_batch: one 8-row prefill, the
                fused c_attn epilogue and the existing decode attention
  equal-ragged  the same 8 prompts through generate_prompts; equal-ragged - equal-fused in ms_per_step is what the
                un-fused c_attn epilogue and the new attention cost against the fused route
For every route: `tokens_per_s` of the whole call (prefills, graph capture, 8 x 128 tokens; wall time between device
synchronisations) and `ms_per_step` of the captured decode step alone (a session of the same route: prefill,
capture, warm-up steps, then `steps` replays between synchronisations; loop: a batch-1 session on the prompt of
middle length, whose step yields one token, not 8). Prints one JSON line per route and two "verdict" lines: ragged
beats loop when median(ragged) - median(loop) tokens_per_s exceeds ragged's spread (max - min); the cost line gives
equal-ragged - equal-fused.

  python tools/ragged_decode_ab.py > profiles/ragged_decode_ab.json
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
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "lit-llama-ja_amd"))

import bench  # noqa: E402
import generate as G  # noqa: E402
from lit_llama.engine import DecodeSession  # noqa: E402

ROUTES = ("loop", "ragged", "equal-fused", "equal-ragged")
ORDER = ("loop", "ragged", "equal-fused", "equal-ragged", "ragged")


def whole_call(model, route, prompts, new, S):
    """seconds of the whole call between device synchronisations"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if route == "loop":
        for p in prompts:
            G.generate(model, p, new, max_seq_length=S, top_k=1)
            model.reset_cache()
    elif route == "equal-fused":
        G.generate_batch(model, torch.stack(prompts), new, max_seq_length=S)
    else:
        G.generate_prompts(model, prompts, new, max_seq_length=S, top_k=1)
    torch.cuda.synchronize()
    model.reset_cache()
    return time.perf_counter() - t0


def session(model, route, prompts, new, S):
    tmax = max(p.numel() for p in prompts)
    if route == "loop":
        mid = sorted(prompts, key=lambda p: p.numel())[len(prompts) // 2]
        sess = DecodeSession(model, 1, S, mid.numel() + new)
        sess.prefill(mid.view(1, -1))
    elif route == "equal-fused":
        sess = DecodeSession(model, len(prompts), S, tmax + new)
        sess.prefill(torch.stack(prompts))
    else:
        sess = DecodeSession(model, len(prompts), S, tmax + new)
        sess.prefill_ragged(prompts)
    return sess


def decode_ms(model, route, prompts, new, S, warm, steps):
    """ms per captured decode step, and whether the session took the ragged route"""
    sess = session(model, route, prompts, new, S)
    sess.decode(warm)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sess.decode(steps)
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    ragged = bool(sess.work.ragged)
    del sess
    model.reset_cache()
    return t / steps * 1e3, ragged


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="7B")
    ap.add_argument("--quantize", default="gptq.int4")
    ap.add_argument("--prompts", type=int, default=8)
    ap.add_argument("--min-len", type=int, default=64)
    ap.add_argument("--max-len", type=int, default=1024)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--max-seq-length", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warm", type=int, default=8)
    args = ap.parse_args()
    mode = None if args.quantize == "none" else args.quantize
    n, new, S = args.prompts, args.new_tokens, args.max_seq_length
    steps = new - 1 - args.warm
    model = bench.build_model(args.model, mode)
    assert model.ragged_support() is None, model.ragged_support()
    V = model.config.vocab_size
    lens = [round(args.min_len + (args.max_len - args.min_len) * i / max(1, n - 1)) for i in range(n)]
    eq = round(sum(lens) / n)
    gen = torch.Generator().manual_seed(1)
    spread_prompts = [torch.randint(3, V, (t,), generator=gen).cuda() for t in lens]
    equal_prompts = [torch.randint(3, V, (eq,), generator=gen).cuda() for _ in range(n)]
    inputs = {r: equal_prompts if r.startswith("equal") else spread_prompts for r in ROUTES}
    for r in ROUTES:  # warm-up: every route once, untimed (allocator, code objects)
        decode_ms(model, r, inputs[r], new, S, 2, 4)
    res = {r: {"s": [], "ms": []} for r in ROUTES}
    routed = {}
    for rnd in range(args.rounds):
        for r in ORDER:
            s = whole_call(model, r, inputs[r], new, S)
            ms, routed[r] = decode_ms(model, r, inputs[r], new, S, args.warm, steps)
            res[r]["s"].append(s)
            res[r]["ms"].append(ms)
            print(f"[ragged decode ab] round {rnd} {r}: {n * new / s:.1f} tok/s whole call, {ms:.4f} ms/step",
                  file=sys.stderr, flush=True)
    common = {"model": args.model, "quantize": args.quantize, "prompts": n, "new_tokens": new, "max_seq_length": S,
              "rounds": args.rounds, "timed_steps": steps}
    for r, v in res.items():
        s, ms = statistics.median(v["s"]), statistics.median(v["ms"])
        rows = 1 if r == "loop" else n
        print(json.dumps({"route": r, "prompt_lens": [eq] * n if r.startswith("equal") else lens,
                          "tokens_per_s": round(n * new / s, 1), "ms_per_step": round(ms, 4), "step_rows": rows,
                          "decode_tokens_per_s": round(rows / ms * 1e3, 1), "ragged_session": routed[r],
                          "all_tokens_per_s": [round(n * new / x, 1) for x in v["s"]],
                          "all_ms_per_step": [round(x, 4) for x in v["ms"]], **common}), flush=True)
    tps = {r: [n * new / x for x in res[r]["s"]] for r in ROUTES}
    spread = max(tps["ragged"]) - min(tps["ragged"])
    gain = statistics.median(tps["ragged"]) - statistics.median(tps["loop"])
    print(json.dumps({"verdict": "ragged beats loop" if gain > spread else "no gain beyond the spread",
                      "loop_tokens_per_s": round(statistics.median(tps["loop"]), 1),
                      "ragged_tokens_per_s": round(statistics.median(tps["ragged"]), 1),
                      "gain_tokens_per_s": round(gain, 1), "ragged_spread_tokens_per_s": round(spread, 1),
                      "ratio": round(statistics.median(tps["ragged"]) / statistics.median(tps["loop"]), 3)}), flush=True)
    ms_spread = max(res["ragged"]["ms"]) - min(res["ragged"]["ms"])
    cost = statistics.median(res["equal-ragged"]["ms"]) - statistics.median(res["equal-fused"]["ms"])
    print(json.dumps({"verdict": "cost of the un-fused c_attn epilogue and the ragged attention at equal lengths",
                      "equal_fused_ms_per_step": round(statistics.median(res["equal-fused"]["ms"]), 4),
                      "equal_ragged_ms_per_step": round(statistics.median(res["equal-ragged"]["ms"]), 4),
                      "cost_ms_per_step": round(cost, 4), "ragged_spread_ms_per_step": round(ms_spread, 4)}), flush=True)


if __name__ == "__main__":
    main()
