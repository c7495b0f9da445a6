"""A/B timing of `num_samples` continuations of one prompt (synthetic 7B gptq.int4, 8 samples, S = 2048, 128 new
tokens, prompts of 64 / 512 / 1024 / 1900 tokens): one process, the routes alternated inside every round so clock
and box drift cancel, warm-up before every timed span, device-synchronised timing.

Routes:
  loop     the per-sample loop of generate.py main: 8 successive generate() calls (8 prefills, batch-1 decode)
  copy     generate_samples with SHARED_PREFIX_MIN above S: one prefill, the prompt's K / V copied to the 8 rows,
           the existing per-row decode attention (llj_attention_split at S = 2048). Measured twice per round: the
           spread of all its measurements is the run-to-run noise a difference has to exceed
  shared   generate_samples with SHARED_PREFIX_MIN = 1: the same caches, decode attention by llj_attention_shared
For every (route, prompt length): `tokens_per_s` of the whole call (prefills, graph capture, 8 x 128 tokens; wall
time between device synchronisations) and `ms_per_step` of the captured decode step alone (a session of the same
route: prefill, capture, warm-up steps, then `steps` replays between synchronisations; loop: a batch-1 session,
whose step yields one token, not 8). Prints one JSON line per (route, prompt length) and one "verdict" line per
prompt length: shared beats copy when median(copy) - median(shared) ms_per_step exceeds copy's spread (max - min).

  python tools/shared_prefix_ab.py > profiles/shared_prefix_ab.json

--profile P: no timing; one shared-route session at prompt length P (prefill, capture, 40 replays) for a
`rocprofv3 --kernel-trace --stats -- python tools/shared_prefix_ab.py --profile 1024` run of its own.
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
from lit_llama import model as MD  # noqa: E402
from lit_llama.engine import DecodeSession  # noqa: E402

ROUTES = {"loop": None, "copy": 10 ** 9, "shared": 1}  # route -> SHARED_PREFIX_MIN (None: not a batch)
KW = dict(temperature=0.8, top_k=200)


def whole_call(model, route, prompt, n, new, S):
    """seconds of the whole call between device synchronisations"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if route == "loop":
        for _ in range(n):
            G.generate(model, prompt, new, max_seq_length=S, **KW)
            model.reset_cache()
    else:
        G.generate_samples(model, prompt, n, new, max_seq_length=S, **KW)
    torch.cuda.synchronize()
    model.reset_cache()
    return time.perf_counter() - t0


def session(model, route, prompt, n, new, S):
    B = 1 if route == "loop" else n
    sess = DecodeSession(model, B, S, prompt.numel() + new, seed=1234, **KW)
    if route == "loop":
        sess.prefill(prompt.view(1, -1))
    else:
        sess.prefill_shared(prompt)
    return sess


def decode_ms(model, route, prompt, n, new, S, warm, steps):
    """ms per captured decode step, and the session's work.shared_prefix"""
    sess = session(model, route, prompt, n, new, S)
    sess.decode(warm)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sess.decode(steps)
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    sp = sess.work.shared_prefix
    del sess
    model.reset_cache()
    return t / steps * 1e3, sp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="7B")
    ap.add_argument("--quantize", default="gptq.int4")
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--max-seq-length", type=int, default=2048)
    ap.add_argument("--prompt-lens", nargs="+", type=int, default=[64, 512, 1024, 1900])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warm", type=int, default=8)
    ap.add_argument("--profile", type=int, default=0, metavar="P")
    args = ap.parse_args()
    mode = None if args.quantize == "none" else args.quantize
    n, new, S = args.samples, args.new_tokens, args.max_seq_length
    steps = new - 1 - args.warm
    model = bench.build_model(args.model, mode)
    V = model.config.vocab_size
    default = MD.SHARED_PREFIX_MIN
    if args.profile:
        MD.SHARED_PREFIX_MIN = 1
        prompt = torch.randint(3, V, (args.profile,), generator=torch.Generator().manual_seed(1)).cuda()
        sess = session(model, "shared", prompt, n, new, S)
        assert sess.work.shared_prefix == args.profile
        sess.decode(40)
        torch.cuda.synchronize()
        print(f"[shared prefix ab] profiled session: P = {args.profile}, nsplit = {sess.work.shared_split}",
              file=sys.stderr)
        return
    order = ["loop", "copy", "shared", "copy"]
    res = {(r, P): {"s": [], "ms": []} for r in ROUTES for P in args.prompt_lens}
    routed = {}
    for P in args.prompt_lens:
        prompt = torch.randint(3, V, (P,), generator=torch.Generator().manual_seed(P)).cuda()
        for r in ROUTES:  # warm-up: every route once, untimed (allocator, code objects)
            MD.SHARED_PREFIX_MIN = default if ROUTES[r] is None else ROUTES[r]
            decode_ms(model, r, prompt, n, new, S, 2, 4)
        for rnd in range(args.rounds):
            for r in order:
                MD.SHARED_PREFIX_MIN = default if ROUTES[r] is None else ROUTES[r]
                torch.manual_seed(1234)
                s = whole_call(model, r, prompt, n, new, S)
                ms, sp = decode_ms(model, r, prompt, n, new, S, args.warm, steps)
                routed[(r, P)] = sp
                res[(r, P)]["s"].append(s)
                res[(r, P)]["ms"].append(ms)
                print(f"[shared prefix ab] P={P} round {rnd} {r}: {n * new / s:.1f} tok/s whole call, "
                      f"{ms:.4f} ms/step", file=sys.stderr, flush=True)
    MD.SHARED_PREFIX_MIN = default
    common = {"model": args.model, "quantize": args.quantize, "samples": n, "new_tokens": new, "max_seq_length": S,
              "rounds": args.rounds, "timed_steps": steps}
    for (r, P), v in res.items():
        s, ms = statistics.median(v["s"]), statistics.median(v["ms"])
        print(json.dumps({"route": r, "prompt_len": P, "tokens_per_s": round(n * new / s, 1),
                          "ms_per_step": round(ms, 4), "step_rows": 1 if r == "loop" else n,
                          "decode_tokens_per_s": round((1 if r == "loop" else n) / ms * 1e3, 1),
                          "shared_prefix": routed[(r, P)], "all_ms_per_step": [round(x, 4) for x in v["ms"]],
                          "all_call_s": [round(x, 4) for x in v["s"]], **common}), flush=True)
    for P in args.prompt_lens:
        c, sh = res[("copy", P)]["ms"], res[("shared", P)]["ms"]
        spread = max(c) - min(c)
        gain = statistics.median(c) - statistics.median(sh)
        print(json.dumps({"verdict": "shared beats copy" if gain > spread else "no gain beyond the spread",
                          "prompt_len": P, "copy_ms_per_step": round(statistics.median(c), 4),
                          "shared_ms_per_step": round(statistics.median(sh), 4), "gain_ms": round(gain, 4),
                          "copy_spread_ms": round(spread, 4)}), flush=True)


if __name__ == "__main__":
    main()
