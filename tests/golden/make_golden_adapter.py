"""Generate tests/golden/adapter.npz from the REFERENCE's LLaMA-Adapter model
(lit_llama/adapter.py, scripts/prepare_alpaca.py:generate_prompt).

Same conditions as make_golden.py (whose module set-up -- sys.path, the `lightning` placeholder --
this script reuses by importing it): runs only where the reference is mounted; only the arrays
written here are committed. Base weights are oracle.weights.make_params(cfg, seed); the adapter
tensors (adapter_wte ~ N(0, 1), gating_factor = +-U(0.5, 1.5) per head: non-zero gates, so the
prefix term carries a large part of every adapted layer's attention output) are stored in the file.

The greedy prompts are found by a seed scan that looks at the reference alone: the bf16 and fp32
ids must agree on all N_NEW steps and the first GUARD_STEPS steps of each trace must have a
top-1 / top-2 margin above that dtype's guard (the tolerances of tests/test_model_gpu.py), so a
margin-guarded comparison cannot legitimately stop before GUARD_STEPS.

Usage:  python tests/golden/make_golden_adapter.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_golden as MG  # noqa: E402  (path + placeholder set-up, ref_model-style helpers)
from lit_llama import adapter as radp  # noqa: E402  (the reference's)
from lit_llama.utils import quantization as rquantization  # noqa: E402
from scripts.prepare_alpaca import generate_prompt  # noqa: E402

from oracle.weights import Cfg, make_params, make_prompt  # noqa: E402

N_NEW, GUARD_STEPS = 24, 20
TOL = {"bf16": 0.15, "fp32": 0.25}
AT, START = 10, 2


def adapter_tensors(cfg: Cfg, start: int, aT: int, seed: int, scalar_gate_layer: int | None = None) -> dict:
    rng = np.random.default_rng(seed)
    out = {}
    for i in range(start, cfg.n_layer):
        p = f"transformer.h.{i}.attn."
        out[p + "adapter_wte.weight"] = rng.standard_normal((aT, cfg.n_embd), dtype=np.float32)
        g = (rng.uniform(0.5, 1.5, cfg.n_head) * rng.choice([-1.0, 1.0], cfg.n_head)).astype(np.float32)
        out[p + "gating_factor"] = g.reshape(1, cfg.n_head, 1, 1)
        if i == scalar_gate_layer:  # a checkpoint from before the per-head gate: one value
            out[p + "gating_factor"] = g[:1].copy()
    return out


def ref_adapter(cfg: Cfg, params: dict, adp: dict, start: int, aT: int, dtype=torch.float32, sd_extra=None, mode=None):
    rc = radp.LLaMAConfig(block_size=cfg.block_size, vocab_size=cfg.vocab_size, n_layer=cfg.n_layer, n_head=cfg.n_head,
                          n_embd=cfg.n_embd, adapter_prompt_length=aT, adapter_start_layer=start)
    with rquantization(mode):
        m = radp.LLaMA(rc)
    sd = {k: torch.from_numpy(np.ascontiguousarray(v).copy()) for k, v in {**params, **adp}.items()}
    if sd_extra is not None:
        for k in list(sd):
            if k.endswith(".weight") and k[:-7] + ".quant_weight" in sd_extra:
                del sd[k]
        sd.update({k: torch.from_numpy(np.ascontiguousarray(v).copy()) for k, v in sd_extra.items()})
    m.load_state_dict(sd)
    return m.to(dtype).eval()


def margins_ok(top_v, tol):
    m = top_v[:GUARD_STEPS, 0] - top_v[:GUARD_STEPS, 1]
    return bool((m > tol).all())


def scan(models, vocab, T, max_seq_length, first_seed):
    """The first prompt seed at which the reference's two precisions agree with guarded margins."""
    for ps in range(first_seed, first_seed + 20000):
        prompt = make_prompt(T, vocab, ps)
        tr = {}
        for tag in ("fp32", "bf16"):  # most seeds fail the fp32 margins: the bf16 trace only after them
            tr[tag] = MG.greedy_trace(models[tag], prompt, N_NEW, max_seq_length=max_seq_length)
            if not margins_ok(tr[tag][2], TOL[tag]):
                break
        else:
            same = np.array_equal(tr["bf16"][0], tr["fp32"][0])
            print(f"  prompt seed {ps}: margins guarded in both precisions, ids agree {same}")
            if same:
                return ps, prompt, tr
    raise AssertionError("no prompt seed satisfies the reference-only condition")


@torch.no_grad()
def gen_adapter():
    out = {}
    cfg = Cfg(block_size=128, n_layer=4, n_head=4, n_embd=256, vocab_size=2048)
    seed = 2303
    params = make_params(cfg, seed)
    adp = adapter_tensors(cfg, START, AT, seed + 1)
    out["seed"] = np.int64(seed)
    out["aT"], out["start"] = np.int64(AT), np.int64(START)
    for k, v in adp.items():
        out["adp/" + k] = v
    m32 = ref_adapter(cfg, params, adp, START, AT)
    out["sd_keys"] = np.array(sorted(m32.state_dict().keys()))
    models = {"fp32": m32, "bf16": ref_adapter(cfg, params, adp, START, AT, torch.bfloat16)}

    # ---- prefill: fp32 no-cache logits of a 12-token prompt; how much the gates matter, and the
    # reference's own bf16 distance (recorded for the record, not asserted by the tests)
    for tag, S, first in (("", None, 100), ("roll_", 16, 200)):
        ps, prompt, tr = scan(models, cfg.vocab_size, 12, S, first)
        out[tag + "prompt_seed"], out[tag + "prompt"] = np.int64(ps), prompt
        for dt in ("fp32", "bf16"):
            ids, L, v, i = tr[dt]
            assert np.array_equal(tr["bf16"][0], tr["fp32"][0]) and margins_ok(v, TOL[dt])
            out[f"{tag}{dt}_ids"], out[f"{tag}{dt}_top_v"], out[f"{tag}{dt}_top_i"] = ids, v, i
    idx = torch.from_numpy(out["prompt"][None]).long()
    ref = m32(idx).numpy()[0]
    out["fp32_prefill_nocache"] = ref
    zero = {k: (np.zeros_like(v) if k.endswith("gating_factor") else v) for k, v in adp.items()}
    z = ref_adapter(cfg, params, zero, START, AT)(idx).numpy()[0]
    b = models["bf16"](idx).float().numpy()[0]
    out["rel_zero_gates"] = np.float64(np.linalg.norm(z - ref) / np.linalg.norm(ref))
    out["rel_ref_bf16"] = np.float64(np.linalg.norm(b - ref) / np.linalg.norm(ref))
    print(f"zeroed gates move the fp32 logits by {out['rel_zero_gates']:.3f} relative; "
          f"reference bf16 vs fp32 {out['rel_ref_bf16']:.3e}")
    assert out["rel_zero_gates"] > 0.1  # the gates carry a large share: a dropped prefix term cannot pass

    # ---- head size 128 (n_head 2): fp32 prefill logits only
    cfg2 = Cfg(block_size=128, n_layer=4, n_head=2, n_embd=256, vocab_size=2048)
    p2 = make_params(cfg2, seed + 10)
    a2 = adapter_tensors(cfg2, START, AT, seed + 11)
    for k, v in a2.items():
        out["hs128/adp/" + k] = v
    out["hs128/seed"] = np.int64(seed + 10)
    pr2 = make_prompt(12, cfg2.vocab_size, seed + 10)
    out["hs128/prompt"] = pr2
    out["hs128/fp32_prefill_nocache"] = ref_adapter(cfg2, p2, a2, START, AT)(torch.from_numpy(pr2[None]).long()).numpy()[0]

    # ---- legacy gating: layer 2's gate as a single value (reference adapter.py:174-188)
    al = adapter_tensors(cfg, START, AT, seed + 1, scalar_gate_layer=2)
    for k, v in al.items():
        out["legacy/adp/" + k] = v
    out["legacy/fp32_prefill_nocache"] = ref_adapter(cfg, params, al, START, AT)(idx).numpy()[0]

    # ---- int4: the packed weights of int4_gptq.npz (2 layers) + adapter tensors from layer 1 on,
    # through the reference's quantization("gptq.int4") forward
    g4 = dict(np.load(HERE / "int4_gptq.npz"))
    cfg4 = Cfg(block_size=128, n_layer=2, n_head=4, n_embd=256, vocab_size=2048)
    p4 = make_params(cfg4, int(g4["seed"]))
    packed = {k[3:]: v for k, v in g4.items() if k.startswith("sd/")}
    a4 = adapter_tensors(cfg4, 1, AT, seed + 21)
    for k, v in a4.items():
        out["int4/adp/" + k] = v
    out["int4/start"] = np.int64(1)
    out["int4/prompt"] = g4["prompt"]
    m4 = ref_adapter(cfg4, p4, a4, 1, AT, sd_extra=packed, mode="gptq.int4")
    ids, L, v, i = MG.greedy_trace(m4, g4["prompt"], N_NEW)
    out.update({"int4/fp32_ids": ids, "int4/fp32_top_v": v, "int4/fp32_top_i": i, "int4/fp32_logits_step0": L[0],
                "int4/fp32_logits_step5": L[5]})
    ids, L, v, i = MG.greedy_trace(m4.to(torch.bfloat16), g4["prompt"], N_NEW)
    out.update({"int4/bf16_ids": ids, "int4/bf16_top_v": v, "int4/bf16_top_i": i})

    # ---- the Alpaca prompt contract of the adapter checkpoints (scripts/prepare_alpaca.py)
    s1 = {"instruction": "Translate the sentence to French.", "input": "The llama eats grass."}
    s2 = {"instruction": "What food do lamas eat?", "input": ""}
    out["alpaca_instruction"] = np.array([s1["instruction"], s2["instruction"]])
    out["alpaca_input"] = np.array([s1["input"], s2["input"]])
    out["alpaca_prompt"] = np.array([generate_prompt(s1), generate_prompt(s2)])
    MG.save("adapter", **out)


if __name__ == "__main__":
    gen_adapter()
