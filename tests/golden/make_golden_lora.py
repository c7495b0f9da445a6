"""Generate tests/golden/lora.npz from the REFERENCE's LoRA model: lit_llama/model.py's LLaMA built under
lit_llama/lora.py's lora() context manager (MergedLinear on c_attn, enable_lora = [True, False, True]).

Same conditions and helpers as make_golden_adapter.py (which this script imports): runs only where the
reference is mounted; only the arrays written here are committed. Base weights are
oracle.weights.make_params(cfg, seed); per layer
    lora_A ~ N(0, 1 / n_embd),   lora_B ~ N(0, 0.12^2),   r = 8, alpha = 16 (scaling 2).
The generator asserts, on the reference alone, that the LoRA term moves the fp32 logits by more than 0.1
relative (a dropped term cannot pass) and that the reference's own bf16 models, merged and unmerged, stay
within 1.5e-2 of its fp32 logits on every prompt whose logits are stored (pick_prompt takes the first prompt
seed at which they do); both figures are recorded.

Merged = the reference's eval() (lora.py:241-278); unmerged = its train mode with dropout 0
(lora.py:310-323). The greedy prompts come from make_golden_adapter.scan (bf16 and fp32 ids of the merged
models agree on all N_NEW steps, margins above the guards on the first GUARD_STEPS steps).

Usage:  python tests/golden/make_golden_lora.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_golden as MG  # noqa: E402  (path + the `lightning` placeholder)
import make_golden_adapter as MA  # noqa: E402  (scan, margins_ok, the guards)
import lit_llama.model as rmodel  # noqa: E402  (the reference's)
from lit_llama import lora as rlora  # noqa: E402

from oracle.weights import Cfg, make_params, make_prompt  # noqa: E402

R, ALPHA = 8, 16
B_STD = 0.12
LONG_T, LONG_ROWS = 40, 4  # a prompt long enough for the prefill GEMMs; its last rows' logits are stored
# rows of layer 0's merged c_attn.weight that are stored (the file stays small): 64 of q, 16 of k (disabled:
# the pretrained rows), 64 of v
W0_ROWS = np.r_[0:64, 256:272, 512:576]


def lora_tensors(cfg: Cfg, seed: int, r: int = R) -> dict:
    rng = np.random.default_rng(seed)
    C, out = cfg.n_embd, {}
    for i in range(cfg.n_layer):
        out[f"transformer.h.{i}.attn.c_attn.lora_A"] = (rng.standard_normal((2 * r, C)) / np.sqrt(C)).astype(np.float32)
        out[f"transformer.h.{i}.attn.c_attn.lora_B"] = (rng.standard_normal((2 * C, r)) * B_STD).astype(np.float32)
    return out


def ref_lora(cfg: Cfg, params: dict, lo: dict, dtype=torch.float32, merged: bool = True, r: int = R):
    """The reference's LoRA model in eval mode (merged) or in train mode with dropout 0 (unmerged)."""
    with rlora.lora(r=r, alpha=ALPHA, dropout=0.0, enabled=True):
        m = rmodel.LLaMA(rmodel.LLaMAConfig(block_size=cfg.block_size, vocab_size=cfg.vocab_size, n_layer=cfg.n_layer,
                                            n_head=cfg.n_head, n_embd=cfg.n_embd))
    sd = {k: torch.from_numpy(np.ascontiguousarray(v).copy()) for k, v in {**params, **lo}.items()}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all("lora_" in k for k in missing), (missing, unexpected)
    m = m.to(dtype)
    return m.eval() if merged else m.train()


def rel(a, b) -> float:
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


REF_BF16_BOUND = 1.5e-2  # the reference's own bf16 models against its fp32 logits, on every stored prompt


def pick_prompt(T: int, vocab: int, first_seed: int, m32, bf16_models, rows=slice(None)):
    """The first prompt seed at which every bf16 model of the reference stays within REF_BF16_BOUND of its
    fp32 logits (the tests' bound for this package's bf16 is 2e-2): (seed, prompt, fp32 logits, worst rel)."""
    for ps in range(first_seed, first_seed + 200):
        prompt = make_prompt(T, vocab, ps)
        idx = torch.from_numpy(prompt[None]).long()
        ref = m32(idx).numpy()[0][rows]
        worst = max(rel(m(idx).float().numpy()[0][rows], ref) for m in bf16_models)
        print(f"  prompt seed {ps} (T = {T}): reference bf16 vs fp32 {worst:.3e}")
        if worst <= REF_BF16_BOUND:
            return ps, prompt, ref, worst
    raise AssertionError("no prompt seed within the reference's own bf16 bound")


@torch.no_grad()
def gen_lora():
    out = {}
    cfg = Cfg(block_size=128, n_layer=4, n_head=4, n_embd=256, vocab_size=2048)
    seed = 2501
    params = make_params(cfg, seed)
    lo = lora_tensors(cfg, seed + 1)
    out["seed"], out["r"], out["alpha"] = np.int64(seed), np.int64(R), np.int64(ALPHA)
    for k, v in lo.items():
        out["lora/" + k] = v
    m32 = ref_lora(cfg, params, lo)
    out["sd_keys"] = np.array(sorted(m32.state_dict().keys()))
    for mode in ("none", "all", "lora_only"):
        out["lora_keys_" + mode] = np.array(sorted(rlora.lora_state_dict(m32, bias=mode).keys()))
    c0 = m32.transformer.h[0].attn.c_attn
    out["lora_ind"] = c0.lora_ind.numpy()
    zp = c0.zero_pad(torch.arange(2 * cfg.n_embd * 3, dtype=torch.float32).view(2 * cfg.n_embd, 3))
    out["zero_pad_in_shape"], out["zero_pad_out"] = np.array([2 * cfg.n_embd, 3]), zp.numpy()
    models = {"fp32": m32, "bf16": ref_lora(cfg, params, lo, torch.bfloat16)}
    out["merged_w0_rows"] = W0_ROWS
    out["merged_w0_fp32"] = c0.weight.numpy()[W0_ROWS].copy()
    w16 = models["bf16"].transformer.h[0].attn.c_attn.weight.float().numpy()[W0_ROWS]
    out["merged_w0_bf16_bits"] = (w16.view(np.uint32) >> 16).astype(np.uint16)  # bf16 bit patterns

    # (the scans start a little below the first seeds that satisfy them, found from 100 and 200)
    for tag, S, first in (("", None, 1300), ("roll_", 16, 9700)):
        ps, prompt, tr = MA.scan(models, cfg.vocab_size, 12, S, first)
        out[tag + "prompt_seed"], out[tag + "prompt"] = np.int64(ps), prompt
        for dt in ("fp32", "bf16"):
            ids, L, v, i = tr[dt]
            assert np.array_equal(tr["bf16"][0], tr["fp32"][0]) and MA.margins_ok(v, MA.TOL[dt])
            out[f"{tag}{dt}_ids"], out[f"{tag}{dt}_top_v"], out[f"{tag}{dt}_top_i"] = ids, v, i

    # ---- prefill: a 12-token prompt of its own, chosen on the reference's bf16 error alone
    un16 = ref_lora(cfg, params, lo, torch.bfloat16, merged=False)
    ps, pp, ref, _ = pick_prompt(12, cfg.vocab_size, seed + 3, m32, [models["bf16"], un16])
    out["prefill_prompt_seed"], out["prefill_prompt"] = np.int64(ps), pp
    idx = torch.from_numpy(pp[None]).long()
    un32 = ref_lora(cfg, params, lo, merged=False)(idx).numpy()[0]
    out["fp32_prefill_merged"], out["fp32_prefill_unmerged_tail"] = ref, un32[-LONG_ROWS:]  # (all rows; the last 4)
    base = ref_lora(cfg, params, {})(idx).numpy()[0]  # lora_B = 0: the base model
    out["rel_lora_term"] = np.float64(rel(base, ref))
    out["rel_merged_vs_unmerged_fp32"] = np.float64(rel(un32, ref))
    out["rel_ref_bf16_merged"] = np.float64(rel(models["bf16"](idx).float().numpy()[0], ref))
    out["rel_ref_bf16_unmerged"] = np.float64(rel(un16(idx).float().numpy()[0], ref))
    print(f"the LoRA term moves the fp32 logits by {out['rel_lora_term']:.3f} relative; merged vs unmerged fp32 "
          f"{out['rel_merged_vs_unmerged_fp32']:.2e}; reference bf16 vs fp32: merged {out['rel_ref_bf16_merged']:.3e}, "
          f"unmerged {out['rel_ref_bf16_unmerged']:.3e}")
    assert out["rel_lora_term"] > 0.1  # a dropped term cannot pass
    assert out["rel_merged_vs_unmerged_fp32"] < 1e-5
    assert max(out["rel_ref_bf16_merged"], out["rel_ref_bf16_unmerged"]) <= REF_BF16_BOUND

    # ---- a prompt of LONG_T tokens (the prefill GEMM rows): the last LONG_ROWS rows of the fp32 logits
    ps, lp, tail, worst = pick_prompt(LONG_T, cfg.vocab_size, seed + 30, m32, [models["bf16"], un16],
                                      rows=slice(-LONG_ROWS, None))
    out["long_prompt_seed"], out["long_prompt"] = np.int64(ps), lp
    out["long_fp32_prefill_tail"], out["long_rel_ref_bf16"] = tail, np.float64(worst)

    # ---- head size 128 (n_head 2): fp32 prefill logits only
    cfg2 = Cfg(block_size=128, n_layer=4, n_head=2, n_embd=256, vocab_size=2048)
    p2 = make_params(cfg2, seed + 10)
    l2 = lora_tensors(cfg2, seed + 11)
    for k, v in l2.items():
        out["hs128/lora/" + k] = v
    out["hs128/seed"] = np.int64(seed + 10)
    _, pr2, ref2, worst2 = pick_prompt(12, cfg2.vocab_size, seed + 10, ref_lora(cfg2, p2, l2),
                                       [ref_lora(cfg2, p2, l2, torch.bfloat16),
                                        ref_lora(cfg2, p2, l2, torch.bfloat16, merged=False)])
    out["hs128/prompt"], out["hs128/fp32_prefill_merged"], out["hs128/rel_ref_bf16"] = pr2, ref2, np.float64(worst2)

    # ---- int4 (the reference refuses LoRA on quantized Linears): only the LoRA tensors for the 2-layer
    # model of int4_gptq.npz; the test builds its own reference from the dequantized weights
    g4 = dict(np.load(HERE / "int4_gptq.npz"))
    cfg4 = Cfg(block_size=128, n_layer=2, n_head=4, n_embd=256, vocab_size=2048)
    for k, v in lora_tensors(cfg4, seed + 21).items():
        out["int4/lora/" + k] = v
    out["int4/prompt"] = g4["prompt"]
    MG.save("lora", **out)


if __name__ == "__main__":
    gen_lora()
