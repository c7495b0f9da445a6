"""Generate tests/golden/eval_finetuned.npz: the REFERENCE's perplexity loop (evaluate/adapter.py:128-144,
evaluate/adapter_v2.py, evaluate/lora.py) on its adapter v1, adapter v2 and LoRA (merged) models.

Same conditions and helpers as make_golden_adapter.py / make_golden_adapter_v2.py / make_golden_lora.py
(which this script imports): runs only where the reference is mounted; only the arrays written here are
committed. The three models are those of adapter.npz, adapter_v2.npz and lora.npz -- the same Cfg, the base
weights oracle.weights.make_params(cfg, that fixture's seed), the fine-tune tensors read from that
fixture -- so this file stores no weights.

A stream of 300 tokens per variant, cut at block_size = 128 into windows of 128, 128 and 44 tokens;
logits[:-1] of every window score inp[1:] with a summed cross entropy, in fp32. Every window of a stream is
make_prompt(12, vocab, token_seed + window) followed by the greedy continuation of the reference's own fp32
fine-tuned model (make_golden.greedy_trace), so the text is one the fine-tuned model finds likely and the base
model does not. (Uniformly random tokens cannot serve: on make_prompt(300, vocab, seed) both models score about
log(vocab) per token and the v1 prefix and the LoRA term move a window's summed NLL by at most 9e-3 relative
over 200 seeds -- below the tests' bf16 bound, so a model without the term would pass.)
Stored per variant (v1, v2, lora): the tokens, the per-window summed NLL, the token count and the perplexity,
the same for the base model (the fine-tune tensors left out), and two figures the generator asserts on the
reference alone, scanning token seeds until both hold for every variant (as make_golden_lora.pick_prompt):
  * rel_finetune_min: the fine-tune moves every window's summed NLL by at least MOVE_MIN = 5e-2 relative to
    the base model's -- 5 x the tests' bf16 bound, so a model that drops the prefix, the affine or the LoRA
    term cannot pass;
  * rel_ref_bf16_max: the reference's own bf16 run of the same loop stays within REF_BF16_BOUND = 5e-3
    relative of its fp32 per-window NLL -- half the bound the tests give this package's bf16 models.
Also stored: the string scripts/prepare_alpaca.generate_prompt returns for {"instruction": "TEXT",
"input": input} with the Python builtin `input`, which is what the reference's evaluate scripts pass
(evaluate/adapter.py:118) -- recorded data that pins the instruction wrap.

Usage:  python tests/golden/make_golden_eval_finetuned.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_golden as MG  # noqa: E402  (path + the `lightning` placeholder, ref_model, save)
import make_golden_adapter as MA  # noqa: E402
import make_golden_adapter_v2 as MA2  # noqa: E402
import make_golden_lora as ML  # noqa: E402
from scripts.prepare_alpaca import generate_prompt  # noqa: E402  (the reference's)

from oracle.weights import Cfg, make_params, make_prompt  # noqa: E402

CFG = Cfg(block_size=128, n_layer=4, n_head=4, n_embd=256, vocab_size=2048)
N_TOKENS = 300
MOVE_MIN = 5e-2
REF_BF16_BOUND = 5e-3
FIRST_TOKEN_SEED = 2601


@torch.inference_mode()
def ppl_loop(model, tokens: np.ndarray, block_size: int):
    """reference evaluate/adapter.py:128-144 with its block_size cut at the model's: (per-window summed
    NLL, tokens scored)."""
    enc = torch.from_numpy(tokens)
    per, toks = [], 0
    for i in range(0, enc.shape[1], block_size):
        inp = enc[:, i:i + block_size]
        logits = model(inp)[0]
        nll = torch.nn.functional.cross_entropy(logits[:-1], inp[0, 1:].to(dtype=torch.long), reduction="sum")
        toks += inp.size(1) - 1
        per.append(float(nll.item()))
    return np.array(per, np.float64), toks


def _prefixed(g, prefix):
    return {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}


def variants():
    """tag -> (fp32 fine-tuned, bf16 fine-tuned, fp32 base) reference models of the existing fixtures."""
    out = {}
    g = dict(np.load(HERE / "adapter.npz"))
    p, adp = make_params(CFG, int(g["seed"])), _prefixed(g, "adp/")
    start, aT = int(g["start"]), int(g["aT"])
    out["v1"] = (MA.ref_adapter(CFG, p, adp, start, aT), MA.ref_adapter(CFG, p, adp, start, aT, torch.bfloat16),
                 MG.ref_model(CFG, p))
    g = dict(np.load(HERE / "adapter_v2.npz"))
    p, adp = make_params(CFG, int(g["seed"])), _prefixed(g, "adp/")
    out["v2"] = (MA2.ref_v2(CFG, p, adp), MA2.ref_v2(CFG, p, adp, torch.bfloat16), MG.ref_model(CFG, p))
    g = dict(np.load(HERE / "lora.npz"))
    p, lo = make_params(CFG, int(g["seed"])), _prefixed(g, "lora/")
    out["lora"] = (ML.ref_lora(CFG, p, lo), ML.ref_lora(CFG, p, lo, torch.bfloat16), MG.ref_model(CFG, p))
    return out


WINDOWS = (128, 128, 44)
N_RANDOM = 12  # random tokens at the head of every window; the rest is the fine-tuned model's greedy continuation


def stream(m32, token_seed: int) -> np.ndarray:
    parts = []
    for w, n in enumerate(WINDOWS):
        head = make_prompt(N_RANDOM, CFG.vocab_size, token_seed + w)
        ids = MG.greedy_trace(m32, head, n - N_RANDOM)[0]
        assert ids.shape == (n,) and np.array_equal(ids[:N_RANDOM], head)
        parts.append(ids)
    return np.concatenate(parts)[None].astype(np.int64)


def measure(models, token_seed):
    res = {}
    for tag, (m32, m16, base) in models.items():
        tokens = stream(m32, token_seed)
        assert tokens.shape == (1, N_TOKENS)
        nll, toks = ppl_loop(m32, tokens, CFG.block_size)
        nll16, _ = ppl_loop(m16, tokens, CFG.block_size)
        nllb, toksb = ppl_loop(base, tokens, CFG.block_size)
        res[tag] = dict(tokens=tokens, nll=nll, toks=toks, nll16=nll16, nllb=nllb, toksb=toksb,
                        move=float((np.abs(nll - nllb) / nllb).min()), bf16=float((np.abs(nll16 - nll) / nll).max()))
    return res


def gen_eval_finetuned():
    models = variants()
    for ts in range(FIRST_TOKEN_SEED, FIRST_TOKEN_SEED + 200):
        res = measure(models, ts)
        print(f"  token seed {ts}: " + "; ".join(f"{t}: fine-tune moves the window NLL by >= {r['move']:.3f}, "
                                               f"reference bf16 vs fp32 <= {r['bf16']:.2e}" for t, r in res.items()))
        if all(r["move"] >= MOVE_MIN and r["bf16"] <= REF_BF16_BOUND for r in res.values()):
            break
    else:
        raise AssertionError("no token seed satisfies the reference-only conditions")
    out = {"token_seed": np.int64(ts), "block_size": np.int64(CFG.block_size),
           "move_min": np.float64(MOVE_MIN), "ref_bf16_bound": np.float64(REF_BF16_BOUND)}
    for tag, r in res.items():
        assert r["move"] >= MOVE_MIN and r["bf16"] <= REF_BF16_BOUND
        assert [len(r["nll"]), r["toks"]] == [3, N_TOKENS - 3]  # windows of 128, 128 and 44 tokens
        out[f"{tag}/tokens"] = r["tokens"]
        out[f"{tag}/nll_per_window"], out[f"{tag}/toks"] = r["nll"], np.int64(r["toks"])
        out[f"{tag}/ppl"] = np.float64(np.exp(r["nll"].sum() / r["toks"]))
        out[f"{tag}/base_nll_per_window"], out[f"{tag}/base_toks"] = r["nllb"], np.int64(r["toksb"])
        out[f"{tag}/base_ppl"] = np.float64(np.exp(r["nllb"].sum() / r["toksb"]))
        out[f"{tag}/ref_bf16_nll_per_window"] = r["nll16"]
        out[f"{tag}/rel_finetune_min"], out[f"{tag}/rel_ref_bf16_max"] = np.float64(r["move"]), np.float64(r["bf16"])
    # the instruction wrap of the reference's evaluate scripts: the builtin `input` as the sample's input
    out["wrap_instruction"] = np.array("TEXT")
    out["wrap_prompt"] = np.array(generate_prompt({"instruction": "TEXT", "input": input}))
    MG.save("eval_finetuned", **out)


if __name__ == "__main__":
    gen_eval_finetuned()
