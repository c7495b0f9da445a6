"""Generate tests/golden/adapter_v2.npz from the REFERENCE's LLaMA-Adapter v2 model: lit_llama/adapter.py's
LLaMA with lit_llama/adapter_v2.py's add_adapter_v2_parameters_to_linear_layers.

Same conditions and helpers as make_golden_adapter.py (which this script imports): runs only where
the reference is mounted; only the arrays written here are committed. Base weights are
oracle.weights.make_params(cfg, seed) (RMSNorm scales ~ U(0.5, 1.5)); the v1 tensors are
make_golden_adapter.adapter_tensors; every Linear, lm_head included, gets
    adapter_scale = +-U(0.5, 1.5) per column,
    adapter_bias  = BIAS_REL * rms(that Linear's own output on the probe prompt) * N(0, 1) per column,
drawn per Linear (so they differ per column and per layer). The bias is sized from the Linear's output
so that it matters in every Linear; the generator asserts on the reference alone that an identity affine
(scale 1, bias 0) moves the fp32 logits by more than 0.1 relative.

The greedy prompts come from make_golden_adapter.scan (bf16 and fp32 ids agree on all N_NEW steps,
margins above the guards on the first GUARD_STEPS steps).

Usage:  python tests/golden/make_golden_adapter_v2.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_golden as MG  # noqa: E402
import make_golden_adapter as MA  # noqa: E402  (adapter_tensors, scan, margins_ok, the guards)
from lit_llama import adapter as radp  # noqa: E402  (the reference's)
from lit_llama import adapter_v2 as radp2  # noqa: E402

from oracle.weights import Cfg, make_params, make_prompt  # noqa: E402

AT, START = MA.AT, MA.START
BIAS_REL = 0.5
LINEARS = ("attn.c_attn", "attn.c_proj", "mlp.c_fc1", "mlp.c_fc2", "mlp.c_proj")


def linear_names(cfg: Cfg):
    return [f"transformer.h.{i}.{n}" for i in range(cfg.n_layer) for n in LINEARS] + ["lm_head"]


def ref_v2(cfg: Cfg, params: dict, adp: dict, dtype=torch.float32, start: int = START):
    """The reference's v2 model; adapter_scale / adapter_bias missing from `adp` stay at their
    identity initialisation (ones / zeros, adapter_v2.py:35-36)."""
    rc = radp.LLaMAConfig(block_size=cfg.block_size, vocab_size=cfg.vocab_size, n_layer=cfg.n_layer, n_head=cfg.n_head,
                          n_embd=cfg.n_embd, adapter_prompt_length=AT, adapter_start_layer=start)
    m = radp.LLaMA(rc)
    radp2.add_adapter_v2_parameters_to_linear_layers(m)
    sd = {k: torch.from_numpy(np.ascontiguousarray(v).copy()) for k, v in {**params, **adp}.items()}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all("adapter_scale" in k or "adapter_bias" in k for k in missing), (missing, unexpected)
    return m.to(dtype).eval()


@torch.no_grad()
def v2_tensors(cfg: Cfg, params: dict, v1: dict, seed: int, start: int = START) -> dict:
    """adapter_scale / adapter_bias of every Linear; the bias scale from the rms of the Linear's own
    output (identity affine, fp32) on a fixed probe prompt."""
    m = ref_v2(cfg, params, v1, start=start)
    rms, hooks = {}, []
    mods = dict(m.named_modules())
    for name in linear_names(cfg):
        def hook(_m, _i, out, name=name):
            rms[name] = max(rms.get(name, 0.0), float(out.float().pow(2).mean().sqrt()))
        hooks.append(mods[name].register_forward_hook(hook))
    m(torch.from_numpy(make_prompt(12, cfg.vocab_size, seed)[None]).long())
    for h in hooks:
        h.remove()
    rng = np.random.default_rng(seed)
    out = {}
    for name in linear_names(cfg):
        N = mods[name].weight.shape[0]
        out[name + ".adapter_scale"] = (rng.uniform(0.5, 1.5, N) * rng.choice([-1.0, 1.0], N)).astype(np.float32)
        out[name + ".adapter_bias"] = (BIAS_REL * rms[name] * rng.standard_normal(N)).astype(np.float32)
    return out


@torch.no_grad()
def gen_adapter_v2():
    out = {}
    cfg = Cfg(block_size=128, n_layer=4, n_head=4, n_embd=256, vocab_size=2048)
    seed = 2403
    params = make_params(cfg, seed)
    v1 = MA.adapter_tensors(cfg, START, AT, seed + 1)
    adp = {**v1, **v2_tensors(cfg, params, v1, seed + 2)}
    out["seed"] = np.int64(seed)
    out["aT"], out["start"] = np.int64(AT), np.int64(START)
    for k, v in adp.items():
        out["adp/" + k] = v
    m32 = ref_v2(cfg, params, adp)
    out["sd_keys"] = np.array(sorted(m32.state_dict().keys()))
    out["adapter_keys"] = np.array(sorted(radp2.adapter_v2_state_from_state_dict(m32.state_dict()).keys()))
    models = {"fp32": m32, "bf16": ref_v2(cfg, params, adp, torch.bfloat16)}

    for tag, S, first in (("", None, 100), ("roll_", 16, 200)):
        ps, prompt, tr = MA.scan(models, cfg.vocab_size, 12, S, first)
        out[tag + "prompt_seed"], out[tag + "prompt"] = np.int64(ps), prompt
        for dt in ("fp32", "bf16"):
            ids, L, v, i = tr[dt]
            assert np.array_equal(tr["bf16"][0], tr["fp32"][0]) and MA.margins_ok(v, MA.TOL[dt])
            out[f"{tag}{dt}_ids"], out[f"{tag}{dt}_top_v"], out[f"{tag}{dt}_top_i"] = ids, v, i
    idx = torch.from_numpy(out["prompt"][None]).long()
    ref = m32(idx).numpy()[0]
    out["fp32_prefill_nocache"] = ref
    ident = ref_v2(cfg, params, v1)(idx).numpy()[0]  # scale 1, bias 0: the v1 model
    b = models["bf16"](idx).float().numpy()[0]
    out["rel_identity_affine"] = np.float64(np.linalg.norm(ident - ref) / np.linalg.norm(ref))
    out["rel_ref_bf16"] = np.float64(np.linalg.norm(b - ref) / np.linalg.norm(ref))
    print(f"an identity affine moves the fp32 logits by {out['rel_identity_affine']:.3f} relative; "
          f"reference bf16 vs fp32 {out['rel_ref_bf16']:.3e}")
    assert out["rel_identity_affine"] > 0.1  # a dropped affine cannot pass
    # ... and so does dropping the bias alone, or the scale alone
    nob = ref_v2(cfg, params, {k: v for k, v in adp.items() if "adapter_bias" not in k})(idx).numpy()[0]
    nos = ref_v2(cfg, params, {k: v for k, v in adp.items() if "adapter_scale" not in k})(idx).numpy()[0]
    out["rel_no_bias"] = np.float64(np.linalg.norm(nob - ref) / np.linalg.norm(ref))
    out["rel_no_scale"] = np.float64(np.linalg.norm(nos - ref) / np.linalg.norm(ref))
    print(f"without the biases {out['rel_no_bias']:.3f}, without the scales {out['rel_no_scale']:.3f}")
    assert out["rel_no_bias"] > 0.1 and out["rel_no_scale"] > 0.1

    # ---- head size 128 (n_head 2): fp32 prefill logits only
    cfg2 = Cfg(block_size=128, n_layer=4, n_head=2, n_embd=256, vocab_size=2048)
    p2 = make_params(cfg2, seed + 10)
    v12 = MA.adapter_tensors(cfg2, START, AT, seed + 11)
    a2 = {**v12, **v2_tensors(cfg2, p2, v12, seed + 12)}
    for k, v in a2.items():
        out["hs128/adp/" + k] = v
    out["hs128/seed"] = np.int64(seed + 10)
    pr2 = make_prompt(12, cfg2.vocab_size, seed + 10)
    out["hs128/prompt"] = pr2
    out["hs128/fp32_prefill_nocache"] = ref_v2(cfg2, p2, a2)(torch.from_numpy(pr2[None]).long()).numpy()[0]

    # ---- int4 (the reference cannot run v2 on quantized Linears): only the v1 + v2 tensors for the
    # 2-layer model of int4_gptq.npz, adapter from layer 1 on; the test builds its own reference from
    # the dequantized weights
    g4 = dict(np.load(HERE / "int4_gptq.npz"))
    cfg4 = Cfg(block_size=128, n_layer=2, n_head=4, n_embd=256, vocab_size=2048)
    p4 = make_params(cfg4, int(g4["seed"]))
    v14 = MA.adapter_tensors(cfg4, 1, AT, seed + 21)
    a4 = {**v14, **v2_tensors(cfg4, p4, v14, seed + 22, start=1)}
    for k, v in a4.items():
        out["int4/adp/" + k] = v
    out["int4/start"] = np.int64(1)
    out["int4/prompt"] = g4["prompt"]
    MG.save("adapter_v2", **out)


if __name__ == "__main__":
    gen_adapter_v2()
