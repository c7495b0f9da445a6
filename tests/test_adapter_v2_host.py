"""CPU tests of the LLaMA-Adapter v2 surface (no GPU needed): lit_llama.adapter_v2 mirrors the reference's
lit_llama/adapter_v2.py (names, parameter shapes and initial values, state-dict keys, the substrings an
adapter checkpoint holds), the parameters go onto ColBlockQuantizedLinear inside quantization(mode),
generate/adapter_v2.py keeps the reference's flags and defaults, and include/lit_llama_amd.h declares
the new entry points next to the untouched existing ones. Expected values: tests/golden/adapter_v2.npz,
written by the reference (tests/golden/make_golden_adapter_v2.py)."""
import hashlib
import importlib.util
import inspect
import re
import subprocess
import sys
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
CLI = REPO / "lit-llama-ja_amd" / "generate" / "adapter_v2.py"
HEADER = REPO / "include" / "lit_llama_amd.h"

V2_ENTRY_POINTS = {  # name -> the existing entry point whose argument list it extends, pointer arguments added
    "llj_linear_v2": ("llj_linear", 2),
    "llj_norm_qkv_rope_v2": ("llj_norm_qkv_rope", 2),
    "llj_linear_resid_v2": ("llj_linear_resid", 2),
    "llj_linear_resid_attn_v2": ("llj_linear_resid_attn", 2),
    "llj_norm_swiglu_v2": ("llj_norm_swiglu", 4),
    "llj_norm_linear_v2": ("llj_norm_linear", 2),
    "llj_gemm_linear_v2": ("llj_gemm_linear", 2),
    "llj_gemm_resid_v2": ("llj_gemm_resid", 2),
    "llj_gemm_silu_mul_v2": ("llj_gemm_silu_mul", 2),
    "llj_gemm_qkv_rope_v2": ("llj_gemm_qkv_rope", 2),
    "llj_g_linear_v2": ("llj_g_linear", 2),
}
# sha256 over the declarations ("ret name(args);", whitespace collapsed, sorted by name) the header held
# before the adapter v2 entry points were added
EXISTING_DECLS_SHA256 = "caeb2088d8cdd92f3c363c851252fae6b348ddd47dd35df4b54ebde22309f782"
EXISTING_DECLS_COUNT = 67


def tiny(**kw):
    from lit_llama.adapter import LLaMAConfig

    return LLaMAConfig(block_size=128, vocab_size=2048, n_layer=4, n_head=4, n_embd=256, **kw)


def v2_model(mode=None):
    from lit_llama.adapter import LLaMA
    from lit_llama.adapter_v2 import add_adapter_v2_parameters_to_linear_layers
    from lit_llama.utils import quantization

    with quantization(mode):
        m = LLaMA(tiny())
        add_adapter_v2_parameters_to_linear_layers(m)
    return m


def test_state_dict_keys_equal_the_reference(golden):
    g = golden("adapter_v2")
    m = v2_model()
    assert sorted(m.state_dict().keys()) == [str(k) for k in g["sd_keys"]]
    lins = [mod for mod in m.modules() if isinstance(mod, torch.nn.Linear)]
    assert len(lins) == 4 * 5 + 1
    for lin in lins:  # adapter_v2.py:35-36: zeros / ones of out_features, trainable
        assert lin.adapter_bias.shape == lin.adapter_scale.shape == (lin.weight.shape[0],)
        assert torch.count_nonzero(lin.adapter_bias) == 0 and bool((lin.adapter_scale == 1).all())
        assert lin.adapter_bias.requires_grad and lin.adapter_scale.requires_grad
    for k in g:
        if k.startswith("adp/"):
            assert tuple(m.state_dict()[k[4:]].shape) == g[k].shape, k


def test_adapter_state_selects_the_reference_substrings(golden):
    from lit_llama.adapter_v2 import (adapter_v2_state_from_state_dict, get_adapter_substrings,
                                      mark_only_adapter_v2_as_trainable)

    g = golden("adapter_v2")
    assert get_adapter_substrings() == ["adapter_wte", "gating_factor", "adapter_scale", "adapter_bias", "rms_1",
                                        "rms_2", "ln_f"]
    m = v2_model()
    sel = adapter_v2_state_from_state_dict(m.state_dict())
    assert sorted(sel) == [str(k) for k in g["adapter_keys"]]
    assert "transformer.ln_f.scale" in sel and "lm_head.adapter_scale" in sel and "lm_head.weight" not in sel
    mark_only_adapter_v2_as_trainable(m)
    for name, prm in m.named_parameters():
        assert prm.requires_grad == (name in sel), name


@pytest.mark.parametrize("mode,bits", [("gptq.int4", 4), ("gptq.int8", 8)])
def test_parameters_on_colblock_linears(mode, bits, golden):
    from lit_llama.quantization import ColBlockQuantizedLinear

    m = v2_model(mode)
    assert torch.nn.Linear is not ColBlockQuantizedLinear  # the context restored the class
    lins = [mod for mod in m.modules() if isinstance(mod, ColBlockQuantizedLinear)]
    assert len(lins) == 4 * 5 + 1 and all(lin.bits == bits for lin in lins)
    for lin in lins:
        assert isinstance(lin.adapter_scale, torch.nn.Parameter) and lin.adapter_scale.shape == (lin.out_features,)
        assert isinstance(lin.adapter_bias, torch.nn.Parameter) and torch.count_nonzero(lin.adapter_bias) == 0
    keys = set(m.state_dict())
    g = golden("adapter_v2")
    assert {str(k) for k in g["adapter_keys"]} <= keys  # the reference's adapter checkpoint loads
    assert "lm_head.quant_weight" in keys and "lm_head.weight" not in keys
    # ... and outside the context too (a model that was built earlier)
    from lit_llama.adapter import LLaMA
    from lit_llama.adapter_v2 import add_adapter_v2_parameters_to_linear_layers
    from lit_llama.utils import quantization

    with quantization(mode):
        m2 = LLaMA(tiny())
    add_adapter_v2_parameters_to_linear_layers(m2)
    assert set(m2.state_dict()) == keys


def test_llm_int8_linear_with_parameters_is_refused():
    """Linear8bitLt + adapter v2 parameters: NotImplementedError from the operand set-up, before a launch."""
    from lit_llama import model
    from lit_llama.adapter_v2 import adapter_v2_linear_with_bias_and_scale
    from lit_llama.quantization import Linear8bitLt

    lin = Linear8bitLt(128, 16, bias=False)
    assert model._affine(lin) is None
    adapter_v2_linear_with_bias_and_scale(lin)
    assert lin.adapter_scale.shape == (16,)
    with pytest.raises(NotImplementedError, match="LLM.int8"):
        model._affine(lin)


def test_generate_adapter_v2_cli_matches_the_reference_flags():
    out = subprocess.run([sys.executable, str(CLI), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    for flag in ("--prompt", "--input", "--adapter_path", "--pretrained_path", "--tokenizer_path", "--quantize",
                 "--max_new_tokens", "--top_k", "--temperature"):
        assert flag in out.stdout, flag
    spec = importlib.util.spec_from_file_location("llj_generate_adapter_v2", CLI)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sig = inspect.signature(mod.main)
    # reference generate/adapter_v2.py:22-32
    assert [(n, p.default) for n, p in sig.parameters.items()] == [
        ("prompt", "What food do lamas eat?"), ("input", ""),
        ("adapter_path", Path("out/adapter_v2/alpaca/lit-llama-adapter-finetuned.pth")),
        ("pretrained_path", Path("checkpoints/lit-llama/7B/lit-llama.pth")),
        ("tokenizer_path", Path("checkpoints/lit-llama/tokenizer.model")), ("quantize", None),
        ("max_new_tokens", 100), ("top_k", 200), ("temperature", 0.8)]
    assert mod.RESPONSE_MARK == "### Response:"
    v1 = importlib.util.spec_from_file_location("llj_generate_adapter", CLI.with_name("adapter.py"))
    m1 = importlib.util.module_from_spec(v1)
    v1.loader.exec_module(m1)
    for s in ({"instruction": "a", "input": "b"}, {"instruction": "a", "input": ""}):
        assert mod.generate_prompt(s) == m1.generate_prompt(s)  # (pinned to the reference by test_adapter_host)


def _decls():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return {name: (ret, " ".join(args.split()))
            for ret, name, args in re.findall(r"\b(int|size_t)\s+(llj_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.S)}


def test_header_declares_the_v2_entry_points_and_keeps_the_rest():
    from lit_llama import _hip

    decls = _decls()
    for name, (base, extra) in V2_ENTRY_POINTS.items():
        assert name in decls and name in _hip.SIGNATURES, name
        args, bargs = decls[name][1].split(", "), decls[base][1].split(", ")
        assert args[:len(bargs)] == bargs, name  # the existing argument list ...
        tail = args[len(bargs):]
        assert len(tail) == extra and all(a.startswith("const void* adapter_") for a in tail), (name, tail)
    old = {n: d for n, d in decls.items() if n not in V2_ENTRY_POINTS}
    blob = "\n".join(f"{old[n][0]} {n}({old[n][1]});" for n in sorted(old))
    assert len(old) == EXISTING_DECLS_COUNT
    assert hashlib.sha256(blob.encode()).hexdigest() == EXISTING_DECLS_SHA256
