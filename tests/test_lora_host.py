"""CPU tests of the LoRA surface (no GPU needed): lit_llama.lora mirrors the reference's lit_llama/lora.py
(names, parameter shapes, state-dict keys, lora_state_dict's three bias modes, lora_ind / zero_pad, the
context manager), LoRA goes onto ColBlockQuantizedLinear inside quantization(mode), the unsupported
combinations are refused before any launch, generate/lora.py and scripts/convert_lora_weights.py keep
the reference's flags and defaults, and the new entry points are declared and bound. Expected values:
tests/golden/lora.npz, written by the reference (tests/golden/make_golden_lora.py)."""
import ctypes
import importlib.util
import inspect
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
CLI = REPO / "lit-llama-ja_amd" / "generate" / "lora.py"
CONVERT = REPO / "lit-llama-ja_amd" / "scripts" / "convert_lora_weights.py"
HEADER = REPO / "include" / "lit_llama_amd.h"
LORA_HEADER = REPO / "include" / "lit_llama_amd_lora.h"

LORA_TAIL = ["const void* lora_t", "int ldt", "const void* lora_B", "int r", "int enable_mask", "float scaling"]
LORA_ENTRY_POINTS = {"llj_norm_qkv_rope_lora": "llj_norm_qkv_rope", "llj_gemm_qkv_rope_lora": "llj_gemm_qkv_rope",
                     "llj_g_linear_lora": "llj_g_linear"}


def tiny():
    from lit_llama import LLaMAConfig

    return LLaMAConfig(block_size=128, vocab_size=2048, n_layer=4, n_head=4, n_embd=256)


def lora_model(mode=None, r=8, alpha=16, dropout=0.0):
    from lit_llama import LLaMA
    from lit_llama.lora import lora
    from lit_llama.utils import quantization

    with quantization(mode), lora(r=r, alpha=alpha, dropout=dropout, enabled=True):
        return LLaMA(tiny())


def test_state_dict_keys_equal_the_reference(golden):
    from lit_llama.lora import LoRALayer, MergedLinear

    g = golden("lora")
    m = lora_model()
    assert sorted(m.state_dict().keys()) == [str(k) for k in g["sd_keys"]]
    for blk in m.transformer.h:
        c = blk.attn.c_attn
        assert isinstance(c, MergedLinear) and isinstance(c, LoRALayer) and isinstance(c, torch.nn.Linear)
        assert c.lora_A.shape == (8 * 2, 256) and c.lora_B.shape == (3 * 256 // 3 * 2, 8)  # lora.py:149-153
        assert c.scaling == 2.0 and c.r == 8 and c.lora_alpha == 16 and c.enable_lora == [True, False, True]
        assert not c.merged and c.merge_weights and not c.weight.requires_grad
        assert torch.count_nonzero(c.lora_B) == 0 and torch.count_nonzero(c.lora_A) > 0  # lora.py:194-201
        assert type(blk.attn.c_proj) is torch.nn.Linear
    for k in g:
        if k.startswith("lora/"):
            assert tuple(m.state_dict()[k[5:]].shape) == g[k].shape, k


@pytest.mark.parametrize("bias", ["none", "all", "lora_only"])
def test_lora_state_dict_bias_modes(golden, bias):
    from lit_llama.lora import lora_state_dict

    g = golden("lora")
    assert sorted(lora_state_dict(lora_model(), bias=bias)) == [str(k) for k in g["lora_keys_" + bias]]


def test_lora_state_dict_and_trainable_marks():
    from lit_llama.lora import lora_state_dict, mark_only_lora_as_trainable

    m = lora_model()
    with pytest.raises(NotImplementedError):
        lora_state_dict(m, bias="some")
    mark_only_lora_as_trainable(m)
    for name, prm in m.named_parameters():
        assert prm.requires_grad == ("lora_" in name), name
    with pytest.raises(NotImplementedError):
        mark_only_lora_as_trainable(m, bias="some")
    # a biased LoRA Linear: its bias follows "all" and "lora_only" (lora.py:346-357, 381-391)
    from lit_llama.lora import MergedLinear

    holder = torch.nn.ModuleDict({"a": MergedLinear(32, 48, r=2, lora_alpha=4, enable_lora=[True, False, True], bias=True),
                                  "b": torch.nn.Linear(8, 8, bias=True)})
    assert sorted(lora_state_dict(holder, "lora_only")) == ["a.bias", "a.lora_A", "a.lora_B"]
    assert sorted(lora_state_dict(holder, "all")) == ["a.bias", "a.lora_A", "a.lora_B", "b.bias"]
    mark_only_lora_as_trainable(holder, "lora_only")
    assert holder["a"].bias.requires_grad and not holder["b"].bias.requires_grad


def test_context_manager_swaps_and_restores():
    from lit_llama import LLaMA
    from lit_llama import lora as L
    from lit_llama import model

    orig = model.CausalSelfAttention
    with L.lora(r=8, alpha=16, dropout=0.05):
        assert model.CausalSelfAttention is L.CausalSelfAttention
        assert L.CausalSelfAttention.lora_config == L.LoRAConfig(r=8, alpha=16, dropout=0.05)
    assert model.CausalSelfAttention is orig and L.CausalSelfAttention.lora_config is None
    with pytest.raises(KeyError):
        with L.lora(r=8, alpha=16, dropout=0.05):
            raise KeyError("body raised")
    assert model.CausalSelfAttention is orig and L.CausalSelfAttention.lora_config is None
    with L.lora(r=8, alpha=16, dropout=0.05, enabled=False):  # a no-op: the plain model
        assert model.CausalSelfAttention is orig
        m = LLaMA(tiny())
    assert type(m.transformer.h[0].attn.c_attn) is torch.nn.Linear
    assert not any("lora_" in k for k in m.state_dict())


def test_lora_ind_and_zero_pad_match_the_reference(golden):
    g = golden("lora")
    c = lora_model().transformer.h[0].attn.c_attn
    np.testing.assert_array_equal(c.lora_ind.numpy(), g["lora_ind"])
    assert c.lora_ind.dtype == torch.bool and int(c.lora_ind.sum()) == 2 * 256
    rows, cols = (int(v) for v in g["zero_pad_in_shape"])
    x = torch.arange(rows * cols, dtype=torch.float32).view(rows, cols)
    np.testing.assert_array_equal(c.zero_pad(x).numpy(), g["zero_pad_out"])


@pytest.mark.parametrize("en", [[True, False, False], [False, True, False], [False, False, True], [True, True, False],
                                [True, False, True], [False, True, True], [True, True, True]])
def test_enable_lora_masks(en):
    from lit_llama.lora import MergedLinear, _enable_mask

    lin = MergedLinear(32, 48, r=3, lora_alpha=6, enable_lora=en, bias=False)
    n_en = sum(en)
    assert lin.lora_A.shape == (3 * n_en, 32) and lin.lora_B.shape == (16 * n_en, 3)
    assert lin.lora_ind.view(3, 16).all(dim=1).tolist() == en
    assert _enable_mask(en) == sum(1 << i for i, on in enumerate(en) if on)
    z = lin.zero_pad(torch.ones(16 * n_en, 5))
    assert z.shape == (48, 5) and (z.view(3, 16, 5).sum(dim=(1, 2)) > 0).tolist() == en


@pytest.mark.parametrize("mode,bits", [("gptq.int4", 4), ("gptq.int8", 8)])
def test_lora_on_colblock_linears(mode, bits, golden):
    from lit_llama.quantization import ColBlockQuantizedLinear

    m = lora_model(mode)
    assert torch.nn.Linear is torch.nn.modules.linear.Linear  # the context restored the class
    g = golden("lora")
    for blk in m.transformer.h:
        c = blk.attn.c_attn
        assert isinstance(c, ColBlockQuantizedLinear) and c.bits == bits
        assert isinstance(c.lora_A, torch.nn.Parameter) and c.lora_A.shape == (16, 256)
        assert isinstance(c.lora_B, torch.nn.Parameter) and c.lora_B.shape == (512, 8)
        assert c.r == 8 and c.scaling == 2.0 and c.enable_lora == [True, False, True] and not c.merge_weights
        m.eval()
        assert c.merged is False  # never merges
        m.train()
        assert c.merged is False
        assert isinstance(blk.attn.c_proj, ColBlockQuantizedLinear) and not hasattr(blk.attn.c_proj, "lora_A")
    keys = set(m.state_dict())
    assert {str(k) for k in g["lora_keys_none"]} <= keys  # the reference's LoRA checkpoint loads
    assert "transformer.h.0.attn.c_attn.quant_weight" in keys and "transformer.h.0.attn.c_attn.weight" not in keys


def test_refusals_need_no_gpu():
    """Section "Refused before any launch": every one of them raises from the operand set-up on the CPU."""
    from lit_llama import model
    from lit_llama.adapter_v2 import adapter_v2_linear_with_bias_and_scale
    from lit_llama.lora import MergedLinear, lora, lora_operands
    from lit_llama.quantization import Linear8bitLt
    from lit_llama.utils import quantization

    with pytest.raises(NotImplementedError, match="LLM.int8"):  # Linear8bitLt with LoRA
        lora_model("llm.int8")
    l8 = Linear8bitLt(128, 48, bias=False)
    l8.lora_A = torch.nn.Parameter(torch.zeros(16, 128))
    l8.lora_B = torch.nn.Parameter(torch.zeros(32, 8))
    with pytest.raises(NotImplementedError, match="LLM.int8"):
        model._lora(l8, torch.bfloat16)
    with pytest.raises(NotImplementedError, match="fan_in_fan_out"):
        MergedLinear(32, 48, r=2, enable_lora=[True, False, True], fan_in_fan_out=True)
    # LoRA + adapter v2 parameters on one Linear: TypeError, dense and quantized
    for mode in (None, "gptq.int4"):
        c = lora_model(mode).transformer.h[0].attn.c_attn
        assert model._lora(torch.nn.Linear(8, 8)) is None
        adapter_v2_linear_with_bias_and_scale(c)
        with pytest.raises(TypeError, match="adapter v2"):
            model._lora(c, torch.float32)
    # a forward in train mode with lora_dropout > 0
    m = lora_model(dropout=0.05).train()
    with pytest.raises(NotImplementedError, match="dropout"):
        m._layer_specs()
    with pytest.raises(NotImplementedError, match="dropout"):
        lora_operands(m.transformer.h[0].attn.c_attn, torch.float32)
    with quantization("gptq.int4"), lora(r=8, alpha=16, dropout=0.05):
        from lit_llama import LLaMA

        mq = LLaMA(tiny())
    with pytest.raises(NotImplementedError, match="dropout"):
        model._lora(mq.train().transformer.h[0].attn.c_attn, torch.float32)


def test_product_path_has_no_cpu_fallback():
    """eval() merges on the GPU only; an unmerged forward off the GPU raises."""
    from lit_llama import _hip

    m = lora_model()
    with pytest.raises(_hip.HipError):
        m.eval()
    c = lora_model().transformer.h[0].attn.c_attn
    with pytest.raises(_hip.HipError):
        c(torch.zeros(1, 256))


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_generate_lora_cli_matches_the_reference_flags():
    out = subprocess.run([sys.executable, str(CLI), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    for flag in ("--prompt", "--input", "--lora_path", "--pretrained_path", "--tokenizer_path", "--quantize",
                 "--max_new_tokens", "--top_k", "--temperature"):
        assert flag in out.stdout, flag
    mod = _load(CLI, "llj_generate_lora")
    # reference generate/lora.py:20-35
    assert (mod.lora_r, mod.lora_alpha, mod.lora_dropout) == (8, 16, 0.05)
    assert [(n, p.default) for n, p in inspect.signature(mod.main).parameters.items()] == [
        ("prompt", "What food do lamas eat?"), ("input", ""),
        ("lora_path", Path("out/lora/alpaca/lit-llama-lora-finetuned.pth")),
        ("pretrained_path", Path("checkpoints/lit-llama/7B/lit-llama.pth")),
        ("tokenizer_path", Path("checkpoints/lit-llama/tokenizer.model")), ("quantize", None),
        ("max_new_tokens", 100), ("top_k", 200), ("temperature", 0.8)]
    assert mod.RESPONSE_MARK == "### Response:"
    assert "extension" in mod.__doc__ and "gptq.int4" in mod.__doc__
    with pytest.raises(NotImplementedError, match="LLM.int8"):
        mod.load_model({}, {}, "llm.int8")


def test_convert_lora_weights_cli_matches_the_reference_flags():
    out = subprocess.run([sys.executable, str(CONVERT), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    for flag in ("--accelerator", "--lora_path", "--checkpoint_path", "--dtype"):
        assert flag in out.stdout, flag
    mod = _load(CONVERT, "llj_convert_lora_weights")
    # reference scripts/convert_lora_weights.py:33-38
    assert [(n, p.default) for n, p in inspect.signature(mod.main).parameters.items()] == [
        ("accelerator", "auto"), ("lora_path", None), ("checkpoint_path", None), ("dtype", "bfloat16")]
    assert mod.lora_model_lookup({"transformer.h.0.attn.c_attn.lora_B": torch.zeros(512, 4)}) == 4
    m = lora_model()
    assert sorted(mod.del_lora_state_dict(m)) == sorted(k for k in m.state_dict() if "lora_" not in k)


def _decls(path):
    text = re.sub(r"/\*.*?\*/", "", path.read_text(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return {name: " ".join(args.split())
            for _, name, args in re.findall(r"\b(int|size_t)\s+(llj_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.S)}


def test_header_declares_the_lora_entry_points():
    """The LoRA header is part of the ABI header (included by it); each `_lora` form takes the existing
    argument list plus (lora_t, ldt, lora_B, r, enable_mask, scaling); the ctypes table has the same kinds."""
    from lit_llama import _hip

    assert '#include "lit_llama_amd_lora.h"' in HEADER.read_text()
    base, decls = _decls(HEADER), _decls(LORA_HEADER)
    assert set(decls) == set(LORA_ENTRY_POINTS) | {"llj_lora_merge"} == set(_hip.LORA_SIGNATURES)
    for name, parent in LORA_ENTRY_POINTS.items():
        args, bargs = decls[name].split(", "), base[parent].split(", ")
        assert args[:len(bargs)] == bargs and args[len(bargs):] == LORA_TAIL, name
    kind = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_float: "f"}
    for name, argt in _hip.LORA_SIGNATURES.items():
        want = ["p" if "*" in a else "f" if a.startswith("float") else "i" for a in decls[name].split(", ")]
        assert [kind[a] for a in argt] == want, name


def test_library_exports_the_lora_entry_points():
    from lit_llama import _build, _hip

    if not _hip.LIB_PATH.exists():
        _build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", str(_hip.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(_hip.LORA_SIGNATURES) <= exported
    L = ctypes.CDLL(str(_hip.LIB_PATH))
    L.llj_lora_merge.argtypes = _hip.LORA_SIGNATURES["llj_lora_merge"]
    assert L.llj_lora_merge(None, None, None, 48, 128, 8, 5, 2.0, 1, 0, None) == 1000  # refused before any launch
