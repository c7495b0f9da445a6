"""CPU tests of evaluate/adapter.py, evaluate/adapter_v2.py and evaluate/lora.py (no GPU needed): the
reference's flags with the reference's defaults, the refusal of llm.int8 before anything is read, and the
instruction wrap against the string recorded from the reference (tests/golden/eval_finetuned.npz).
"""
import importlib.util
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
EVAL = REPO / "lit-llama-ja_amd" / "evaluate"
# script -> (the fine-tuned checkpoint's flag, its default in the reference's script of the same name)
SCRIPTS = {
    "adapter": ("adapter_path", "out/adapter/alpaca/lit-llama-adapter-finetuned.pth"),
    "adapter_v2": ("adapter_path", "out/adapter_v2/alpaca/lit-llama-adapter-finetuned.pth"),
    "lora": ("lora_path", "out/lora/alpaca/lit-llama-lora-finetuned.pth"),
}


def load(name):
    spec = importlib.util.spec_from_file_location(f"llj_evaluate_{name}", EVAL / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", list(SCRIPTS))
def test_flags_and_defaults_are_the_references(name):
    mod = load(name)
    flag, default = SCRIPTS[name]
    a = mod.cli().parse_args(["--text_path", "a.txt,b.txt"])
    assert a.text_path == "a.txt,b.txt"
    assert getattr(a, flag) == Path(default)
    assert a.checkpoint_path == Path("checkpoints/lit-llama/7B/lit-llama.pth")
    assert a.tokenizer_path == Path("checkpoints/lit-llama/tokenizer.model")
    assert a.dtype == "float32" and a.quantize is None
    b = mod.cli().parse_args(["--text_path", "t", f"--{flag}", "x.pth", "--checkpoint_path", "c.pth", "--tokenizer_path",
                              "tok.json", "--dtype", "bfloat16", "--quantize", "gptq.int4"])
    assert (getattr(b, flag), b.checkpoint_path, b.tokenizer_path) == (Path("x.pth"), Path("c.pth"), Path("tok.json"))
    assert (b.dtype, b.quantize) == ("bfloat16", "gptq.int4")
    assert mod.instruction_tuning is True
    if name == "lora":
        assert (mod.lora_r, mod.lora_alpha, mod.lora_dropout) == (8, 16, 0.05)


@pytest.mark.parametrize("name", list(SCRIPTS))
def test_help_runs_without_a_gpu(name):
    out = subprocess.run([sys.executable, str(EVAL / f"{name}.py"), "--help"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    for flag in ("--text_path", f"--{SCRIPTS[name][0]}", "--checkpoint_path", "--tokenizer_path", "--dtype",
                 "--quantize"):
        assert flag in out.stdout


@pytest.mark.parametrize("name", ["adapter_v2", "lora"])
def test_llm_int8_is_refused_before_any_file_is_read(name, tmp_path):
    """The paths do not exist: the refusal comes before the scripts look at them."""
    mod = load(name)
    missing = tmp_path / "missing.pth"
    with pytest.raises(NotImplementedError, match="LLM.int8"):
        mod.main("missing.txt", **{SCRIPTS[name][0]: missing}, checkpoint_path=missing, tokenizer_path=missing,
                 quantize="llm.int8")


def test_invalid_dtype_is_named():
    with pytest.raises(ValueError, match="not a valid dtype"):
        load("adapter").main("missing.txt", dtype="float33")


def test_instruction_wrap_is_the_references(golden):
    """The reference passes the builtin `input` as the sample's input: the "with input" prompt whose input
    section reads "<built-in function input>". The fixture holds what the reference's own generate_prompt
    returned for it."""
    g = golden("eval_finetuned")
    text, want = str(g["wrap_instruction"]), str(g["wrap_prompt"])
    assert "### Input:\n<built-in function input>\n\n### Response:" in want
    for name in SCRIPTS:
        mod = load(name)
        v1 = mod if name == "adapter" else mod._v1
        assert v1.instruction_text(text, mod.instruction_tuning) == want
        assert v1.instruction_text(text, False) == text
    v1 = load("adapter")
    assert v1.instruction_text(text) == want  # None = the module constant
    v1.instruction_tuning = False
    assert v1.instruction_text("raw text\n") == "raw text\n"
    long = "line one\n\nline two " * 50
    assert v1.instruction_text(long, True) == want.replace("TEXT", long)
