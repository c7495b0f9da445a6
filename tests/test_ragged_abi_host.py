"""CPU tests of the boundary of llj_attention_ragged (no GPU needed), in the style of tests/test_samples_abi_host.py:
the entry point is declared in include/lit_llama_amd_ragged.h, which lit_llama_amd.h includes, bound in
lit_llama/_hip.py's RAGGED_SIGNATURES with the same arity and argument kinds, exported by the built library, and
refuses bad arguments on the host (LLJ_EINVAL before any launch, so no device is touched); generate.py and
generate/adapter.py list --prompts_file.
"""
import ctypes
import subprocess
import sys

import pytest

import tests.test_abi_host as ABI
from tests.test_abi_host import _lib_path

RAGGED_HEADER = ABI.REPO / "include" / "lit_llama_amd_ragged.h"

# qkv, q_out, kcache, vcache, y, rope, pos, off, B, n_head, head_size, S, rope_rows, stream
DECLS = {
    "llj_attention_ragged": ("int", ["p", "p", "p", "p", "p", "p", "p", "p", "i", "i", "i", "i", "i", "p"]),
}


def test_header_declares_it(monkeypatch):
    assert '#include "lit_llama_amd_ragged.h"' in ABI.HEADER.read_text()
    monkeypatch.setattr(ABI, "HEADER", RAGGED_HEADER)  # test_abi_host's parser over the new header
    assert ABI._header_decls() == DECLS


def test_ctypes_table_matches():
    from lit_llama import _hip

    kind = {ctypes.c_void_p: "p", ctypes.c_int: "i"}
    assert set(_hip.RAGGED_SIGNATURES) == set(DECLS)
    for name, (_, kinds) in DECLS.items():
        assert [kind[a] for a in _hip.RAGGED_SIGNATURES[name]] == kinds, name
    others = set(_hip.SIGNATURES) | set(_hip.LORA_SIGNATURES) | set(_hip.NLL_SIGNATURES) | set(_hip.SAMPLES_SIGNATURES)
    assert not set(_hip.RAGGED_SIGNATURES) & others


def test_library_exports_it():
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib_path())], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(DECLS) <= exported


def test_argument_checks_on_the_host():
    """A NULL pointer other than stream, head_size outside {64, 128}, B < 1 or > 65535, n_head < 1, S < 1,
    rope_rows < 1 and S > rope_rows: LLJ_EINVAL (1000), decided before any launch. The pointers are never
    dereferenced on this path, so placeholders serve."""
    from lit_llama import _hip

    f = ctypes.CDLL(str(_lib_path())).llj_attention_ragged
    f.argtypes, f.restype = _hip.RAGGED_SIGNATURES["llj_attention_ragged"], ctypes.c_int
    p = ctypes.c_void_p(4096)
    #       qkv q  k  v  y  rope pos off B  nh hs   S   rows stream
    good = [p, p, p, p, p, p, p, p, 8, 2, 128, 64, 128, None]
    bad = [(i, None) for i in range(8)]
    bad += [(10, 32), (10, 96), (10, 256), (10, 0), (8, 0), (8, -1), (8, 65536), (9, 0), (9, -2), (11, 0), (11, -1),
            (12, 0), (12, -5), (12, 63), (11, 129)]
    for i, v in bad:
        a = list(good)
        a[i] = v
        assert f(*a) == 1000, (i, v)


@pytest.mark.parametrize("script", ["generate.py", "generate/adapter.py"])
def test_help_lists_prompts_file(script):
    out = subprocess.run([sys.executable, str(ABI.REPO / "lit-llama-ja_amd" / script), "--help"],
                         capture_output=True, text=True, check=True).stdout
    assert "--prompts_file" in out and "--prompt" in out
