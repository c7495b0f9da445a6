"""CPU tests of the shared-prefix attention entry points' boundary (no GPU needed), in the style of
tests/test_nll_abi_host.py: llj_attention_shared and llj_attention_shared_ws_bytes are declared in
include/lit_llama_amd_samples.h, which lit_llama_amd.h includes, bound in lit_llama/_hip.py's SAMPLES_SIGNATURES
with the same arity and argument kinds, exported by the built library, and refuse bad arguments on the host
(LLJ_EINVAL before any launch, so no device is touched); generate.py lists --batch_samples.
"""
import ctypes
import subprocess
import sys

import tests.test_abi_host as ABI
from tests.test_abi_host import _lib_path

SAMPLES_HEADER = ABI.REPO / "include" / "lit_llama_amd_samples.h"

# q, kcache, vcache, y, pos, B, P, n_head, head_size, S, nsplit, ws, stream
DECLS = {
    "llj_attention_shared_ws_bytes": ("size_t", ["i", "i", "i", "i"]),
    "llj_attention_shared": ("int", ["p", "p", "p", "p", "p", "i", "i", "i", "i", "i", "i", "p", "p"]),
}


def test_header_declares_both(monkeypatch):
    assert '#include "lit_llama_amd_samples.h"' in ABI.HEADER.read_text()
    monkeypatch.setattr(ABI, "HEADER", SAMPLES_HEADER)  # test_abi_host's parser over the new header
    assert ABI._header_decls() == DECLS


def test_ctypes_table_matches():
    from lit_llama import _hip

    kind = {ctypes.c_void_p: "p", ctypes.c_int: "i"}
    assert set(_hip.SAMPLES_SIGNATURES) == set(DECLS)
    for name, (_, kinds) in DECLS.items():
        assert [kind[a] for a in _hip.SAMPLES_SIGNATURES[name]] == kinds, name
    assert not set(_hip.SAMPLES_SIGNATURES) & (set(_hip.SIGNATURES) | set(_hip.LORA_SIGNATURES) | set(_hip.NLL_SIGNATURES))


def test_library_exports_both():
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib_path())], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(DECLS) <= exported


def _bound():
    from lit_llama import _hip

    L = ctypes.CDLL(str(_lib_path()))
    f, g = L.llj_attention_shared, L.llj_attention_shared_ws_bytes
    f.argtypes, f.restype = _hip.SAMPLES_SIGNATURES["llj_attention_shared"], ctypes.c_int
    g.argtypes, g.restype = _hip.SAMPLES_SIGNATURES["llj_attention_shared_ws_bytes"], ctypes.c_size_t
    return f, g


def test_workspace_size():
    """nsplit prefix partials and one suffix partial per (row, head), each head_size + 4 floats (kAttPart)."""
    _, g = _bound()
    assert g(8, 32, 128, 16) == 8 * 32 * 17 * 132 * 4
    assert g(5, 3, 64, 1) == 5 * 3 * 2 * 68 * 4


def test_argument_checks_on_the_host():
    """NULL q / caches / y / pos / ws, head_size outside {64, 128}, B < 1, P < 1, P > S and nsplit outside 1 .. 64:
    LLJ_EINVAL (1000), decided before any launch. The pointers are never dereferenced on this path, so
    placeholders serve."""
    f, _ = _bound()
    p = ctypes.c_void_p(4096)
    #       q  k  v  y  pos B  P   nh hs   S   ns ws stream
    good = [p, p, p, p, p, 8, 17, 2, 128, 64, 4, p, None]
    bad = [(i, None) for i in (0, 1, 2, 3, 4, 11)]
    bad += [(8, 32), (8, 96), (8, 256), (8, 0), (5, 0), (5, -1), (6, 0), (6, -3), (6, 65), (10, 0), (10, -1), (10, 65)]
    for i, v in bad:
        a = list(good)
        a[i] = v
        assert f(*a) == 1000, (i, v)


def test_generate_help_lists_batch_samples():
    out = subprocess.run([sys.executable, str(ABI.REPO / "lit-llama-ja_amd" / "generate.py"), "--help"],
                         capture_output=True, text=True, check=True).stdout
    assert "--batch_samples" in out and "--num_samples" in out
