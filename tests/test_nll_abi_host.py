"""CPU tests of the NLL entry points' boundary (no GPU needed), in the style of tests/test_abi_host.py: llj_nll
and llj_g_nll are declared in include/lit_llama_amd_nll.h, which lit_llama_amd.h includes (its own declaration
list is pinned by tests/test_adapter_v2_host.py), bound in lit_llama/_hip.py's NLL_SIGNATURES with the same
arity and argument kinds, exported by the built library, and refuse bad arguments on the host (LLJ_EINVAL before any
launch, so no device is touched); LLaMA carries window_nll and evaluate/full.py's perplexity goes through it.
"""
import ctypes
import inspect
import subprocess

import tests.test_abi_host as ABI
from tests.test_abi_host import _lib_path

NLL_HEADER = ABI.REPO / "include" / "lit_llama_amd_nll.h"

NAMES = ("llj_nll", "llj_g_nll")
KINDS = ["p", "i", "i", "i", "p", "p", "p", "p"]  # logits, ldl, M, V, targets, row_nll, total, stream


def _nll_decls(monkeypatch):
    monkeypatch.setattr(ABI, "HEADER", NLL_HEADER)  # test_abi_host's parser over the NLL header
    return ABI._header_decls()


def test_header_declares_both(monkeypatch):
    assert '#include "lit_llama_amd_nll.h"' in ABI.HEADER.read_text()
    decls = _nll_decls(monkeypatch)
    assert set(decls) == set(NAMES)
    for name in NAMES:
        assert decls[name] == ("int", KINDS), name


def test_ctypes_table_matches():
    from lit_llama import _hip

    kind = {ctypes.c_void_p: "p", ctypes.c_int: "i"}
    assert set(_hip.NLL_SIGNATURES) == set(NAMES)
    for name in NAMES:
        assert [kind[a] for a in _hip.NLL_SIGNATURES[name]] == KINDS, name


def test_library_exports_both():
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib_path())], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NAMES) <= exported


def test_argument_checks_on_the_host():
    """NULL pointers, M <= 0, V <= 0 and ldl < V: LLJ_EINVAL (1000), decided before any launch. The pointers
    are never dereferenced on this path, so placeholders serve."""
    from lit_llama import _hip

    L = ctypes.CDLL(str(_lib_path()))
    p = ctypes.c_void_p(4096)
    for name in NAMES:
        f = getattr(L, name)
        f.argtypes, f.restype = _hip.NLL_SIGNATURES[name], ctypes.c_int
        good = [p, 8, 2, 8, p, p, None, None]
        for i, bad in ((0, None), (4, None), (5, None), (2, 0), (2, -1), (3, 0), (3, -5), (1, 7)):
            a = list(good)
            a[i] = bad
            assert f(*a) == 1000, (name, i, bad)


def test_model_method_and_perplexity_use_it():
    from evaluate import full
    from lit_llama import LLaMA
    from lit_llama.adapter import LLaMA as AdapterLLaMA

    assert list(inspect.signature(LLaMA.window_nll).parameters) == ["self", "idx", "total"]
    assert AdapterLLaMA.window_nll is LLaMA.window_nll
    assert list(inspect.signature(full.perplexity).parameters) == ["model", "encoded_text", "window"]
    src = inspect.getsource(full.perplexity)
    assert "window_nll" in src and "cross_entropy" not in src
