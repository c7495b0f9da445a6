"""CPU tests of the boundary of the packed prefill (no GPU needed), in the style of tests/test_ragged_abi_host.py:
llj_rope_kv_packed and llj_attention_prefill_packed are declared in include/lit_llama_amd_packed.h, which
lit_llama_amd.h includes, bound in lit_llama/_hip.py's PACKED_SIGNATURES with the same arity and argument kinds,
exported by the built library, and refuse bad arguments on the host (LLJ_EINVAL before any launch, so no device is
touched); engine.packed_layout's row offsets and tile list; the four generate CLIs list --prompts_file and
--packed_prefill.
"""
import ctypes
import subprocess
import sys

import pytest

import tests.test_abi_host as ABI
from tests.test_abi_host import _lib_path

PACKED_HEADER = ABI.REPO / "include" / "lit_llama_amd_packed.h"

DECLS = {
    # qkv, q_out, kcache, vcache, rope, cu, B, M, n_head, head_size, S, rope_rows, stream
    "llj_rope_kv_packed": ("int", ["p", "p", "p", "p", "p", "p", "i", "i", "i", "i", "i", "i", "p"]),
    # q, kcache, vcache, y, cu, tiles, n_tiles, B, M, n_head, head_size, S, stream
    "llj_attention_prefill_packed": ("int", ["p", "p", "p", "p", "p", "p", "i", "i", "i", "i", "i", "i", "p"]),
}


def test_header_declares_them(monkeypatch):
    assert PACKED_HEADER.is_file()
    assert '#include "lit_llama_amd_packed.h"' in ABI.HEADER.read_text()
    monkeypatch.setattr(ABI, "HEADER", PACKED_HEADER)  # test_abi_host's parser over the new header
    assert ABI._header_decls() == DECLS
    text = " ".join(PACKED_HEADER.read_text().split())
    assert ("int llj_rope_kv_packed(const void* qkv, void* q_out, void* kcache, void* vcache, const float* rope, "
            "const int* cu, int B, int M, int n_head, int head_size, int S, int rope_rows, void* stream);") in text
    assert ("int llj_attention_prefill_packed(const void* q, const void* kcache, const void* vcache, void* y, "
            "const int* cu, const int* tiles, int n_tiles, int B, int M, int n_head, int head_size, int S, "
            "void* stream);") in text


def test_ctypes_table_matches():
    from lit_llama import _hip

    kind = {ctypes.c_void_p: "p", ctypes.c_int: "i"}
    assert set(_hip.PACKED_SIGNATURES) == set(DECLS)
    for name, (_, kinds) in DECLS.items():
        assert [kind[a] for a in _hip.PACKED_SIGNATURES[name]] == kinds, name
    others = (set(_hip.SIGNATURES) | set(_hip.LORA_SIGNATURES) | set(_hip.NLL_SIGNATURES)
              | set(_hip.SAMPLES_SIGNATURES) | set(_hip.RAGGED_SIGNATURES))
    assert not set(_hip.PACKED_SIGNATURES) & others


def test_library_exports_them():
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib_path())], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(DECLS) <= exported


# (index, value) replacements of a good argument list that must give LLJ_EINVAL; tests/test_packed_prefill_kernels_gpu.py
# sends the same lists with real buffers and checks that nothing was written
P = ctypes.c_void_p(4096)
#            qkv q  k  v  rope cu B  M   nh hs   S   rows stream
ROPE_GOOD = [P, P, P, P, P, P, 8, 40, 2, 128, 64, 128, None]
ROPE_BAD = [(i, None) for i in range(6)]
ROPE_BAD += [(9, 32), (9, 96), (9, 256), (9, 0), (6, 0), (6, -1), (6, 65536), (7, 7), (7, 0), (8, 0), (8, -2), (10, 0),
             (10, -1), (11, 0), (11, -5), (11, 63), (10, 129)]
#           q  k  v  y  cu tiles n_tiles B M  nh hs   S   stream
ATT_GOOD = [P, P, P, P, P, P, 8, 8, 40, 2, 128, 64, None]
ATT_BAD = [(i, None) for i in range(6)]
ATT_BAD += [(10, 32), (10, 96), (10, 256), (10, 0), (7, 0), (7, -1), (7, 65536), (8, 7), (8, 0), (9, 0), (9, -2),
            (11, 0), (11, -1), (6, 0), (6, -3)]


def test_argument_checks_on_the_host():
    """A NULL pointer other than stream, head_size outside {64, 128}, B < 1 or > 65535, M < B, n_head < 1, S < 1,
    n_tiles < 1, rope_rows < 1 and S > rope_rows: LLJ_EINVAL (1000), decided before any launch. The pointers are
    never dereferenced on this path, so placeholders serve."""
    from lit_llama import _hip

    L = ctypes.CDLL(str(_lib_path()))
    for name, good, bad in (("llj_rope_kv_packed", ROPE_GOOD, ROPE_BAD),
                            ("llj_attention_prefill_packed", ATT_GOOD, ATT_BAD)):
        f = getattr(L, name)
        f.argtypes, f.restype = _hip.PACKED_SIGNATURES[name], ctypes.c_int
        for i, v in bad:
            a = list(good)
            a[i] = v
            assert f(*a) == 1000, (name, i, v)


def _keys(lengths, b, qb):
    return min(lengths[b], 64 * qb + 64)


@pytest.mark.parametrize("lengths,cu", [([1], [0, 1]), ([64], [0, 64]), ([65, 1, 128], [0, 65, 66, 194])])
def test_packed_layout_rows(lengths, cu):
    from lit_llama.engine import packed_layout

    got_cu, tiles = packed_layout(lengths)
    assert got_cu == cu
    assert all(isinstance(v, int) for v in got_cu) and all(isinstance(v, int) for t in tiles for v in t)


@pytest.mark.parametrize("lengths", [[1], [64], [65, 1, 128], [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200],
                                     [320], [200, 200, 7]])
def test_packed_layout_tiles(lengths):
    from lit_llama.engine import packed_layout

    _, tiles = packed_layout(lengths)
    want = {(b, qb) for b, t in enumerate(lengths) for qb in range((t + 63) // 64)}
    assert len(tiles) == len(want) and set(map(tuple, tiles)) == want  # every (b, qb) exactly once
    keys = [_keys(lengths, b, qb) for b, qb in tiles]
    assert keys == sorted(keys, reverse=True)  # long tiles first
    for (t0, k0), (t1, k1) in zip(zip(tiles, keys), zip(tiles[1:], keys[1:])):
        assert k0 > k1 or tuple(t0) < tuple(t1)  # ties in (b, qb) order


def test_packed_layout_example():
    from lit_llama.engine import packed_layout

    cu, tiles = packed_layout([65, 1, 128])
    assert [tuple(t) for t in tiles] == [(2, 1), (0, 1), (0, 0), (2, 0), (1, 0)]  # 128, 65, 64, 64, 1 keys


@pytest.mark.parametrize("lengths", [[], [3, 0, 2], [-1]])
def test_packed_layout_refuses_empty_prompts(lengths):
    from lit_llama.engine import packed_layout

    with pytest.raises(ValueError):
        packed_layout(lengths)


@pytest.mark.parametrize("script", ["generate.py", "generate/adapter.py", "generate/adapter_v2.py", "generate/lora.py"])
def test_help_lists_the_flags(script):
    out = subprocess.run([sys.executable, str(ABI.REPO / "lit-llama-ja_amd" / script), "--help"],
                         capture_output=True, text=True, check=True).stdout
    assert "--prompts_file" in out and "--packed_prefill" in out and "--prompt" in out
