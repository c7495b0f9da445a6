"""The exact LLM.int8 input families of tests/test_int8_exact_gpu.py, on the CPU: for every family the oracle's
restatement (oracle/llama_np.py int8_linear, numpy float32) equals the integer / float64 reference of
tests/helpers.py i8_reference bit for bit, so the GPU file's expectation is the oracle's; and the wrong-rounding
references differ from the right one by the floors of helpers.I8Power (test power, from the references alone)."""
import numpy as np
import pytest

from oracle import llama_np as O
from tests import helpers as H


def oracle_equals(c, what):
    ref = O.int8_linear(c["a"], c["cb"], c["scb"])
    assert ref.dtype == np.float32
    assert np.array_equal(ref, c["y16"]), \
        f"{what}: {(ref != c['y16']).sum()} / {ref.size} elements of the oracle differ from the integer reference"
    assert not np.isnan(ref).any()


@pytest.mark.parametrize("layout", list(H.I8_GEMV_LAYOUTS))
def test_gemv_families_oracle_equals_integer_reference(layout):
    pool = H.I8Power()
    wide = H.I8_GEMV_LAYOUTS[layout][0] >= 8192
    for M in (1, 2, 5, 8, 12):
        for N in (16,) if wide else (16, 48):
            c = H.i8_gemv_case(layout, M, N)
            oracle_equals(c, f"{layout} M {M} N {N}")
            pool.add(c)
    if not wide:
        oracle_equals(H.i8_gemv_case(layout, 8, 48, with14=False), f"{layout}, classes 5 and 6 only")
    if H.I8_GEMV_LAYOUTS[layout][0] == 128:  # the QKV cases (C = 128, N = 3 C)
        for M in (1, 8, 10):
            oracle_equals(H.i8_gemv_case(layout, M, 384), f"{layout} M {M} N 384")
    has = len(H.I8_GEMV_LAYOUTS[layout][1]) > 0
    pool.finish(layout, ("inner", "outer", "dropcol", "halfaway") if has else ("halfaway",))


def test_quant8f_family():
    pool = H.I8Power()
    for M in (1, 5, 8):
        for N, K in [(16, 128), (48, 640)]:
            c = H.i8_quant8f_case(M, N, K)
            assert (c["sca"] < 1.0 / 64).all()
            oracle_equals(c, f"quant8f M {M} K {K}")
            pool.add(c)
    pool.finish("quant8f", ("halfaway",))


def test_swiglu_families():
    """The SwiGLU cases of the GEMV and of the GEMM (scale exponents 10 .. 13, so that silu is not the identity)."""
    for layout in ("none", "walk640", "instream"):
        for M in (1, 8):
            for Hn in (16, 48):
                for ws in (1, 2):
                    oracle_equals(H.i8_gemv_case(layout, M, Hn, 0, 10, 13, ws), f"swiglu {layout} M {M} H {Hn}")
            oracle_equals(H.i8_gemv_case(layout, 8, 48, 0, 10, 13, 1, False), f"swiglu {layout}, classes 5 and 6 only")
    for M in (40, 300):
        for K in (128, 640):
            for ncols in sorted({n for n, _ in H.I8_GEMM_SIDES}):
                for ws in (1, 2):
                    oracle_equals(H.i8_gemm_case(M, 128, K, ncols, ws, 10, 13), f"gemm swiglu M {M} K {K} columns {ncols}")


def test_zero_row_family():
    for M in (1, 3):
        c = H.i8_zero_row_case(M, 16, 128)
        oracle_equals(c, f"zero row M {M}")
        assert not O.int8_linear(c["a"], c["cb"], c["scb"])[M - 1].any()


def test_sca_decided_inside_an_outlier_column():
    """Every family with outlier columns and more than one row has a row whose SCA comes from a sub-threshold
    element of an outlier column that another row sets: leaving flagged columns out of SCA changes SCA there."""
    cases = [H.i8_gemv_case(layout, M, 16) for layout in H.I8_GEMV_LAYOUTS for M in (2, 5, 8, 12)]
    cases += [H.i8_gemm_case(M, 128, K, n) for M in (40, 300) for K in (128, 640) for n, _ in H.I8_GEMM_SIDES]
    cases += [H.i8_generic_case(*s) for s in H.I8_GENERIC_SHAPES]
    for c in cases:
        if not c["cols"].size or c["M"] == 1:
            continue
        r = c["rowmax_row"]
        a = np.abs(c["a"][r].astype(np.float64))
        off = np.delete(a, c["cols"]).max()
        assert c["sca"][r] > off, "SCA of the row is reached outside the outlier columns too"
        assert a[c["cols"][0]] == c["sca"][r] < H.I8_THR and (np.abs(c["a"][:, c["cols"][0]]) >= H.I8_THR).any()


@pytest.mark.parametrize("K", [128, 640])
@pytest.mark.parametrize("M", [40, 300])
def test_gemm_families_oracle_equals_integer_reference(M, K):
    pool = H.I8Power()
    for ncols in sorted({n for n, _ in H.I8_GEMM_SIDES}):
        c = H.i8_gemm_case(M, 128, K, ncols)
        oracle_equals(c, f"gemm M {M} K {K} columns {ncols}")
        pool.add(c)
    pool.finish(f"gemm M {M} K {K}")


def test_generic_families_oracle_equals_integer_reference():
    p0, p1 = H.I8Power(), H.I8Power(out=lambda y: np.asarray(y, np.float32).astype(np.float16).astype(np.float32))
    for shape in H.I8_GENERIC_SHAPES:
        c = H.i8_generic_case(*shape)
        oracle_equals(c, f"generic {shape}")
        p0.add(c)
        p1.add(c)
    p0.finish("generic, bf16 output")
    p1.finish("generic, fp16 values as fp32 (dt 1)", ("inner", "dropcol", "halfaway"))


def test_gather_and_qkv_gemm_families():
    for total in (0, 1, 64, 65):
        cols = np.random.default_rng([29, total]).choice(256, total, replace=False)
        oracle_equals(H.i8_exact_case(3, 32, 256, cols, (5, 6, 5), 0, mutants=False), f"gather total {total}")
    for M in (40, 300):
        for ncols in (0, 3, 33):
            oracle_equals(H.i8_gemm_case(M, 384, 128, ncols), f"gemm qkv M {M} columns {ncols}")


def test_special_rows():
    """An all-zero row (SCA 0, output 0, no NaN) and rows that are outliers in every column (SCA 0, every code 0:
    the result is the side product alone)."""
    rng = np.random.default_rng(5)
    c = H.i8_exact_case(3, 16, 128, [7, 90], (5, 6, 5), 0, hot=[[0], [0]])
    a = c["a"].copy()
    a[2] = 0.0
    r = H.i8_reference(a, c["cb"], c["e"])
    ref = O.int8_linear(a, c["cb"], c["scb"])
    assert np.array_equal(ref, r["y16"]) and (ref[2] == 0).all() and r["sca"][2] == 0
    a = rng.choice([6.0, -8.0, 12.0], size=(2, 128)).astype(np.float32)
    r = H.i8_reference(a, c["cb"], c["e"])
    assert (r["sca"] == 0).all() and r["O"].all() and not r["codes"].any()
    assert np.array_equal(O.int8_linear(a, c["cb"], c["scb"]), r["y16"])
