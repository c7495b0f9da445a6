"""The input conditions of tests/test_epilogue_exact_gpu.py, on the CPU: for every format and shape that file uses,
the exactness conditions (the Linear's, the fp32 sum and product of the affine, d, d * scaling and the LoRA sum:
asserted inside the reference builders for every element) and the power conditions (each wrong-rounding result
differs from the expected one in >= 10 % of the elements, the epilogue changes >= 99 % of them, the first of 16
seeds that meets the floors) are decided by the references alone, before any GPU run. Each group prints its
measured shares and the chosen seeds."""
import numpy as np
import pytest

from tests import helpers as H
from tests import test_epilogue_exact_gpu as E
from tests.helpers import bf16
from tests.test_streaming_exact_gpu import GEMM_FMTS, GEMV_FMTS, NORM_ROWS, QKV_ROWS, ROWS, SWIGLU_ROWS

CUS = 256  # compute units of an MI355X: the multi-tile shapes the GPU file derives from the device


def rows_of(table):
    return sorted({r[0] for r in table})


def test_helpers_rounding_points():
    """exact_affine / affine_bf16 / exact_lora / lora_bf16 on a hand-sized case: value ranges, exactness for every
    element (asserted inside), and each skipped rounding is a different function."""
    rng = np.random.default_rng(5)
    y = rng.integers(-40000, 40001, size=(8, 64)) / 64.0
    sc, bi = H.exact_affine(rng, y)
    odd = np.abs(sc) * 128
    assert (odd == np.rint(odd)).all() and (odd.astype(int) % 2 == 1).all() and (np.abs(sc) != 1.0).all()
    mag = H._col_mag(y)
    assert (np.abs(bi) <= 255 * mag / 128).all() and (np.log2(mag) % 1 == 0).all()
    y32 = y.astype(np.float32)
    want = H.affine_bf16(y32, sc, bi)
    assert np.array_equal(want, bf16(bf16(bf16(y32) + bi) * sc))
    for k in ("y", "sum"):
        assert np.mean(H.affine_bf16(y32, sc, bi, skip=k) != want) > 0.05, k
    one, zero = np.ones(64, np.float32), np.zeros(64, np.float32)
    assert np.array_equal(H.affine_bf16(y32, one, zero), bf16(y32))
    t, B = H.exact_lora(rng, y, 8, 8, 2)
    assert t.shape == (8, 16) and B.shape == (64, 8) and np.abs(t).max() <= 8
    d = H.lora_delta(t, B, 8, 2)
    cols = np.arange(64)
    lo = H.lora_bf16(y32, d, H.LORA_SCALING, cols)
    assert np.array_equal(lo, bf16(bf16(y32) + bf16(bf16(d.astype(np.float32)) * np.float32(0.75))))
    for k in ("y", "d", "ds"):
        assert np.mean(H.lora_bf16(y32, d, H.LORA_SCALING, cols, skip=k) != lo) > 0.05, k
    half = H.lora_bf16(y32, d[:, :32], H.LORA_SCALING, cols[:32])
    assert np.array_equal(half[:, 32:], bf16(y32)[:, 32:]) and np.array_equal(half[:, :32], lo[:, :32])


@pytest.mark.parametrize("wfmt", GEMV_FMTS)
def test_gemv_affine_conditions(wfmt):
    for M in rows_of(ROWS):
        E.linear_v2_refs(wfmt, M)
        E.resid_v2_refs(wfmt, M)
    for M in rows_of(NORM_ROWS):
        E.norm_linear_v2_refs(wfmt, M)
    for M in rows_of(E.BIG_ROWS):
        E.resid_v2_big_refs(wfmt, M)
    for M in (1, 8):
        E.long_k_refs(wfmt, M)
    for M in rows_of(SWIGLU_ROWS):
        E.swiglu_v2_refs(wfmt, M)


@pytest.mark.parametrize("C", E.QKV_C)
@pytest.mark.parametrize("wfmt", GEMV_FMTS)
def test_gemv_qkv_conditions(wfmt, C):
    for rows in rows_of(QKV_ROWS):
        E.qkv_v2_refs(wfmt, C, rows)
        E.lora_refs(wfmt, C, rows)


@pytest.mark.parametrize("wfmt", [0, 1, 3])
def test_attention_merge_conditions(wfmt):
    for nsplit in (2, 4):
        for affine in (True, False):
            E.merge_refs(wfmt, nsplit, affine)


@pytest.mark.parametrize("wfmt", [0, 3])
def test_multi_tile_conditions(wfmt):
    for M in (7, 8):
        for k in (1, 2, 3):
            E.multi_tile_refs(wfmt, M, 16 * (k * CUS + 1), k == 1)
    E.lora_multi_tile_refs(wfmt)
    E.np_weight.cache_clear()


@pytest.mark.parametrize("wfmt", GEMM_FMTS)
def test_gemm_conditions(wfmt):
    for M in sorted({v[2] for v in E._GV if v[1] == wfmt}):
        E.gemm_v2_refs(wfmt, M)
    for C in (128, 256):
        for B, T_, S, p0 in E.GEMM_QKV:
            E.gemm_qkv_refs(wfmt, C, B, T_, S, p0)


def test_any_shape_conditions():
    for dt in (0, 1):
        for kind in E.G_KINDS:
            for with_resid in (False, True):
                E.g_v2_refs(kind, dt, with_resid)
            E.g_lora_refs(kind, dt)
