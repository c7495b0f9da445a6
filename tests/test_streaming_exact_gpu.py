"""Exact-input tests of the streaming kernels every real model runs on (GPU only): the weight-streaming
GEMV family (csrc/gemv_impl.h), the prefill GEMMs (csrc/gemm.hip) and the decode / flash attention
kernels (csrc/attention.h, csrc/attention_prefill.hip), each against integer numpy with tolerance zero (values
compared as bf16 numbers: +0 and -0 count as equal).

Technique (tests/helpers.py "exact operands"): activations are small integers (|a| <= 4) in bf16, codes and
zeros integers over their full range, scales powers of two (2^-9 .. 2^-3, per column or per (group,
column)), bf16 weights 8-bit integers times 2^-e. Then every product and every fp32 partial sum -- per
chunk, per wave, per group, per K slice, in any order, with the offset removed as s * (acc - (128 + z) *
rowsum), as bf16((q - z) * s) fragments or with the scale in the epilogue -- is an exact dyadic number, so a
correct kernel has one bf16 bit pattern to produce: bf16(sum_k a (q - z) s), computed here in float64 on
integer arrays. Outputs are compared as bf16 values (the sign of a zero aside) and every buffer starts
from a sentinel pattern that rows >= M, padding columns and untouched cache slots must keep bitwise.

Input conditions, all asserted on the CPU before a launch, decided by the references alone (figures: the
inputs of this file):
  * sum_k |a| * cmax < 2^24 (cmax 143 int4, 2431 gptq.int8, max |w| bf16; grouped int4 also with a column's
    largest |q - z| s over its smallest scale, 15 * 64, which one fp32 accumulator must span). 2^24 over the
    largest figure, K = 128 / 640 / 1152 / 8192: int4 364 / 78 / 44 / 11.8; bf16 418 / 88 / 50 / 13.4;
    gptq.int8 21.6 / 4.6 / 2.6 / 3.4 (K = 8192: |a| = 1 on a quarter of the positions, four phases that
    cover every k; |a| <= 2 for the others); grouped int4 365 / 11.5 / 6.5 / 1.76. GEMM shapes: >= 4.5.
  * test power: 25 - 90 % of a test's expected elements need rounding (more than 8 significant bits;
    floor MIN_INEXACT). Where a test pins a rounding point it builds the wrong-rounding result too and
    asserts that it differs in >= 10 % of the elements: residual bf16(x0 + y) 0.12 - 0.31 (GEMV, per shape of
    K >= 640 with >= 96 elements and pooled over them; the int4 formats at K = 128 cannot meet it, see
    test_linear_resid_exact), 0.11 - 0.27 (GEMM); RoPE of the unrounded y 0.10 - 0.41 (one row of C = 128 is 0.1 on average: the first
    of 16 seeds whose references meet the condition is taken, seed 0 or 1 here).
  * fused RMSNorm: rows +-c_m (c_m in 0.5, 1, 2) give rstd = 1 / c_m through rms_rstd's bf16 chain.
  * nstat_out: bitwise wherever the 16-term fp32 sum is exact in any order (71 % of the tile sums of the
    fractional-x0 cases, all of them in test_resid_nstat_out_exact), 16 roundings elsewhere.
  * SwiGLU: silu goes through __expf, so each element must be one of the two products with the bf16
    neighbours of float64 silu(bf16(y1)) (per launch), and over the elements of a test's launches (at least
    112: one decode row over three shapes, where it means all of them) >= 99 % the one from the nearer
    neighbour (measured 100 %); numpy float32 silu disagrees with the float64 nearest rounding in 0 of the
    elements used here (cap 1 %).
  * attention, selected key: (q.K[target] - max_other q.K[s]) / sqrt(hs) >= 110; measured 256 (hs 64,
    S 256), 208 - 272 (hs 64, S 2048), 441 - 475 (hs 128, S 2048), 192 (hs 64, S 512), at least 192 overall:
    every other weight is exactly 0 in fp32.
  * LLM.int8 (wfmt 2): power-of-two SCA / 127 and SCB / 127 make the dequantization constant exact, so Part C
    is bitwise too (tests/test_int8_exact_gpu.py covers the rest of that family).

611 cases, 12 s for the file on an MI355X (the slowest case 0.4 s).

Mutations of the kernels that this file catches (scratch builds, each run once on the GPU): `t` and `grp`
swapped in the int4 kofs; a wave's last chunk skipped; the inner round_bf(y) of the residual epilogues
removed (GEMV, GEMM, split-K reduce); round_bf(y) before RoPE removed; the square in nstat_out left
unrounded; silu of the unrounded a1; decode attention's visible keys < p instead of <= p; flash prefill's
diagonal mask off by one.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

from lit_llama import _hip
from tests import helpers as H
from tests.helpers import bf16
from tests.test_kernels_gpu import GLDS_TILES, T, call, option, repack, repack8, st, sz_grouped, sz_of

pytestmark = pytest.mark.gpu
dev = "cuda"

W4G_128, W4G_256 = 4 | (1 << 8), 4 | (2 << 8)
ZINT4 = _hip.WF_ZINT
GEMV_FMTS = [0, 1, 3, W4G_128, W4G_256]
GEMM_FMTS = [0, ZINT4, 1, 3, W4G_128, W4G_256]
SENT = H.SENTINEL
f32 = np.float32


def P(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------ operands and buffers
@functools.lru_cache(maxsize=None)
def np_weight(wfmt, N, K, seed=0, e_lo=3, e_hi=9):
    return H.exact_weight(np.random.default_rng([wfmt & 0xFFFF, N, K, seed]), wfmt, N, K, e_lo, e_hi)


_dev_weights = {}


def dev_weight(hip, wfmt, N, K, seed=0, e_lo=3, e_hi=9):
    """(host dict, device weight operand, device sz) of the exact weight (wfmt, N, K, seed)."""
    key = (wfmt & 0xFFFF, N, K, seed, e_lo, e_hi)
    w = np_weight(wfmt, N, K, seed, e_lo, e_hi)
    if key not in _dev_weights:
        wf = wfmt & 0xFF
        if wf == 1:
            d = (T(w["wb"], torch.bfloat16), None)
        elif wf == 3:
            d = (repack8(hip, w["qw"]), sz_of(hip, w["scales"], w["zeros"], 8))
        elif wf == 4:
            d = (repack(hip, w["qw"]), sz_grouped(hip, w["scales"], w["zeros"]))
        else:
            d = (repack(hip, w["qw"]), sz_of(hip, w["scales"], w["zeros"]))
        torch.cuda.synchronize()
        _dev_weights[key] = d
    return (w,) + _dev_weights[key]


def sentinel(*shape):
    """A bf16 buffer (as int16 words) holding the sentinel pattern everywhere."""
    return torch.full(shape, SENT, dtype=torch.int16, device=dev)


def put(buf, vals, r0=0):
    """Exact bf16 values into the top-left corner of a sentinel buffer (rows from r0)."""
    vals = np.asarray(vals, f32)
    assert np.array_equal(bf16(vals), vals), "operand is not a bf16 value"
    buf[r0:r0 + vals.shape[0], :vals.shape[1]] = T(vals, torch.bfloat16).view(torch.int16)
    return buf


def a_operand(a, lda):
    """Activation rows at row stride lda; the padding columns hold 1000 (reading them breaks the result)."""
    M, K = a.shape
    buf = torch.full((M, lda), 1000.0, dtype=torch.bfloat16, device=dev).view(torch.int16)
    return put(buf, a)


def words(t):
    return t.cpu().numpy().view(np.uint16)


def check(buf, want, what):
    """buf (2-D sentinel buffer) holds `want` (bf16 values as float32) in its top-left corner and the
    sentinel everywhere else."""
    b = words(buf)
    want = np.asarray(want, f32)
    live = np.zeros(b.shape, bool)
    live[:want.shape[0], :want.shape[1]] = True
    assert (b[~live] == SENT).all(), f"{what}: {(b[~live] != SENT).sum()} words written outside the result"
    got = H.f32_of_bits(b[live]).reshape(want.shape)
    assert not np.isnan(got).any(), f"{what}: {np.isnan(got).sum()} / {got.size} elements not written (or NaN)"
    bad = got != want
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {bad.sum()} / {bad.size} elements differ; first at {i}: got {got[i]!r}, "
                             f"want {want[i]!r}")


class stream_a:
    """llj_set_stream_a for the duration of a `with` block."""

    def __init__(self, hip, mode):
        self.hip, self.mode = hip, mode

    def __enter__(self):
        self.old = self.hip.llj_set_stream_a(self.mode)

    def __exit__(self, *exc):
        self.hip.llj_set_stream_a(self.old)


def want_of(y):
    """bf16 of an exact float64 result (exact in fp32 first: asserted)."""
    y32 = y.astype(f32)
    assert np.array_equal(y32.astype(np.float64), y), "the exact result does not fit fp32"
    return bf16(y32)


def hand_nstat(c, K, M):
    """Three uneven partial sums of squares per row, adding up to K c_m^2 exactly (npart = 3)."""
    tot = K * c.astype(np.float64) ** 2
    part = np.zeros((3, 16), f32)
    part[0, :M] = tot / 2
    part[1, :M] = tot / 4 + c ** 2
    part[2, :M] = tot / 4 - c ** 2
    assert np.array_equal(part.astype(np.float64).sum(0)[:M], tot)
    return part


# ================================================================== Part A: the GEMV family
# (rows, llj_set_stream_a): AM_LDS one row; AM_STREAM one row; AM_STREAM 2..8; the LDS-image forms at
# 2..8 rows; AM_GLOBAL (8 waves) at 9 and 16 rows
ROWS = [(1, 1), (1, 2), (2, 1), (7, 1), (8, 1), (2, 0), (7, 0), (8, 0), (9, 1), (16, 1)]
# K = 128: one chunk (three of four waves idle); 640: 5 chunks, uneven over 4 waves, ragged last group at
# g = 256; 1152: 9 chunks over 8 waves
NK = [(16, 128), (48, 128), (16, 640), (48, 640), (16, 1152), (48, 1152)]
MIN_INEXACT = 0.2  # floor on the share of a test's expected elements that need rounding


def linear_case(wfmt, M, N, K, seed=0, amax=4):
    w = np_weight(wfmt, N, K)
    a = H.exact_acts(np.random.default_rng([7, wfmt & 0xFFFF, M, N, K, seed]), M, K, amax)
    H.assert_exact_condition(a, w, f"wfmt {wfmt} M {M} N {N} K {K}")
    y = H.exact_linear(a, w)
    return a, y


@pytest.mark.parametrize("M,stream", ROWS)
@pytest.mark.parametrize("wfmt", GEMV_FMTS)
def test_linear_exact(hip, wfmt, M, stream):
    """llj_linear on every A path of pick_am / launch, bitwise bf16(sum_k a (q - z) s); lda > K and
    ldc > N at N = 48."""
    ys = []
    with stream_a(hip, stream):
        for N, K in NK:
            a, y = linear_case(wfmt, M, N, K)
            ys.append(y.ravel())
            _, Wd, szd = dev_weight(hip, wfmt, N, K)
            lda, ldc = (K + 8, N + 6) if N == 48 else (K, N)
            ad, out = a_operand(a, lda), sentinel(16, ldc)
            call(hip, "llj_linear", wfmt, ad.data_ptr(), lda, Wd.data_ptr(), P(szd), None, out.data_ptr(), ldc, M, N,
                 K, None, 0, None, st())
            torch.cuda.synchronize()
            check(out, want_of(y), f"linear wfmt {wfmt} M {M} N {N} K {K} stream_a {stream}")
    share = H.inexact_share(np.concatenate(ys))  # over the six shapes (M = 1, N = 16 alone is 16 elements)
    print("share of expected elements that need rounding:", round(share, 3))
    assert share >= MIN_INEXACT, share


@pytest.mark.parametrize("M", [1, 5, 16])
def test_linear_bf16_bias_exact(hip, M):
    """bf16 weights with a bias (integers times the column's 2^-e: y + bias stays exact in fp32)."""
    N, K = 48, 640
    a, y = linear_case(1, M, N, K)
    w, Wd, _ = dev_weight(hip, 1, N, K)
    bias = (np.random.default_rng(M).integers(-100, 101, size=N) * 2.0 ** -w["e"]).astype(f32)
    assert np.array_equal(bf16(bias), bias)
    out = sentinel(16, N)
    ad = a_operand(a, K)
    call(hip, "llj_linear", 1, ad.data_ptr(), K, Wd.data_ptr(), None, T(bias, torch.bfloat16).data_ptr(),
         out.data_ptr(), N, M, N, K, None, 0, None, st())
    torch.cuda.synchronize()
    check(out, want_of(y + bias[None, :].astype(np.float64)), f"bf16 linear with bias M {M}")


@pytest.mark.parametrize("M,stream", [(1, 1), (5, 1), (5, 0), (12, 1)])
def test_linear_int4_rowsum_operand_exact(hip, M, stream):
    """int4 with the caller's row sums (the `rowsum` operand: exact integers) for the offset term."""
    N, K = 48, 640
    a, y = linear_case(0, M, N, K)
    _, Wd, szd = dev_weight(hip, 0, N, K)
    rs = T(a.sum(1).astype(f32))
    out, ad = sentinel(16, N), a_operand(a, K)
    with stream_a(hip, stream):
        call(hip, "llj_linear", 0, ad.data_ptr(), K, Wd.data_ptr(), szd.data_ptr(), None, out.data_ptr(), N, M, N, K,
             None, 0, rs.data_ptr(), st())
    torch.cuda.synchronize()
    check(out, want_of(y), f"int4 linear with rowsum M {M} stream_a {stream}")


def resid_case(wfmt, M, N, K, big_x0=False, seed=0, amax=4, density=1.0, phase=0):
    """x0, exact y, expected x, the wrong-rounding x, and the expected nstat_out (float64 tile sums of
    bf16(x^2)) with the mask of the sums that are exact in fp32 in any order."""
    w = np_weight(wfmt, N, K)
    rng = np.random.default_rng([11, wfmt & 0xFFFF, M, N, K, seed, phase])
    a = H.exact_acts(rng, M, K, amax, density, phase)
    H.assert_exact_condition(a, w, f"resid wfmt {wfmt} M {M} N {N} K {K}")
    y = H.exact_linear(a, w)
    if big_x0:  # |x0| in [b, 2 b) with b >= 4 max |y|: the squares of a tile span three binades whatever y adds
        b = 2.0 ** (np.ceil(np.log2(np.abs(y).max())) + 2)
        x0 = (rng.choice([-1.0, 1.0], size=(M, N)) * (b + b / 128 * rng.integers(0, 128, size=(M, N)))).astype(f32)
    else:  # fractional, of the size of y's rounding step
        x0 = (rng.integers(-256, 257, size=(M, N)) / 64.0).astype(f32)
    assert np.array_equal(bf16(x0), x0)
    y32 = y.astype(f32)
    assert np.array_equal(y32.astype(np.float64), y)
    want = bf16(x0 + bf16(y32))  # fp32 add, as the kernel's
    wrong = bf16(x0 + y32)
    sq = bf16(want * want)
    return dict(a=a, x0=x0, y=y, want=want, wrong=wrong, nstat=sq.astype(np.float64).reshape(M, N // 16, 16).sum(-1),
                nstat_exact=H.exact_sum_mask(sq))


def run_resid(hip, wfmt, c, M, N, K, lda, ldx):
    _, Wd, szd = dev_weight(hip, wfmt, N, K)
    ad, x = a_operand(c["a"], lda), put(sentinel(16, ldx), c["x0"])
    nst = torch.full((N // 16, 16), float("nan"), dtype=torch.float32, device=dev)
    call(hip, "llj_linear_resid", wfmt, ad.data_ptr(), lda, Wd.data_ptr(), P(szd), x.data_ptr(), ldx, M, N, K, None, 0,
         nst.data_ptr(), st())
    torch.cuda.synchronize()
    return x, nst.cpu().numpy()


def check_nstat(got, c, M, what, all_exact=False):
    """nstat_out[t * 16 + m]: bitwise the fp32 sum of tile t's bf16(x^2) where that sum is exact in any
    order, within 16 fp32 roundings of positive terms elsewhere; slots of rows >= M untouched."""
    assert np.isnan(got[:, M:]).all(), f"{what}: nstat_out slots of rows >= M written"
    g, ref, ex = got[:, :M].T.astype(np.float64), c["nstat"], c["nstat_exact"]
    if all_exact:
        assert ex.all(), f"{what}: {(~ex).sum()} tile sums are not exact (an input condition)"
    assert np.array_equal(g[ex], ref[ex]), f"{what}: {(g[ex] != ref[ex]).sum()} / {ex.sum()} exact tile sums differ"
    np.testing.assert_allclose(g[~ex], ref[~ex], rtol=16 * 2.0 ** -24, atol=0, err_msg=what)
    return float(ex.mean())


@pytest.mark.parametrize("M,stream", ROWS)
@pytest.mark.parametrize("wfmt", GEMV_FMTS)
def test_linear_resid_exact(hip, wfmt, M, stream):
    """llj_linear_resid pins x = bf16(x0 + bf16(y)) with x0 fractional. The result without the inner rounding,
    bf16(x0 + y), must differ in >= 10 % of the elements: asserted per shape wherever a launch has >= 96
    elements and its sums need rounding (K >= 640, measured 0.12 .. 0.31; bf16 and gptq.int8 weights also at
    K = 128, 0.19 .. 0.29), and over the pooled elements of the four K >= 640 shapes for every row count (0.12
    .. 0.30; one row of N = 16 is 16 elements). The int4 formats at K = 128 cannot meet it: 128 terms of
    |a (q - z)| <= 60 sum to fewer than 256 units for most elements, which bf16 holds exactly (0 .. 0.19);
    those launches cover the path and the sentinel, not the rounding point. nstat_out is bitwise the fp32
    tile sums of bf16(x^2) wherever those are exact in any order (71 % of the tiles here; all of them in
    test_resid_nstat_out_exact)."""
    wr, ex, per = [], [], {}
    with stream_a(hip, stream):
        for N, K in NK:
            c = resid_case(wfmt, M, N, K)
            diff = (c["want"] != c["wrong"]).ravel()
            per[(N, K)] = round(float(diff.mean()), 3)
            if K >= 640:
                wr.append(diff)
            lda, ldx = (K + 8, N + 6) if N == 48 else (K, N)
            x, nst = run_resid(hip, wfmt, c, M, N, K, lda, ldx)
            what = f"resid wfmt {wfmt} M {M} N {N} K {K} stream_a {stream}"
            if diff.size >= 96 and (K >= 640 or wfmt in (1, 3)):
                assert diff.mean() >= 0.10, (what, per)
            check(x, c["want"], what)
            ex.append(check_nstat(nst, c, M, what))
    wr = float(np.mean(np.concatenate(wr)))  # over the four shapes with K >= 640
    print("wrong-rounding difference share:", round(wr, 3), "per (N, K):", per, "exact nstat tiles per shape:",
          np.round(ex, 2))
    assert wr >= 0.10, wr


@pytest.mark.parametrize("M,stream", [(1, 1), (2, 1), (8, 1), (8, 0), (16, 1)])
@pytest.mark.parametrize("wfmt", GEMV_FMTS)
def test_resid_nstat_out_exact(hip, wfmt, M, stream):
    """nstat_out with |x0| in [b, 2 b), b >= 4 max |y|: every tile sum of bf16(x^2) is exact in fp32, so each slot has one
    bit pattern. Without the bf16 rounding of the square the sums differ (asserted on the CPU)."""
    N, K = 48, 640
    c = resid_case(wfmt, M, N, K, big_x0=True)
    unrounded = (c["want"].astype(np.float64) ** 2).reshape(M, N // 16, 16).sum(-1)
    assert np.mean(unrounded != c["nstat"]) >= 0.9
    with stream_a(hip, stream):
        x, nst = run_resid(hip, wfmt, c, M, N, K, K, N)
    check(x, c["want"], f"resid (large x0) wfmt {wfmt} M {M}")
    check_nstat(nst, c, M, f"nstat_out wfmt {wfmt} M {M} stream_a {stream}", all_exact=True)


@pytest.mark.parametrize("M", [1, 8])
@pytest.mark.parametrize("wfmt", GEMV_FMTS)
def test_long_k_residual_eight_waves_exact(hip, wfmt, M):
    """llj_linear_resid at K = 8192 (8-wave workgroups), N = 32: |a| <= 2; gptq.int8 takes |a| = 1 on a quarter
    of the positions (sum |a| * 2431 = 5.0 M < 2^24), four phases so that the supports cover every k."""
    N, K = 32, 8192
    for phase in range(4 if wfmt == 3 else 1):
        c = resid_case(wfmt, M, N, K, amax=1 if wfmt == 3 else 2, density=0.25 if wfmt == 3 else 1.0, phase=phase)
        x, nst = run_resid(hip, wfmt, c, M, N, K, K + 8, N)
        what = f"resid K 8192 wfmt {wfmt} M {M} phase {phase}"
        check(x, c["want"], what)
        check_nstat(nst, c, M, what)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("M", [7, 8])
@pytest.mark.parametrize("wfmt", [0, 3])
def test_multi_tile_workgroups_exact(hip, wfmt, M, k):
    """N = 16 (k CUs + 1) tiles: k + 1 tiles per workgroup with a partial last workgroup (llj_linear,
    streamed A and the LDS image; the residual op, which takes at most 2, at k = 1)."""
    N, K = 16 * (k * _cus() + 1), 128
    a, y = linear_case(wfmt, M, N, K)
    _, Wd, szd = dev_weight(hip, wfmt, N, K)
    for stream in (1, 0):
        with stream_a(hip, stream):
            ad, out = a_operand(a, K), sentinel(M + 1, N)
            call(hip, "llj_linear", wfmt, ad.data_ptr(), K, Wd.data_ptr(), P(szd), None, out.data_ptr(), N, M, N, K,
                 None, 0, None, st())
            torch.cuda.synchronize()
            check(out, want_of(y), f"multi-tile linear wfmt {wfmt} M {M} N {N} stream_a {stream}")
            if k == 1:
                c = resid_case(wfmt, M, N, K)
                x, nst = run_resid(hip, wfmt, c, M, N, K, K, N)
                check(x, c["want"], f"multi-tile resid wfmt {wfmt} M {M} N {N} stream_a {stream}")
                check_nstat(nst, c, M, f"multi-tile nstat_out wfmt {wfmt} M {M}")
    _dev_weights.pop((wfmt & 0xFFFF, N, K, 0, 3, 9), None)  # (the one large operand of this file)


# ---- the norm-fused forms. (rows, llj_set_stream_a, nstat): AM_NORM one row / 2..8 rows (nstat NULL);
# AM_SNORM 2..8 rows and, with llj_set_stream_a(2), one row; the LDS image normalized from nstat; nstat
# from a preceding llj_linear_resid's nstat_out
NORM_ROWS = [(1, 1, None), (2, 1, None), (8, 1, None), (2, 1, "hand"), (7, 1, "hand"), (8, 1, "hand"), (1, 2, "hand"),
             (2, 0, "hand"), (8, 0, "hand"), (3, 1, "resid"), (8, 1, "resid")]


def norm_case(wfmt, M, N, K, seed=0, e_lo=3, e_hi=9, gvals=tuple(range(-4, 5))):
    rng = np.random.default_rng([13, wfmt & 0xFFFF, M, N, K, seed])
    x, g, opnd, c = H.norm_rows(rng, M, K, gvals)
    w = np_weight(wfmt, N, K, seed, e_lo, e_hi)
    H.assert_exact_condition(opnd, w, f"norm wfmt {wfmt} M {M} N {N} K {K}")
    return x, g, c, H.exact_linear(opnd, w)


def nstat_operand(hip, kind, x, c, K, M):
    """(device nstat, npart) for the rows x: None; three hand-made partials; or the nstat_out of a
    llj_linear_resid that produced x (zero activations: x = bf16(x0 + 0), K / 16 partials of 16 c^2)."""
    if kind is None:
        return None, 0, None
    if kind == "hand":
        return T(hand_nstat(c, K, M)), 3, None
    _, Wd, szd = dev_weight(hip, 1, K, 128)
    a0 = a_operand(np.zeros((M, 128), f32), 128)
    xd = put(sentinel(16, K), x)
    nst = torch.full((K // 16, 16), float("nan"), dtype=torch.float32, device=dev)
    call(hip, "llj_linear_resid", 1, a0.data_ptr(), 128, Wd.data_ptr(), None, xd.data_ptr(), K, M, K, 128, None, 0,
         nst.data_ptr(), st())
    torch.cuda.synchronize()
    check(xd, x, "resid of zero activations")
    want = np.full((K // 16, 16), np.nan)
    want[:, :M] = 16.0 * c.astype(np.float64) ** 2
    np.testing.assert_array_equal(nst.cpu().numpy().astype(np.float64), want)
    return nst, K // 16, xd


@pytest.mark.parametrize("M,stream,nstat", NORM_ROWS)
@pytest.mark.parametrize("wfmt", GEMV_FMTS)
def test_norm_linear_exact(hip, wfmt, M, stream, nstat):
    """llj_norm_linear: rows +-c_m normalize to +-1 exactly, so the MFMA operand is sign(x) * norm_w."""
    with stream_a(hip, stream):
        for N, K in [(16, 128), (48, 640), (16, 1152)]:
            x, g, c, y = norm_case(wfmt, M, N, K)
            _, Wd, szd = dev_weight(hip, wfmt, N, K)
            nst, npart, xd = nstat_operand(hip, nstat, x, c, K, M)
            xd = put(sentinel(M, K), x) if xd is None else xd
            ldo = N + 6 if N == 48 else N
            out, gd = sentinel(16, ldo), T(g, torch.bfloat16)
            call(hip, "llj_norm_linear", wfmt, xd.data_ptr(), gd.data_ptr(), 1e-5, Wd.data_ptr(), P(szd), out.data_ptr(),
                 ldo, M, N, K, None, 0, None, P(nst), npart, st())
            torch.cuda.synchronize()
            check(out, want_of(y), f"norm_linear wfmt {wfmt} M {M} N {N} K {K} stream_a {stream} nstat {nstat}")


QKV_G = (-4, -3, 3, 4)  # norm weights of the QKV cases: large enough that K = 128 int4 sums need rounding
QKV_ROWS = [(1, 1, None), (8, 1, None), (8, 1, "hand"), (8, 0, "hand"), (1, 2, "hand"), (10, 1, None), (10, 1, "hand")]


def qkv_expect(y, B, T_, nh, hs, S, pos, rope, q0=None, k0=None, v0=None, exact=True):
    """Expected q (B T, C) and caches (B, nh, S, hs) as float32 with NaN where the sentinel must stay, from
    the exact c_attn output y (B T, 3 C); ring slot pos % S; the wrong-rounding variant rotates y itself.
    exact False (tests/test_epilogue_exact_gpu.py): the rotation of partners of very different size need not fit
    fp32; both products are exact in fp32 (8 x 4 significant bits), so the fp32 result is the one rounding of the
    exact value however the two products are contracted, which is what rope_bf16 computes."""
    C, Mr = nh * hs, B * T_
    v = bf16(y.astype(f32))
    cs = rope[np.asarray(pos)][None, :, None]  # (1, T, 1, hs / 2, 2)

    def split(z):
        return [z[:, i * C:(i + 1) * C].reshape(B, T_, nh, hs) for i in range(3)]

    q, k, vv = split(v)
    qe, ke = H.rope_bf16(q, cs, exact), H.rope_bf16(k, cs, exact)
    qu, ku, _ = split(y)
    wrong_share = float(np.mean(np.concatenate([(H.rope_bf16(qu, cs, exact=False) != qe).ravel(),
                                                (H.rope_bf16(ku, cs, exact=False) != ke).ravel()])))
    kc = np.full((B, nh, S, hs), np.nan, f32)
    vc = np.full((B, nh, S, hs), np.nan, f32)
    for t in range(T_):
        kc[:, :, pos[t] % S] = ke[:, t]
        vc[:, :, pos[t] % S] = vv[:, t]
    return qe.reshape(Mr, C), kc, vc, wrong_share


def check_cache(buf, want, what):
    """A cache buffer against float32 `want` whose NaN entries mark slots that keep the sentinel."""
    b = words(buf).reshape(want.shape)
    keep = np.isnan(want)
    assert (b[keep] == SENT).all(), f"{what}: {(b[keep] != SENT).sum()} untouched cache words overwritten"
    got = H.f32_of_bits(b[~keep])
    assert not np.isnan(got).any(), f"{what}: cache slots not written"
    bad = got != want[~keep]
    assert not bad.any(), f"{what}: {bad.sum()} / {bad.size} cache elements differ"


@pytest.mark.parametrize("rows,stream,nstat", QKV_ROWS)
@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("wfmt", GEMV_FMTS)
def test_norm_qkv_rope_exact(hip, wfmt, C, rows, stream, nstat):
    """llj_norm_qkv_rope with 2 heads of 64 / 128 and a dyadic RoPE table: q, k = bf16(v cos -+ partner sin)
    from v = bf16(y). Rotating the unrounded y instead differs in >= 10 % of the q / k elements (measured
    0.10 .. 0.41). B x T = 1, 8, 2 x 5 (two row chunks); positions past S land in slot pos % S; the whole q
    buffer and both whole caches are compared (untouched slots keep the sentinel)."""
    nh, S = 2, 8
    hs = C // nh
    B, T_ = (2, 5) if rows == 10 else (rows, 1)
    pos = np.arange(6, 11, dtype=np.int32) if T_ == 5 else np.array([13], np.int32)  # slots 6, 7, 0, 1, 2 / 5
    rng = np.random.default_rng([17, wfmt & 0xFFFF, C, rows])
    rope = H.dyadic_rope(rng, 16, hs)
    for seed in range(16):  # the first inputs whose two references differ enough (one row of C = 128: ~0.1 on average)
        x, g, c, y = norm_case(wfmt, rows, 3 * C, C, seed=seed, gvals=QKV_G)
        qe, kce, vce, wrong = qkv_expect(y, B, T_, nh, hs, S, pos, rope)
        if wrong >= 0.10:
            break
    print("wrong-rounding difference share:", round(wrong, 3), "seed", seed)
    assert wrong >= 0.10, wrong
    _, Wd, szd = dev_weight(hip, wfmt, 3 * C, C, seed=seed)
    xd, gd, rd, pd = put(sentinel(rows, C), x), T(g, torch.bfloat16), T(rope), T(pos)
    q, kc, vc = sentinel(rows + 1, C), sentinel(B * nh * S, hs), sentinel(B * nh * S, hs)
    # the op reads nstat + row0: the partials of row m of the B T rows sit in slot m of each 16-float line
    nst = None if nstat is None else T(hand_nstat(c, C, rows))
    with stream_a(hip, stream):
        for r0 in range(0, rows, 8):
            r = min(8, rows - r0)
            call(hip, "llj_norm_qkv_rope", wfmt, xd.data_ptr(), gd.data_ptr(), 1e-5, Wd.data_ptr(), P(szd), q.data_ptr(),
                 kc.data_ptr(), vc.data_ptr(), rd.data_ptr(), pd.data_ptr(), B, T_, C, nh, S, r0, r, None, None, P(nst),
                 3 if nst is not None else 0, st())
    torch.cuda.synchronize()
    check(q, qe, f"q wfmt {wfmt} C {C} rows {rows}")
    check_cache(kc, kce, f"k cache wfmt {wfmt} C {C} rows {rows}")
    check_cache(vc, vce, f"v cache wfmt {wfmt} C {C} rows {rows}")


def swiglu_e(wfmt):
    """Scale exponents of the SwiGLU weights: powers of two that keep |y1| within a few units, where silu
    is not the identity (int4 2^-9 .. 2^-6; gptq.int8, whose sums are 16 times larger, 2^-13 .. 2^-10; bf16
    weights 2^-12 .. 2^-9)."""
    return {1: (12, 15), 3: (10, 13)}.get(wfmt & 0xFF, (6, 9))


class SwigluPool:
    """The SwiGLU rule (helpers.swiglu_candidates) over the launches of one test. add(): the sentinel around a
    launch's result and the two-candidate rule, per launch. finish(): over the pooled elements, silu is not
    trivial (|a1| <= 16, the two neighbours differ), numpy float32 silu disagrees with the float64 nearest
    rounding in under 1 %, and >= 99 % of the elements come from the nearer neighbour."""

    def __init__(self):
        self.near, self.tie, self.small, self.two = [], [], [], []

    def add(self, buf, y1, y2, what, a1=None):
        """buf: a sentinel buffer with the result in its top-left corner; a1: the bf16 c_fc1 output when it is
        an input (llj_gemm_silu_mul) instead of bf16(y1)."""
        lo, hi, near, a1 = H.swiglu_candidates(y1 if a1 is None else a1.astype(np.float64), y2)
        b = words(buf)
        live = np.zeros(b.shape, bool)
        live[:lo.shape[0], :lo.shape[1]] = True
        assert (b[~live] == SENT).all(), f"{what}: words written outside the result"
        got = H.f32_of_bits(b[live]).reshape(lo.shape)
        assert not np.isnan(got).any(), f"{what}: elements not written (or NaN)"
        ok = (got == lo) | (got == hi)
        assert ok.all(), f"{what}: {(~ok).sum()} / {ok.size} elements are neither neighbour's product"
        # numpy float32 silu against the float64 nearest rounding: how often a correct fp32 silu leaves the nearer one
        s32 = bf16((a1 / (f32(1) + np.exp(-a1))).astype(f32))
        self.tie.append((s32 != H.bf16_neighbours(H.silu64(a1))[2]).ravel())
        self.near.append((got == near).ravel())
        self.small.append((np.abs(a1) <= 16).ravel())
        self.two.append((lo != hi).ravel())

    def finish(self, what):
        near, tie, small, two = (float(np.mean(np.concatenate(v))) for v in (self.near, self.tie, self.small, self.two))
        print(f"{what}: {sum(v.size for v in self.near)} elements, nearer-neighbour share {near:.4f}, "
              f"float32-silu disagreement {tie:.4f}")
        assert tie < 0.01, f"{what}: float32 silu disagrees with the float64 nearest rounding in {tie:.4f}"
        assert small > 0.9 and two > 0.5, f"{what}: silu is trivial here"
        assert near >= 0.99, f"{what}: only {near:.4f} of the elements come from the nearer bf16 neighbour of silu"


def check_swiglu(buf, y1, y2, what, a1=None):
    pool = SwigluPool()
    pool.add(buf, y1, y2, what, a1)
    pool.finish(what)


SWIGLU_ROWS = [(1, 1, None), (2, 1, None), (8, 1, None), (8, 1, "hand"), (1, 2, "hand"), (8, 0, "hand"), (8, 1, "resid")]


@pytest.mark.parametrize("M,stream,nstat", SWIGLU_ROWS)
@pytest.mark.parametrize("wfmt", GEMV_FMTS)
def test_norm_swiglu_exact(hip, wfmt, M, stream, nstat):
    """llj_norm_swiglu with exact y1, y2: every element is bf16(s * bf16(y2)) with s one of the two bf16
    neighbours of silu(bf16(y1)), and >= 99 % of the test's elements (three shapes: 112 at one row, where it
    means all of them) take the nearer one (silu of the unrounded y1 does not)."""
    e = swiglu_e(wfmt)
    pool = SwigluPool()
    with stream_a(hip, stream):
        for Hn, K in [(16, 128), (48, 640), (48, 1152)]:
            x, g, c, y1 = norm_case(wfmt, M, Hn, K, 1, *e)
            _, W1, s1 = dev_weight(hip, wfmt, Hn, K, 1, *e)
            w2, W2, s2 = dev_weight(hip, wfmt, Hn, K, 2, *e)
            opnd = g[None, :] * np.sign(x)  # the normalized rows (norm_case asserts it)
            H.assert_exact_condition(opnd, w2)
            y2 = H.exact_linear(opnd, w2)
            nst, npart, xd = nstat_operand(hip, nstat, x, c, K, M)
            xd = put(sentinel(M, K), x) if xd is None else xd
            h, gd = sentinel(9, Hn), T(g, torch.bfloat16)
            call(hip, "llj_norm_swiglu", wfmt, xd.data_ptr(), gd.data_ptr(), 1e-5, W1.data_ptr(), P(s1), W2.data_ptr(),
                 P(s2), h.data_ptr(), M, Hn, K, None, 0, None, P(nst), npart, st())
            torch.cuda.synchronize()
            pool.add(h, y1, y2, f"swiglu wfmt {wfmt} M {M} H {Hn} K {K} stream_a {stream} nstat {nstat}")
    pool.finish(f"swiglu wfmt {wfmt} M {M} stream_a {stream} nstat {nstat}")


# ================================================================== Part B: the prefill GEMMs
GEMM_NK = [(128, 128, 0), (256, 384, 8), (384, 640, 2)]  # (N, K, ldc - N): 16-byte, LDS-staged and 4-byte stores
GEMM_M128 = [1, 17, 128, 129, 255]
GEMM_M256 = [256, 257, 300]


def gemm_variants():
    """(id, wfmt, M, options) of the GEMM cases: every format at the 128-row kernels; at M >= 256 int4 and
    bf16 under the three GLDS_TILES settings, integral-zero int4 with LLJ_OPT_GEMM_W4Z 1 and 0, the rest as is."""
    out = []
    for M in GEMM_M128:
        out += [(f"wfmt{w:#x}-M{M}", w, M, {}) for w in GEMM_FMTS]
    for M in GEMM_M256:
        for w in (0, 1):
            out += [(f"wfmt{w:#x}-M{M}-{name}", w, M, opts) for name, opts in GLDS_TILES.items()]
        out += [(f"zint-M{M}-w4z{v}", ZINT4, M, {_hip.OPT_GEMM_W4Z: v}) for v in (1, 0)]
        out += [(f"wfmt{w:#x}-M{M}", w, M, {}) for w in (3, W4G_128, W4G_256)]
    return out


@contextlib.contextmanager
def options(hip, opts):
    """Several llj_set_option settings for the duration of a `with` block."""
    with contextlib.ExitStack() as stack:
        for k, v in opts.items():
            stack.enter_context(option(hip, k, v))
        yield


_GV = gemm_variants()


@pytest.mark.parametrize("wfmt,M,opts", [v[1:] for v in _GV], ids=[v[0] for v in _GV])
def test_gemm_linear_resid_silu_exact(hip, wfmt, M, opts):
    """llj_gemm_linear, llj_gemm_resid (x0 fractional: bf16(x0 + bf16(y)), which differs from bf16(x0 + y)
    in >= 10 % of the elements over the three shapes) and llj_gemm_silu_mul (the SwiGLU rule, h pre-filled
    with bf16 values on a 1 / 16 grid) on exact operands; lda > K; rows >= M and the padding columns of
    ldc > N keep the sentinel."""
    wr, ys, pool = [], [], SwigluPool()
    with options(hip, opts):
        for N, K, pad in GEMM_NK:
            rng = np.random.default_rng([23, wfmt & 0xFFFF, M, N, K])
            c = resid_case(wfmt, M, N, K)
            a, y = c["a"], c["y"]
            ys.append(y.ravel())
            wr.append((c["want"] != c["wrong"]).ravel())
            _, Wd, szd = dev_weight(hip, wfmt, N, K)
            lda, ldc = K + 8, N + pad
            ad = a_operand(a, lda)
            what = f"gemm wfmt {wfmt:#x} M {M} N {N} K {K} {opts}"
            out = sentinel(M + 2, ldc)
            call(hip, "llj_gemm_linear", wfmt, ad.data_ptr(), lda, Wd.data_ptr(), P(szd), out.data_ptr(), ldc, M, N, K, st())
            xr = put(sentinel(M + 2, ldc), c["x0"])
            call(hip, "llj_gemm_resid", wfmt, ad.data_ptr(), lda, Wd.data_ptr(), P(szd), xr.data_ptr(), ldc, M, N, K, st())
            e = swiglu_e(wfmt)
            w2, W2d, s2d = dev_weight(hip, wfmt, N, K, 2, *e)
            a1 = (rng.integers(-256, 257, size=(M, N)) / 16.0).astype(f32)  # |a1| <= 16 on a 1 / 16 grid
            h = put(sentinel(M + 2, ldc), a1)
            call(hip, "llj_gemm_silu_mul", wfmt, ad.data_ptr(), lda, W2d.data_ptr(), P(s2d), h.data_ptr(), ldc, M, N, K, st())
            torch.cuda.synchronize()
            check(out, want_of(y), what + " linear")
            check(xr, c["want"], what + " resid")
            H.assert_exact_condition(a, w2, what)
            y2 = H.exact_linear(a, w2)
            pool.add(h, None, y2, what + " silu_mul", a1=a1)
    pool.finish(f"gemm silu_mul wfmt {wfmt:#x} M {M} {opts}")  # (768 elements at M = 1)
    wr, share = float(np.mean(np.concatenate(wr))), H.inexact_share(np.concatenate(ys))
    print("wrong-rounding difference share:", round(wr, 3), "needs rounding:", round(share, 3))
    assert wr >= 0.10 and share >= MIN_INEXACT, (wr, share)


@pytest.mark.parametrize("wfmt", [1, ZINT4])
def test_gemm_resid_split_k_exact(hip, wfmt):
    """llj_gemm_resid_ws at (256, 128, 1024): the K slices' fp32 partials are exact, so the split result is
    bitwise bf16(x0 + bf16(y)) too."""
    M, N, K = 256, 128, 1024
    nb = hip.llj_gemm_resid_ws_bytes(wfmt, M, N, K)
    assert nb > 0, "this shape is expected to split"
    c = resid_case(wfmt, M, N, K)
    assert np.mean(c["want"] != c["wrong"]) >= 0.10
    _, Wd, szd = dev_weight(hip, wfmt, N, K)
    ad, xr = a_operand(c["a"], K + 8), put(sentinel(M + 2, N + 8), c["x0"])
    ws = torch.full((nb // 4,), float("nan"), dtype=torch.float32, device=dev)
    call(hip, "llj_gemm_resid_ws", wfmt, ad.data_ptr(), K + 8, Wd.data_ptr(), P(szd), xr.data_ptr(), N + 8, M, N, K,
         ws.data_ptr(), nb, st())
    torch.cuda.synchronize()
    check(xr, c["want"], f"gemm resid split-K wfmt {wfmt:#x}")


def swiglu_dual_case(M, Hn, K, cols=None):
    e = swiglu_e(0)
    a = H.exact_acts(np.random.default_rng([29, M, Hn, K]), M, K)
    w1, w2 = np_weight(ZINT4, Hn, K, 1, *e), np_weight(ZINT4, Hn, K, 2, *e)
    H.assert_exact_condition(a, w1)
    H.assert_exact_condition(a, w2)
    cols = slice(None) if cols is None else cols
    a64 = a.astype(np.float64)
    return a, a64 @ w1["W"][cols].T, a64 @ w2["W"][cols].T


@pytest.mark.parametrize("Hn", [64, 192])
def test_gemm_swiglu_dual_exact(hip, Hn):
    """llj_gemm_swiglu at (256, H, 128): the smallest H it takes and one that is a multiple of 64 only."""
    M, K = 256, 128
    a, y1, y2 = swiglu_dual_case(M, Hn, K)
    e = swiglu_e(0)
    _, W1, s1 = dev_weight(hip, ZINT4, Hn, K, 1, *e)
    _, W2, s2 = dev_weight(hip, ZINT4, Hn, K, 2, *e)
    ad, h = a_operand(a, K + 8), sentinel(M + 2, Hn + 8)
    call(hip, "llj_gemm_swiglu", ZINT4, ad.data_ptr(), K + 8, W1.data_ptr(), s1.data_ptr(), W2.data_ptr(), s2.data_ptr(),
         h.data_ptr(), Hn + 8, M, Hn, K, st())
    torch.cuda.synchronize()
    check_swiglu(h, y1, y2, f"gemm swiglu dual H {Hn}")


def test_gemm_swiglu_tail_split_exact(hip):
    """llj_gemm_swiglu_ws at M = 256, H = 64 (CUs + 4), K = 1024: the tail column tiles (two K halves through
    the fp32 workspace: exact partials) and as many of the other columns, by the SwiGLU rule."""
    M, K = 256, 1024
    Hn = 64 * (_cus() + 4)
    nb = hip.llj_gemm_swiglu_ws_bytes(ZINT4, M, Hn, K)
    assert nb > 0, "this shape is expected to split its tail"
    tail = nb // (16 * M * 64) * 64
    assert 0 < tail < Hn // 2
    rest = np.sort(np.random.default_rng(31).choice(Hn - tail, tail, replace=False))
    cols = np.concatenate([rest, np.arange(Hn - tail, Hn)])
    a, y1, y2 = swiglu_dual_case(M, Hn, K, cols)
    e = swiglu_e(0)
    _, W1, s1 = dev_weight(hip, ZINT4, Hn, K, 1, *e)
    _, W2, s2 = dev_weight(hip, ZINT4, Hn, K, 2, *e)
    ad, h = a_operand(a, K), sentinel(M + 1, Hn)
    ws = torch.full((nb // 4,), float("nan"), dtype=torch.float32, device=dev)
    call(hip, "llj_gemm_swiglu_ws", ZINT4, ad.data_ptr(), K, W1.data_ptr(), s1.data_ptr(), W2.data_ptr(), s2.data_ptr(),
         h.data_ptr(), Hn, M, Hn, K, ws.data_ptr(), nb, st())
    torch.cuda.synchronize()
    assert (words(h)[M] == SENT).all(), "wrote past row M"
    sub = sentinel(M, 2 * tail)
    sub[:, :] = h[:M, T(cols)]
    check_swiglu(sub[:, :tail], y1[:, :tail], y2[:, :tail], "gemm swiglu_ws whole-wave columns")
    check_swiglu(sub[:, tail:], y1[:, tail:], y2[:, tail:], "gemm swiglu_ws tail columns")
    for k in [k for k in _dev_weights if k[1] == Hn]:
        del _dev_weights[k]
    np_weight.cache_clear()  # (the two H x 1024 float64 weights)


_GQ = [(f"wfmt{w:#x}", w, {}) for w in GEMM_FMTS] + \
      [(f"wfmt{w:#x}-{name}", w, o) for w in (0, 1) for name, o in GLDS_TILES.items() if name != "256x256"] + \
      [("zint-w4z0", ZINT4, {_hip.OPT_GEMM_W4Z: 0})]


@pytest.mark.parametrize("B,T_,S,p0", [(2, 150, 256, 200), (1, 257, 512, 0), (1, 17, 32, 20)])
@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("wfmt,opts", [v[1:] for v in _GQ], ids=[v[0] for v in _GQ])
def test_gemm_qkv_rope_exact(hip, wfmt, opts, C, B, T_, S, p0):
    """llj_gemm_qkv_rope (the LDS-staged epilogue of the 256 x 128 LDS-DMA kernel included) on exact operands
    and a dyadic RoPE table: whole q buffer and whole caches (ring slots past S wrap; the rest keeps the
    sentinel). Rotating the unrounded y differs in >= 10 % of the q / k elements."""
    nh = 2
    hs, M = C // nh, B * T_
    rng = np.random.default_rng([37, wfmt & 0xFFFF, C, T_])
    a = rng.choice(np.array([-4, -3, 3, 4], f32), size=(M, C))
    w, Wd, szd = dev_weight(hip, wfmt, 3 * C, C)
    H.assert_exact_condition(a, w)
    y = H.exact_linear(a, w)
    pos = np.arange(p0, p0 + T_, dtype=np.int32)
    rope = H.dyadic_rope(rng, p0 + T_, hs)
    qe, kce, vce, wrong = qkv_expect(y, B, T_, nh, hs, S, pos, rope)
    print("wrong-rounding difference share:", round(wrong, 3))
    assert wrong >= 0.10, wrong
    ad, rd, pd = put(sentinel(M, C), a), T(rope), T(pos)
    q, kc, vc = sentinel(M + 1, C), sentinel(B * nh * S, hs), sentinel(B * nh * S, hs)
    with options(hip, opts):
        call(hip, "llj_gemm_qkv_rope", wfmt, ad.data_ptr(), Wd.data_ptr(), P(szd), q.data_ptr(), kc.data_ptr(),
             vc.data_ptr(), rd.data_ptr(), pd.data_ptr(), B, T_, C, nh, S, st())
    torch.cuda.synchronize()
    what = f"gemm qkv wfmt {wfmt:#x} C {C} B {B} T {T_} {opts}"
    check(q, qe, what + " q")
    check_cache(kc, kce, what + " k cache")
    check_cache(vc, vce, what + " v cache")


# ================================================================== Part D: attention
SPEC = {"half": (0, 0), "full": (1, 0), "batch": (0, 1)}  # LLJ_OPT_ATT_SPEC_FULL, LLJ_OPT_ATT_SPEC_BATCH


def spec_options(hip, spec):
    return options(hip, {_hip.OPT_ATT_SPEC_FULL: SPEC[spec][0], _hip.OPT_ATT_SPEC_BATCH: SPEC[spec][1]})


def probe_values(B, nh, S, hs, off):
    """V[b, h, s, d] = 1 iff s == off + h hs + d (else 0): with q = 0, output column h hs + d of a row is
    1 / nvis if the row sees slot off + h hs + d and exactly 0 if not."""
    V = torch.zeros(B, nh, S, hs, dtype=torch.bfloat16, device=dev)
    c = torch.arange(nh * hs, device=dev)
    c = c[off + c < S]
    V[:, c // hs, off + c, c % hs] = 1.0
    return V


def check_visible(y, off, nvis, what):
    """y (rows, C) float32 from a probe_values run: column c is nonzero exactly when slot off + c is among
    the row's nvis visible slots 0 .. nvis - 1, and then within 2^-8 relative of 1 / nvis."""
    nvis = np.asarray(nvis, np.float64).reshape(-1, 1)
    vis = (off + np.arange(y.shape[1]))[None, :] < nvis
    assert not np.isnan(y).any(), f"{what}: output not written"
    nz = y != 0
    assert np.array_equal(nz, vis), (f"{what}: visible set wrong for {(nz != vis).any(1).sum()} rows; first at "
                                     f"(row, column) {tuple(np.argwhere(nz != vis)[0])}, off {off}")
    err = np.abs(y * nvis - 1.0)
    assert (err[vis] <= 2.0 ** -8).all(), f"{what}: weights differ from 1 / nvis by up to {err[vis].max():.3g} relative"


def rand_keys(rng, B, nh, S, hs):
    k = T(bf16(rng.standard_normal((1, nh, S, hs)).astype(f32)), torch.bfloat16)
    return k.expand(B, nh, S, hs).contiguous()


DEC_P = {2048: [0, 1, 31, 32, 63, 64, 127, 128, 129, 2000, 2047, 2048 + 5], 144: [80, 143, 300]}


def decode_visible(hip, hs, nh, B, S, launch, what):
    """The visible-set probe over every slot of the cache (one offset per C slots) and every position of
    DEC_P[S]; launch(q, k, v, pos, rows) -> float32 y (rows, C)."""
    C = nh * hs
    q = torch.zeros(B, C, dtype=torch.bfloat16, device=dev)
    kd = rand_keys(np.random.default_rng([41, hs, S]), B, nh, S, hs)
    for off in range(0, S, C):
        vd = probe_values(B, nh, S, hs, off)
        for p in DEC_P[S]:
            y = launch(q, kd, vd, T(np.array([p], np.int32)), B)
            check_visible(y, off, [min(p + 1, S)] * B, f"{what} S {S} p {p}")


def read_rows(ybuf, rows):
    """A sentinel output buffer (rows + 1, C) as float32; the row past the end must keep the sentinel."""
    torch.cuda.synchronize()
    b = words(ybuf)
    assert (b[rows:] == SENT).all(), "wrote past the last row"
    return H.f32_of_bits(b[:rows])


@pytest.mark.parametrize("spec", list(SPEC))
@pytest.mark.parametrize("B", [1, 17])
@pytest.mark.parametrize("hs,nh,S", [(64, 8, 2048), (128, 4, 2048), (64, 2, 144), (128, 2, 144)])
def test_attention_visible_set(hip, hs, nh, S, B, spec):
    """llj_attention sees slots <= p, or all S once p >= S: probed slot by slot at the positions either side
    of the 32 / 64 / 128 key-pass boundaries, at p = 2000, at the last slot and past the ring wrap; grids of
    at most 64 blocks (speculative key pass) and above (B = 17)."""
    def launch(q, k, v, pos, rows):
        y = sentinel(rows + 1, nh * hs)
        call(hip, "llj_attention", q.data_ptr(), k.data_ptr(), v.data_ptr(), y.data_ptr(), pos.data_ptr(), rows, 1, nh,
             hs, S, st())
        return read_rows(y, rows)

    with spec_options(hip, spec):
        decode_visible(hip, hs, nh, B, S, launch, f"attention {spec} hs {hs} B {B}")


@pytest.mark.parametrize("nsplit", [2, 16])
@pytest.mark.parametrize("hs,nh,S", [(64, 8, 2048), (128, 4, 2048), (64, 2, 144), (128, 2, 144)])
def test_attention_split_visible_set(hip, hs, nh, S, nsplit):
    B = 2
    ws = torch.empty(hip.llj_attention_ws_bytes(B, nh, hs, nsplit), dtype=torch.uint8, device=dev)

    def launch(q, k, v, pos, rows):
        y = sentinel(rows + 1, nh * hs)
        call(hip, "llj_attention_split", q.data_ptr(), k.data_ptr(), v.data_ptr(), y.data_ptr(), pos.data_ptr(), rows, 1,
             nh, hs, S, nsplit, ws.data_ptr(), st())
        return read_rows(y, rows)

    decode_visible(hip, hs, nh, B, S, launch, f"split attention nsplit {nsplit} hs {hs}")


def merge_parts(part, hs):
    """float64 merge of llj_attention_part's records (rows, nh, nsplit, hs + 4): hs unnormalized outputs,
    the running maximum (log2 domain), the sum, 2 pad -> y (rows, nh * hs)."""
    o, mx, l = part[..., :hs].astype(np.float64), part[..., hs].astype(np.float64), part[..., hs + 1].astype(np.float64)
    top = mx.max(-1, keepdims=True)
    assert np.isfinite(top).all(), "a (row, head) without any visible key"
    f = np.where(np.isneginf(mx), 0.0, np.exp2(np.where(np.isneginf(mx), 0.0, mx) - top))
    y = (o * f[..., None]).sum(-2) / (l * f).sum(-1, keepdims=True)
    return y.reshape(y.shape[0], -1)


@pytest.mark.parametrize("nsplit", [2, 3, 4])
@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("S,plist", [(144, [80, 143, 300]), (256, [5, 90, 255, 300])])
def test_attention_part_visible_set(hip, hs, S, plist, nsplit):
    """llj_attention_part's interleaved key splits, merged here in float64 from the partial records (with
    q = 0 every maximum is 0 or -inf): together the splits see each visible slot exactly once."""
    nh, B = 2, 2
    C = nh * hs
    q = torch.zeros(B, C, dtype=torch.bfloat16, device=dev)
    kd = rand_keys(np.random.default_rng([43, hs, S]), B, nh, S, hs)
    for off in range(0, S, C):
        vd = probe_values(B, nh, S, hs, off)
        for p in plist:
            ws = torch.full((B, nh, nsplit, hs + 4), float("nan"), dtype=torch.float32, device=dev)
            assert ws.numel() * 4 == hip.llj_attention_ws_bytes(B, nh, hs, nsplit)
            call(hip, "llj_attention_part", q.data_ptr(), kd.data_ptr(), vd.data_ptr(), T(np.array([p], np.int32)).data_ptr(),
                 B, 1, nh, hs, S, nsplit, ws.data_ptr(), st())
            torch.cuda.synchronize()
            part = ws.cpu().numpy()
            assert not np.isnan(part[..., :hs + 2]).any(), "partial records not written"
            mx = part[..., hs]
            assert ((mx == 0) | np.isneginf(mx)).all()
            check_visible(merge_parts(part, hs).astype(f32), off, [min(p + 1, S)] * B,
                          f"attention_part nsplit {nsplit} hs {hs} S {S} p {p}")


FLASH = [(130, 17, 160), (64, 0, 64), (257, 0, 512)]  # (T, p0, S)


@pytest.mark.parametrize("pair", [0, 1])
@pytest.mark.parametrize("qb", [1, 2])
@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("T_,p0,S", FLASH)
def test_attention_prefill_visible_set(hip, T_, p0, S, hs, qb, pair):
    """llj_attention_prefill: query t sees slots 0 .. p0 + t; every row's diagonal boundary is checked."""
    nh, B = 2, 2
    C = nh * hs
    q = torch.zeros(B * T_, C, dtype=torch.bfloat16, device=dev)
    kd = rand_keys(np.random.default_rng([47, hs, S]), B, nh, S, hs)
    pd = T(np.arange(p0, p0 + T_, dtype=np.int32))
    nvis = np.tile(p0 + np.arange(T_) + 1, B)
    with options(hip, {_hip.OPT_FLASH_QB: qb, _hip.OPT_FLASH_PAIR: pair}):
        for off in range(0, S, C):
            vd = probe_values(B, nh, S, hs, off)
            y = sentinel(B * T_ + 1, C)
            call(hip, "llj_attention_prefill", q.data_ptr(), kd.data_ptr(), vd.data_ptr(), y.data_ptr(), pd.data_ptr(), B,
                 T_, nh, hs, S, st())
            check_visible(read_rows(y, B * T_), off, nvis, f"flash prefill T {T_} p0 {p0} S {S} hs {hs} qb {qb} pair {pair}")


PASS_EDGES = [31, 32, 33, 63, 64, 65, 127, 128, 129]
MIN_GAP = 110.0


def selected_key_case(hs, nh, S, B, T_, pos, seed):
    """K[s] = 8 code[s] (+-1 codes per head), q[m, h] = 8 code[target(m, h)], V random: the target's score
    exceeds every other slot's by >= MIN_GAP (natural units, asserted), so every other weight is exactly 0 in
    fp32 and y[m, h, :] = V[b, h, target] bitwise. Targets per (row, head) cycle through 0, p, p - 1 and the
    slots either side of the 32 / 64 / 128 key-pass boundaries, all visible."""
    rng = np.random.default_rng([53, hs, S, seed])
    code = rng.choice(np.array([-1.0, 1.0], f32), size=(nh, S, hs))
    V = bf16(rng.standard_normal((B, nh, S, hs)).astype(f32))
    rows = B * T_
    target = np.zeros((rows, nh), np.int64)
    for m in range(rows):
        p = int(pos[m % T_])
        last = p if p < S else S - 1  # the newest slot in slot order (p >= S: every slot is visible)
        cand = [0, last, max(last - 1, 0)] + PASS_EDGES
        for h in range(nh):
            c = cand[(m + 5 * h) % len(cand)]
            target[m, h] = c if c <= last else last
    q = np.stack([np.concatenate([8 * code[h, target[m, h]] for h in range(nh)]) for m in range(rows)])
    gap = np.inf
    want = np.zeros((rows, nh * hs), f32)
    for m in range(rows):
        for h in range(nh):
            s = (8.0 * code[h].astype(np.float64)) @ q[m, h * hs:(h + 1) * hs].astype(np.float64)
            t = target[m, h]
            assert s[t] == 64 * hs
            gap = min(gap, (s[t] - np.delete(s, t).max()) / np.sqrt(hs))
            want[m, h * hs:(h + 1) * hs] = V[m // T_, h, t]
    assert gap >= MIN_GAP, gap
    K = np.broadcast_to(8 * code[None], (B, nh, S, hs))
    return q.astype(f32), K, V, want, gap, target


def run_selected(hip, entry, hs, nh, S, B, T_, pos, seed, extra=()):
    q, K, V, want, gap, target = selected_key_case(hs, nh, S, B, T_, pos, seed)
    qd, kd, vd, pd = T(q, torch.bfloat16), T(K, torch.bfloat16), T(V, torch.bfloat16), T(np.asarray(pos, np.int32))
    y = sentinel(B * T_ + 1, nh * hs)
    call(hip, entry, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), y.data_ptr(), pd.data_ptr(), B, T_, nh, hs, S, *extra,
         st())
    torch.cuda.synchronize()
    print(f"{entry} hs {hs} S {S}: selected-key gap {gap:.0f}")
    check(y, want, f"{entry} selected key hs {hs} nh {nh} S {S} pos {list(pos)[:3]}")


@pytest.mark.parametrize("spec", list(SPEC))
@pytest.mark.parametrize("hs,nh", [(64, 2), (128, 2), (128, 8)])
@pytest.mark.parametrize("S,p", [(2048, 2047), (2048, 130), (2048, 2048 + 5), (256, 255), (144, 300)])
def test_attention_selected_key(hip, hs, nh, S, p, spec):
    """llj_attention returns V[target] bitwise when one key carries all the weight (12 rows with different
    targets per head; 24 and 96 blocks)."""
    with spec_options(hip, spec):
        run_selected(hip, "llj_attention", hs, nh, S, 12, 1, [p], p)


@pytest.mark.parametrize("nsplit", [2, 16])
@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("S,p", [(2048, 2047), (2048, 130), (2048, 2048 + 5), (144, 143)])
def test_attention_split_selected_key(hip, hs, S, p, nsplit):
    nh, B = 2, 12
    ws = torch.empty(hip.llj_attention_ws_bytes(B, nh, hs, nsplit), dtype=torch.uint8, device=dev)
    run_selected(hip, "llj_attention_split", hs, nh, S, B, 1, [p], p, extra=(nsplit, ws.data_ptr()))


@pytest.mark.parametrize("pair", [0, 1])
@pytest.mark.parametrize("qb", [1, 2])
@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("T_,p0,S", FLASH)
def test_attention_prefill_selected_key(hip, T_, p0, S, hs, qb, pair):
    with options(hip, {_hip.OPT_FLASH_QB: qb, _hip.OPT_FLASH_PAIR: pair}):
        run_selected(hip, "llj_attention_prefill", hs, 2, S, 2, T_, np.arange(p0, p0 + T_), T_)


# ================================================================== Part C: LLM.int8 (wfmt 2)
# The epilogue multiplies by 1.f / (127 * 127) and rounds twice to fp16, but for this construction (SCA = 127 *
# 2^-5, SCB = 127 * 2^-e) the fp32 constant SCA SCB / 127^2 is exactly 2^-(5 + e) however it is associated, so
# acc * const is exact while |acc| < 2^24 and both fp16 roundings and the bf16 one have a single correct bit
# pattern (helpers.i8_reference, which asserts the conditions): the check is bitwise. The side-product regimes,
# epilogues and side buffers these shapes do not reach are in tests/test_int8_exact_gpu.py.
I8_THR = 6.0


def i8_case(M, N, K, outliers, seed=0):
    """helpers.i8_exact_case with every row of SCA class 5 (SCA = 127 / 32) and `outliers` random outlier columns;
    `aq` the int8 codes the workspace must hold, `y16` the one correct result."""
    rng = np.random.default_rng([59, M, N, K, outliers, seed])
    ocols = rng.choice(K, outliers, replace=False)
    c = H.i8_exact_case(M, N, K, ocols, (5,) * M, seed, rowmax_in_outlier=M > 1 and outliers > 0, mutants=False)
    return dict(c, aq=c["codes"])


def i8_weights(hip, c):
    N, K = c["cb"].shape
    cb = T(c["cb"])
    cbt = torch.empty_like(cb)
    call(hip, "llj_i8_repack", cb.data_ptr(), cbt.data_ptr(), N, K, st())
    torch.cuda.synchronize()
    return cbt, T(c["scb"])


def check_i8(out, c, what):
    """Bitwise: bf16(f16(f16(main) + side)) in the top-left corner, the sentinel everywhere else."""
    check(out, bf16(c["y16"]), what)


def check_aq(ws, c, what):
    """The workspace's quantized rows (first in the workspace after the 16-byte header) are the reference's codes:
    rint-to-even of 32 a (half of them ties), the outlier columns 0."""
    M, K = c["aq"].shape
    got = ws[16:16 + M * K].cpu().numpy().view(np.int8).reshape(M, K)
    assert np.array_equal(got, c["aq"]), f"{what}: {(got != c['aq']).sum()} int8 codes differ from the reference's"


@pytest.mark.parametrize("outliers", [0, 3])
@pytest.mark.parametrize("M", [1, 2, 8])
def test_int8_linear_exact_quantization(hip, M, outliers):
    """llj_i8_stats + llj_linear (one row: the LDS image; 2 and 8 rows: the workspace's rows streamed) and
    llj_i8_norm_rowstats + llj_linear with LLJ_WF_I8_ROWSTATS (rows quantized per chunk in the GEMV)."""
    for N, K in [(16, 128), (48, 640)]:
        c = i8_case(M, N, K, outliers)
        cbt, scb = i8_weights(hip, c)
        ad = a_operand(c["a"], K + 8)
        ws = torch.zeros(hip.llj_i8_ws_bytes(M, K), dtype=torch.uint8, device=dev)
        call(hip, "llj_i8_stats", ad.data_ptr(), K + 8, M, K, I8_THR, ws.data_ptr(), st())
        out = sentinel(9, N + 6)
        call(hip, "llj_linear", 2, ad.data_ptr(), K + 8, cbt.data_ptr(), scb.data_ptr(), None, out.data_ptr(), N + 6, M, N,
             K, ws.data_ptr(), 0, None, st())
        torch.cuda.synchronize()
        what = f"int8 linear M {M} N {N} K {K} outliers {outliers}"
        check_aq(ws, c, what)
        check_i8(out, c, what)
        ws2 = torch.zeros_like(ws)
        stb = torch.full((hip.llj_i8_rowstats_bytes(K) // 4,), 3, dtype=torch.int32, device=dev)  # rewritten whole
        ac = put(sentinel(M, K), c["a"])  # (llj_i8_norm_rowstats takes contiguous rows)
        call(hip, "llj_i8_norm_rowstats", ac.data_ptr(), None, 1e-5, None, M, K, I8_THR, ws2.data_ptr(), stb.data_ptr(),
             st())
        out2 = sentinel(9, N + 6)
        call(hip, "llj_linear", 2 | _hip.WF_I8_ROWSTATS, ac.data_ptr(), K, cbt.data_ptr(), scb.data_ptr(), None,
             out2.data_ptr(), N + 6, M, N, K, stb.data_ptr(), 0, None, st())
        torch.cuda.synchronize()
        check_i8(out2, c, what + " (row statistics hand-off)")


@pytest.mark.parametrize("outliers", [0, 3])
@pytest.mark.parametrize("M", [40, 300])
def test_gemm_int8_exact_quantization(hip, M, outliers):
    """llj_gemm_i8_linear (128- and 256-row kernels) on the same construction."""
    N = 128
    for K in (128, 640):
        c = i8_case(M, N, K, outliers)
        cbt, scb = i8_weights(hip, c)
        ad = a_operand(c["a"], K + 8)
        ws = torch.zeros(hip.llj_i8_ws_bytes(M, K), dtype=torch.uint8, device=dev)
        call(hip, "llj_i8_stats", ad.data_ptr(), K + 8, M, K, I8_THR, ws.data_ptr(), st())
        out = sentinel(M + 2, N + 8)
        call(hip, "llj_gemm_i8_linear", ad.data_ptr(), K + 8, cbt.data_ptr(), scb.data_ptr(), ws.data_ptr(), None, None, 0,
             out.data_ptr(), N + 8, M, N, K, st())
        torch.cuda.synchronize()
        what = f"int8 gemm M {M} K {K} outliers {outliers}"
        check_aq(ws, c, what)
        check_i8(out, c, what)
