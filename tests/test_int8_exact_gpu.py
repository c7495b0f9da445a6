"""Bitwise tests of the LLM.int8 kernels (wfmt 2) and of their outlier side products (GPU only): the int8
GEMV family (csrc/gemv_impl.h), the prefill GEMMs (csrc/gemm.hip), the statistics, gathers and the one-launch
prep (csrc/int8.hip) and the any-shape kernel (csrc/generic.hip llj_g_i8_linear).

Technique (tests/helpers.py "exact LLM.int8 operands"): row m has SCA = 127 * 2^-j (j in 5, 6, 14) and column n
SCB = 127 * 2^-e, so the fp32 dequantization constant SCA SCB / 127^2 is exactly 2^-(j + e) in every association,
127 / SCA = 2^j and SCB / 127 = 2^-e. Activations are n 2^-(j + 1), |n| <= 254 (half the codes are ties: round to
nearest even is pinned), outlier columns hold +-6 (the threshold itself), +-8 or +-12 in the rows that set them
and sub-threshold multiples of 1 / 4 elsewhere; one case per regime puts a row's maximum inside an outlier
column another row sets. Then acc * const is exact in fp32, the fp16 side product is an exact dyadic sum in any
order, main16 + side is exact in fp32, and the result has one bit pattern:
    y16 = f16(f16(acc 2^-(j + e)) + sum_{k in O} a CB 2^-e),
computed in integers and float64 (helpers.i8_reference) and equal to oracle/llama_np.py int8_linear bit for bit
(tests/test_int8_exact_host.py). The conditions (|acc| < 2^24, sum |a| |CB| < 2^24 side units, the exact fp32
sum, |y| < 65504, the constants) are asserted on the CPU by the reference before any launch. Outputs are
compared as bf16 values; every buffer starts from helpers.SENTINEL, which rows >= M, padding columns and
untouched cache slots keep; activations sit at lda > K with 1000 in the padding.

Class 14 (SCA < 1 / 64) selects the GEMV's quant8f rule for the whole call; such rows hold 0 in the outlier
columns (their main term reaches down to 2^-23: no fp32 sum with a side term holds it exactly). SwiGLU cases use
e in 10 .. 13 so that silu is not the identity (as Part A's swiglu_e), and follow Part A's candidate rule.

Test power, from the references alone (helpers.I8Power; floors asserted per test on its pooled elements --
a GEMV test pools the side-product regimes of its (A path, rows): one row of N = 16 + 48 cannot hold 8 elements
at 3 %; a GEMM test is its own pool). Measured per pool of this file's tests: inner fp16 rounding dropped 3.0 -
5.0 % of the bf16 outputs (floor 1 % and 8 elements), outer dropped 3.8 - 6.2 % (same floor), inner dropped at
fp16 output (dt 1) 22.2 % (floor 10 %), last outlier column dropped 72 - 98 % (98 % at one row, which sets every
column itself; floor 50 %), ties rounded half away 60 - 79 % (floor 50 %).
Every case with outlier columns and more than one row has a row whose SCA is decided inside an outlier column
that another row sets (asserted by the builder and by each test: leaving flagged columns out of SCA fails it).
SwiGLU: 100 % of the elements take the nearer neighbour. The f16 MFMA of the gathered side GEMM accumulates
these dyadic sums without loss (every gathered case is bitwise).

289 cases, 4.2 s for the file on an MI355X (the slowest case 0.3 s, the first, which builds the references).

Mutations of the kernels that this file catches (scratch builds, each run once on the GPU; numerical only): the
inner (_Float16) of the GEMV, GEMM and any-shape epilogues removed; >= thr made > thr in the one-launch prep and
in i8_stats_rows_kernel; the in-stream loop taking one of a chunk's two entries; i8_side_tile's fast path
accumulating len - 1 entries of a round; the general path's SB batch skipping its last column; quant8_fast's
magic constant replaced by roundf; AM_I8Q's two-columns-per-trip walk dropping the second; the gathers' zero pad
not written; the GEMM's dense side loop running SKC - 1 chunks.
"""
import functools

import numpy as np
import pytest
import torch

from lit_llama import _hip
from tests import helpers as H
from tests.helpers import bf16
from tests.test_kernels_gpu import T, _st_decode, call, st
from tests.test_streaming_exact_gpu import P, SENT, SwigluPool, a_operand, check, check_cache, put, sentinel, stream_a, words

pytestmark = pytest.mark.gpu
dev = "cuda"
f32, f64 = np.float32, np.float64
THR = H.I8_THR
ROWSTATS = 2 | _hip.WF_I8_ROWSTATS
FILL = 0xAB  # byte pattern of a workspace / gather buffer before the kernel under test writes it
NSB = 32


# ------------------------------------------------------------------ operands
_dev_w = {}


def dev_w(hip, c):
    """(CB in the I8P tiling, SCB) on the device for a case's weight."""
    key = id(c["cb"])
    if key not in _dev_w:
        N, K = c["cb"].shape
        cb = T(c["cb"])
        cbt = torch.empty_like(cb)
        call(hip, "llj_i8_repack", cb.data_ptr(), cbt.data_ptr(), N, K, st())
        torch.cuda.synchronize()
        _dev_w[key] = (c["cb"], cbt, T(c["scb"]))
    return _dev_w[key][1:]


def ws_offsets(M, K):
    """csrc/i8ws.h i8_offsets, restated."""
    al = lambda x: (x + 15) & ~15  # noqa: E731
    kb = ((K + NSB - 1) // NSB + 31) & ~31
    o = dict(kb=kb, aq=16)
    o["part"] = al(16 + M * K)
    o["cnt"] = o["part"] + 4 * NSB * M
    o["list"] = o["cnt"] + 4 * NSB
    o["sca"] = o["list"] + 4 * NSB * kb
    o["flag"] = al(o["sca"] + 4 * M)
    o["avh"] = al(o["flag"] + K)
    o["aval"] = o["avh"] + 16
    o["total"] = o["aval"] + 16 * NSB * kb
    return o


def stats_ws(hip, ad, lda, M, K):
    ws = torch.full((hip.llj_i8_ws_bytes(M, K),), FILL, dtype=torch.uint8, device=dev)
    call(hip, "llj_i8_stats", ad.data_ptr(), lda, M, K, THR, ws.data_ptr(), st())
    return ws


def ws_counts(ws, M, K):
    """(k-block width, avh[0], the per-k-block outlier counts) of a workspace."""
    o = ws_offsets(M, K)
    b = ws.cpu().numpy()
    return o["kb"], int(b[o["avh"]:o["avh"] + 4].view(np.int32)[0]), b[o["cnt"]:o["list"]].view(np.int32)


def add32(x, y):
    """The kernels' one fp32 addition of two fp32 values: the exact sum (float64 holds it: both are dyadic numbers
    within 2^-24 .. 2^11) rounded once. A class-14 row's result is too small for the sum to be exact in fp32, but
    a single addition has no order to depend on."""
    return (np.asarray(x, f64) + np.asarray(y, f64)).astype(f32)


def want_linear(c, bias=None):
    """bf16(y16 + bias)."""
    return bf16(c["y16"] if bias is None else add32(c["y16"], bias[None, :]))


def want_resid(c, x0):
    """bf16(x0 + bf16(y16))."""
    return bf16(add32(x0, bf16(c["y16"])))


def sca_inside(c):
    """The case has a row whose SCA is decided by an element inside an outlier column that another row sets (the
    builder asserts the property where it sets `rowmax_row`). One row alone cannot have it, nor a case without
    outlier columns."""
    return c["M"] == 1 or not c["cols"].size or c["rowmax_row"] is not None


def dyadic(rng, shape, denom=4, lim=8):
    return (rng.integers(-lim * denom, lim * denom + 1, size=shape) / denom).astype(f32)


def qkv_want(y16, B, T_, nh, hs, S, pos, rope):
    """Expected q (B T, C) and caches (B, nh, S, hs; NaN where the sentinel must stay) from y16 (B T, 3 C): RoPE of
    v = bf16(y16) on a dyadic table. v cos and partner sin are exact in fp32 (8 + 4 bits), so the kernel's one
    fp32 rounding of their sum or difference -- contracted into an fma or not -- is the rounding of the exact
    value, which float64 holds: one bit pattern, though the sum itself need not be exact in fp32 here (columns of
    different scales sit next to each other)."""
    C, Mr = nh * hs, B * T_
    v = bf16(y16)
    cs = rope[np.asarray(pos)][None, :, None]
    q, k, vv = [v[:, i * C:(i + 1) * C].reshape(B, T_, nh, hs) for i in range(3)]
    qe, ke = H.rope_bf16(q, cs, exact=False), H.rope_bf16(k, cs, exact=False)
    kc = np.full((B, nh, S, hs), np.nan, f32)
    vc = np.full((B, nh, S, hs), np.nan, f32)
    for t in range(T_):
        kc[:, :, pos[t] % S] = ke[:, t]
        vc[:, :, pos[t] % S] = vv[:, t]
    return qe.reshape(Mr, C), kc, vc


# ================================================================== the GEMV family
# (A path, rows, llj_set_stream_a): lds the LDS image of one row; i8s the workspace's rows streamed (AM_I8S); img
# the image rows; i8q / i8qf the rows quantized per chunk from llj_i8_norm_rowstats's hand-off block (AM_I8Q; with
# a class-14 row quant8f, i8qf: classes 5 and 6 only, quant8_fast); slice: a 12-row workspace (the two-pass prep,
# avh = 0) served as slices of 8 and 4 rows with i8_row0 = 8
GEMV_PATHS = [("lds", 1, 1), ("i8s", 2, 1), ("i8s", 8, 1), ("img", 2, 0), ("img", 8, 0), ("i8q", 1, 1), ("i8q", 5, 1),
              ("i8q", 8, 1), ("i8qf", 8, 1), ("slice", 12, 1), ("slice", 12, 0)]
LAYOUTS = [k for k, v in H.I8_GEMV_LAYOUTS.items() if v[0] < 8192]
MAXCNT = {"instream": 2, "instream_over": 3, "spc8": 8, "spc9": 9, "spc32w8": 32, "spc33w8": 33}  # per k-block


class Operands:
    """The device operands of one case on one A path: rows at lda = K + 8 (`ad`) and contiguous (`ac`), and per
    slice (first row, rows, wfmt, statistics pointer, i8_row0)."""

    def __init__(self, hip, path, c, layout=None):
        M, K = c["M"], c["K"]
        self.ad, self.ac = a_operand(c["a"], K + 8), put(sentinel(M, K), c["a"])
        self.lda = K + 8
        if path in ("i8q", "i8qf"):
            self.ws = torch.zeros(hip.llj_i8_ws_bytes(M, K), dtype=torch.uint8, device=dev)
            self.stb = torch.full((hip.llj_i8_rowstats_bytes(K) // 4,), 3, dtype=torch.int32, device=dev)  # rewritten whole
            call(hip, "llj_i8_norm_rowstats", self.ac.data_ptr(), None, 1e-5, None, M, K, THR, self.ws.data_ptr(),
                 self.stb.data_ptr(), st())
            self.ad, self.lda = self.ac, K  # (the hand-off block belongs to contiguous rows)
            self.slices = [(0, M, ROWSTATS, self.stb.data_ptr(), 0)]
        else:
            self.ws = stats_ws(hip, self.ad, K + 8, M, K)
            kb, avh, cnt = ws_counts(self.ws, M, K)
            assert avh == (1 if M <= 8 else 0), "one-launch prep for M <= 8, two passes beyond"
            if layout in MAXCNT:  # the workspace is in the regime the layout is named for
                assert cnt.max() == MAXCNT[layout] and kb == {128: 32, 640: 32, 3200: 128, 8192: 256}[K]
            self.slices = [(r0, min(8, M - r0), 2, self.ws.data_ptr(), r0) for r0 in range(0, M, 8)]

    def a(self, r0):
        return self.ad[r0].data_ptr()

    def x(self, r0):
        return self.ac[r0].data_ptr()


def gemv_case(path, layout, M, N, **kw):
    if path == "i8qf":
        kw["with14"] = False
    return H.i8_gemv_case(layout, M, N, **kw)


@functools.lru_cache(maxsize=None)
def gemv_power(path, M, layouts=tuple(LAYOUTS)):
    """The floors of helpers.I8Power on the references of one (A path, rows), pooled over the side-product regimes
    and N = 16, 48: one row of N = 16 + 48 alone cannot hold 8 elements at 3 %."""
    pool = H.I8Power()
    for layout in layouts:
        for N in (16,) if H.I8_GEMV_LAYOUTS[layout][0] >= 8192 else (16, 48):
            pool.add(gemv_case(path, layout, M, N))
    return pool.finish(f"{path} M {M}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("path,M,stream", GEMV_PATHS)
def test_gemv_linear_resid_exact(hip, path, M, stream, layout):
    """llj_linear (with and without bias), llj_linear_resid, llj_norm_linear (norm_w NULL) and, from a hand-off
    block, llj_i8_linear_resid on every A path and every side-product regime, N = 16 and 48 (ldc > N)."""
    gemv_power(path, M)
    with stream_a(hip, stream):
        for N in (16, 48):
            c = gemv_case(path, layout, M, N)
            assert sca_inside(c)
            K = c["K"]
            cbt, scb = dev_w(hip, c)
            op = Operands(hip, path, c, layout)
            rng = np.random.default_rng([3, M, N, K])
            bias, x0 = dyadic(rng, N), dyadic(rng, (M, N), 8, 16)
            bd = T(bias, torch.bfloat16)
            ldc = N + 6
            o1, o2, o3 = sentinel(M + 1, ldc), sentinel(M + 1, ldc), sentinel(M + 1, ldc)
            xr, xq = put(sentinel(M + 1, ldc), x0), put(sentinel(M + 1, ldc), x0)
            for r0, r, wf, stp, row0 in op.slices:
                call(hip, "llj_linear", wf, op.a(r0), op.lda, cbt.data_ptr(), scb.data_ptr(), None, o1[r0].data_ptr(), ldc,
                     r, N, K, stp, row0, None, st())
                call(hip, "llj_linear", wf, op.a(r0), op.lda, cbt.data_ptr(), scb.data_ptr(), bd.data_ptr(),
                     o2[r0].data_ptr(), ldc, r, N, K, stp, row0, None, st())
                call(hip, "llj_linear_resid", wf, op.a(r0), op.lda, cbt.data_ptr(), scb.data_ptr(), xr[r0].data_ptr(), ldc,
                     r, N, K, stp, row0, None, st())
                call(hip, "llj_norm_linear", wf, op.x(r0), None, 1e-5, cbt.data_ptr(), scb.data_ptr(), o3[r0].data_ptr(),
                     ldc, r, N, K, stp, row0, None, None, 0, st())
                if wf == ROWSTATS:
                    call(hip, "llj_i8_linear_resid", op.a(r0), op.lda, cbt.data_ptr(), scb.data_ptr(), xq.data_ptr(), ldc,
                         r, N, K, stp, st())
            torch.cuda.synchronize()
            what = f"{path} M {M} stream_a {stream} {layout} N {N}"
            check(o1, want_linear(c), what + " llj_linear")
            check(o2, want_linear(c, bias), what + " llj_linear + bias")
            check(xr, want_resid(c, x0), what + " llj_linear_resid")
            check(o3, want_linear(c), what + " llj_norm_linear")
            if path in ("i8q", "i8qf"):
                check(xq, want_resid(c, x0), what + " llj_i8_linear_resid")


@pytest.mark.parametrize("layout", ["spc32w8", "spc33w8"])
@pytest.mark.parametrize("path,M,stream", [("lds", 1, 1), ("i8s", 8, 1), ("i8q", 8, 1)])
def test_gemv_resid_eight_waves_exact(hip, path, M, stream, layout):
    """The 8-wave residual form (K = 8192 >= LLJ_NWR_KMIN), N = 16: 32 (the fast path's limit) and 33 (the
    general list walk) outlier columns in one k-block of 256, through llj_linear_resid and llj_i8_linear_resid."""
    N = 16
    gemv_power("w8", 12, ("spc32w8", "spc33w8"))  # (16 columns: pooled over both layouts on 12 rows of references)
    c = gemv_case(path, layout, M, N)
    assert sca_inside(c)
    K = c["K"]
    cbt, scb = dev_w(hip, c)
    rng = np.random.default_rng([4, M, N, K])
    x0 = dyadic(rng, (M, N), 8, 16)
    with stream_a(hip, stream):
        op = Operands(hip, path, c, layout)
        xr, xq = put(sentinel(M + 1, N + 6), x0), put(sentinel(M + 1, N + 6), x0)
        for r0, r, wf, stp, row0 in op.slices:
            call(hip, "llj_linear_resid", wf, op.a(r0), op.lda, cbt.data_ptr(), scb.data_ptr(), xr[r0].data_ptr(), N + 6, r,
                 N, K, stp, row0, None, st())
            if wf == ROWSTATS:
                call(hip, "llj_i8_linear_resid", op.a(r0), op.lda, cbt.data_ptr(), scb.data_ptr(), xq.data_ptr(), N + 6, r,
                     N, K, stp, st())
    torch.cuda.synchronize()
    check(xr, want_resid(c, x0), f"{path} M {M} {layout} llj_linear_resid")
    if path == "i8q":
        check(xq, want_resid(c, x0), f"{path} M {M} {layout} llj_i8_linear_resid")


@pytest.mark.parametrize("path,M,stream",
                         [("lds", 1, 1), ("i8s", 5, 1), ("img", 8, 0), ("i8q", 1, 1), ("i8q", 5, 1), ("i8q", 8, 1)])
def test_gemv_quant8f_rows_exact(hip, path, M, stream):
    """Every row of class 14 (SCA = 127 * 2^-14 < 1 / 64: AM_I8Q's quant8f, the prep's quant8 on the others)."""
    pool = H.I8Power()
    with stream_a(hip, stream):
        for N, K in [(16, 128), (48, 640)]:
            c = H.i8_quant8f_case(M, N, K)
            pool.add(c)
            cbt, scb = dev_w(hip, c)
            op = Operands(hip, path, c)
            out = sentinel(M + 1, N + 6)
            for r0, r, wf, stp, row0 in op.slices:
                call(hip, "llj_linear", wf, op.a(r0), op.lda, cbt.data_ptr(), scb.data_ptr(), None, out[r0].data_ptr(), N + 6,
                     r, N, K, stp, row0, None, st())
            torch.cuda.synchronize()
            check(out, want_linear(c), f"quant8f {path} M {M} N {N} K {K}")
    pool.finish(f"quant8f {path} M {M}", ("halfaway",))


@pytest.mark.parametrize("path,M,stream", [("lds", 1, 1), ("i8s", 3, 1), ("img", 3, 0), ("i8q", 1, 1), ("i8q", 3, 1)])
def test_gemv_zero_row_exact(hip, path, M, stream):
    """An all-zero row gives SCA 0, codes 0 and output 0 (no NaN from 127 / SCA), next to rows with outliers."""
    N, K = 16, 128
    c = H.i8_zero_row_case(M, N, K)
    cbt, scb = dev_w(hip, c)
    with stream_a(hip, stream):
        op = Operands(hip, path, c)
        out = sentinel(M + 1, N + 6)
        for r0, r, wf, stp, row0 in op.slices:
            call(hip, "llj_linear", wf, op.a(r0), op.lda, cbt.data_ptr(), scb.data_ptr(), None, out[r0].data_ptr(), N + 6, r,
                 N, K, stp, row0, None, st())
    torch.cuda.synchronize()
    check(out, want_linear(c), f"zero row {path} M {M}")


QKV_PATHS = [("lds", 1, 1, 1), ("i8s", 8, 1, 1), ("img", 8, 1, 0), ("i8q", 8, 1, 1), ("i8s", 2, 5, 1), ("img", 2, 5, 0)]


@pytest.mark.parametrize("layout", ["none", "walk128", "spc9"])
@pytest.mark.parametrize("path,B,T_,stream", QKV_PATHS)
def test_gemv_qkv_rope_exact(hip, path, B, T_, stream, layout):
    """llj_norm_qkv_rope (norm_w NULL), C = 128, two heads of 64, a dyadic RoPE table: the whole q buffer and both
    whole caches (untouched slots keep the sentinel); ring-wrapped positions (S = 8: 13 -> slot 5; 6 .. 10 ->
    6, 7, 0, 1, 2); B T = 10 rows in two calls on one 10-row workspace."""
    C, nh, S = 128, 2, 8
    hs, M = C // nh, B * T_
    c = gemv_case(path, layout, M, 3 * C)
    assert c["K"] == C and sca_inside(c)
    pos = np.arange(6, 11, dtype=np.int32) if T_ == 5 else np.array([13], np.int32)
    rope = H.dyadic_rope(np.random.default_rng([19, M]), 16, hs)
    qe, kce, vce = qkv_want(c["y16"], B, T_, nh, hs, S, pos, rope)
    cbt, scb = dev_w(hip, c)
    rd, pd = T(rope), T(pos)
    q, kc, vc = sentinel(M + 1, C), sentinel(B * nh * S, hs), sentinel(B * nh * S, hs)
    with stream_a(hip, stream):
        op = Operands(hip, path, c, layout)
        for r0, r, wf, stp, row0 in op.slices:
            call(hip, "llj_norm_qkv_rope", wf, op.ac.data_ptr(), None, 1e-5, cbt.data_ptr(), scb.data_ptr(), q.data_ptr(),
                 kc.data_ptr(), vc.data_ptr(), rd.data_ptr(), pd.data_ptr(), B, T_, C, nh, S, r0, r, stp, None, None, 0, st())
    torch.cuda.synchronize()
    what = f"qkv {path} B {B} T {T_} {layout}"
    check(q, qe, what + " q")
    check_cache(kc, kce, what + " k cache")
    check_cache(vc, vce, what + " v cache")


SWIGLU_PATHS = [("lds", 1, 1), ("i8s", 8, 1), ("img", 8, 0), ("i8q", 8, 1), ("i8q", 1, 1)]
SWIGLU_E = (10, 13)  # |y1| within a few units, where silu is not the identity


def swiglu_cases(path, layout, M, Hn):
    kw = dict(e_lo=SWIGLU_E[0], e_hi=SWIGLU_E[1])
    return gemv_case(path, layout, M, Hn, wseed=1, **kw), gemv_case(path, layout, M, Hn, wseed=2, **kw)


@pytest.mark.parametrize("path,M,stream", SWIGLU_PATHS)
def test_gemv_swiglu_exact(hip, path, M, stream):
    """llj_norm_swiglu (norm_w NULL; the DUAL side accumulators) by Part A's candidate rule, pooled over three
    side-product regimes and H = 16, 48."""
    pool = SwigluPool()
    with stream_a(hip, stream):
        for layout in ("none", "walk640", "instream"):
            for Hn in (16, 48):
                c1, c2 = swiglu_cases(path, layout, M, Hn)
                assert sca_inside(c1) and sca_inside(c2)
                K = c1["K"]
                (cb1, s1), (cb2, s2) = dev_w(hip, c1), dev_w(hip, c2)
                op = Operands(hip, path, c1, layout)
                h = sentinel(M + 1, Hn)
                for r0, r, wf, stp, row0 in op.slices:
                    call(hip, "llj_norm_swiglu", wf, op.x(r0), None, 1e-5, cb1.data_ptr(), s1.data_ptr(), cb2.data_ptr(),
                         s2.data_ptr(), h[r0].data_ptr(), r, Hn, K, stp, row0, None, None, 0, st())
                torch.cuda.synchronize()
                pool.add(h, c1["y16"].astype(f64), c2["y16"].astype(f64), f"swiglu {path} M {M} {layout} H {Hn}")
    pool.finish(f"swiglu {path} M {M}")


@pytest.mark.parametrize("path,M,stream", [("lds", 1, 1), ("i8s", 8, 1), ("img", 8, 0), ("i8q", 1, 1), ("i8q", 8, 1)])
def test_gemv_swiglu_stats_exact(hip, path, M, stream):
    """llj_i8_swiglu_stats with x's statistics in i8ws (lds / i8s / img) and in x_stats (i8q): h by the candidate
    rule, h_stats bitwise the numpy statistics of the h actually produced, the clr block zero afterwards."""
    pool = SwigluPool()
    with stream_a(hip, stream):
        for layout in ("none", "walk640", "instream"):
            for Hn in (16, 48):
                c1, c2 = swiglu_cases(path, layout, M, Hn)
                assert sca_inside(c1) and sca_inside(c2)
                K = c1["K"]
                (cb1, s1), (cb2, s2) = dev_w(hip, c1), dev_w(hip, c2)
                op = Operands(hip, path, c1, layout)
                h = sentinel(M + 1, Hn)
                hst = torch.zeros(hip.llj_i8_rowstats_bytes(Hn) // 4, dtype=torch.int32, device=dev)
                clr = torch.full((40,), 7, dtype=torch.int32, device=dev)
                i8q = path == "i8q"
                call(hip, "llj_i8_swiglu_stats", op.ac.data_ptr(), cb1.data_ptr(), s1.data_ptr(), cb2.data_ptr(), s2.data_ptr(),
                     h.data_ptr(), M, Hn, K, None if i8q else op.ws.data_ptr(), op.stb.data_ptr() if i8q else None,
                     hst.data_ptr(), clr.data_ptr(), 32, THR, st())
                torch.cuda.synchronize()
                what = f"swiglu_stats {path} M {M} {layout} H {Hn}"
                pool.add(h, c1["y16"].astype(f64), c2["y16"].astype(f64), what)
                cl = clr.cpu().numpy()
                assert not cl[:32].any() and (cl[32:] == 7).all(), f"{what}: clr block"
                hv = np.abs(H.f32_of_bits(words(h)[:M]).astype(np.float16).astype(f32))
                sca, flags = _st_decode(hst, M, Hn)
                np.testing.assert_array_equal(sca, np.where(hv >= THR, 0, hv).max(1), what)
                np.testing.assert_array_equal(flags, (hv >= THR).any(0), what)
                raw = hst.cpu().numpy().view(np.uint32)[16:16 + 512].reshape(64, 8)
                assert not raw[:, M:].any(), f"{what}: statistics of rows >= M"
    pool.finish(f"swiglu_stats {path} M {M}")


def test_gemv_int8_refuses_norm_weight(hip):
    """wfmt 2 with a norm weight (there is no norm-fused LLM.int8 form) returns LLJ_EINVAL and writes nothing."""
    M, C = 2, 128
    c = H.i8_gemv_case("none", M, 3 * C)
    cbt, scb = dev_w(hip, c)
    op = Operands(hip, "i8s", c)
    g = T(np.ones(C, f32), torch.bfloat16)
    out, q, kc, vc = sentinel(M + 1, 3 * C), sentinel(M + 1, C), sentinel(M * 2 * 8, 64), sentinel(M * 2 * 8, 64)
    rd, pd = T(H.dyadic_rope(np.random.default_rng(1), 16, 64)), T(np.array([3], np.int32))
    stp = op.ws.data_ptr()
    rc = [hip.llj_norm_linear(2, op.ac.data_ptr(), g.data_ptr(), 1e-5, cbt.data_ptr(), scb.data_ptr(), out.data_ptr(), 3 * C,
                              M, 3 * C, C, stp, 0, None, None, 0, st()),
          hip.llj_norm_qkv_rope(2, op.ac.data_ptr(), g.data_ptr(), 1e-5, cbt.data_ptr(), scb.data_ptr(), q.data_ptr(),
                                kc.data_ptr(), vc.data_ptr(), rd.data_ptr(), pd.data_ptr(), M, 1, C, 2, 8, 0, M, stp, None,
                                None, 0, st()),
          hip.llj_norm_swiglu(2, op.ac.data_ptr(), g.data_ptr(), 1e-5, cbt.data_ptr(), scb.data_ptr(), cbt.data_ptr(),
                              scb.data_ptr(), out.data_ptr(), M, 3 * C, C, stp, 0, None, None, 0, st())]
    assert rc == [1000, 1000, 1000], rc
    torch.cuda.synchronize()
    for b in (out, q, kc, vc):
        assert (words(b) == SENT).all()


# ================================================================== the prefill GEMMs
def fill16(*shape):
    """A buffer of 16-bit words (fp16 data) holding the FILL byte pattern."""
    return torch.full(shape, (FILL | (FILL << 8)) - 65536, dtype=torch.int16, device=dev)


def gathers(hip, op_ad, lda, c, ws, weights, kpad):
    """(ao16 buffer, [w16 buffers]) filled with the byte pattern and gathered, or (None, [None, ...]) for kpad None."""
    if kpad is None:
        return None, [None] * len(weights)
    M, K = c["M"], c["K"]
    ao = fill16(M, kpad)
    call(hip, "llj_i8_gather_act", op_ad.data_ptr(), lda, M, K, ws.data_ptr(), ao.data_ptr(), kpad, st())
    ws16 = []
    for cbt, scb, N in weights:
        w = fill16(N, kpad)
        call(hip, "llj_i8_gather_weight", cbt.data_ptr(), scb.data_ptr(), N, K, ws.data_ptr(), w.data_ptr(), kpad, st())
        ws16.append(w)
    return ao, ws16


def check_gather(ao, ws16, c, weights_np, kpad, what):
    """ao16[m, i] = f16 bits of a[m, list[i]], w16[n, i] = f16(f32(CB) * f32(SCB / 127)) for i < total; zero up to
    the next multiple of 64; the fill pattern everywhere else -- in every word when total > kpad."""
    cols = c["cols"]
    total = cols.size
    pat = np.uint16(FILL | (FILL << 8))
    nop = 0 if total > kpad else (total + 63) & ~63
    take = cols if total <= kpad else cols[:0]

    def expect(rows):
        e = np.full((rows.shape[0], kpad), pat, np.uint16)
        e[:, :nop] = 0
        e[:, :take.size] = rows
        return e

    got = ao.cpu().numpy().view(np.uint16)
    np.testing.assert_array_equal(got, expect(H.f16_bits(c["a"][:, take])), what + " ao16")
    for w, (cb, scb) in zip(ws16, weights_np):
        w16 = H.f16_bits(cb[:, take].astype(f32) * (scb.astype(f32) / f32(127.0))[:, None])
        np.testing.assert_array_equal(w.cpu().numpy().view(np.uint16), expect(w16), what + " w16")


@pytest.mark.parametrize("ncols,kpad", H.I8_GEMM_SIDES)
@pytest.mark.parametrize("K", [128, 640])
@pytest.mark.parametrize("M", [40, 300])
def test_gemm_int8_exact(hip, M, K, ncols, kpad):
    """llj_gemm_i8_linear, _resid and _silu_mul (the 128- and 256-row kernels, ragged last tiles), N = 128: the
    per-tile side product over 0, 3, 32, 33 (the kSideK = 32 boundary) and 70 columns -- one of them set by a
    single row --, the dense f16 GEMM over columns gathered with kpad = 128 (70: two 64-deep chunks and the zero
    pad) and kpad = 64 (exactly 64; 3), and 70 columns over a capacity of 64 (nothing gathered: both gather
    buffers keep their fill pattern in every word, the results are the per-tile ones)."""
    N = 128
    c = H.i8_gemm_case(M, N, K, ncols)
    c1 = H.i8_gemm_case(M, N, K, ncols, 1, *SWIGLU_E)
    c2 = H.i8_gemm_case(M, N, K, ncols, 2, *SWIGLU_E)
    assert np.array_equal(c["a"], c1["a"]) and np.array_equal(c["a"], c2["a"]) and sca_inside(c)
    pool = H.I8Power()
    pool.add(c)
    pool.finish(f"gemm M {M} K {K} columns {ncols}", ("inner", "outer", "dropcol", "halfaway") if ncols else ("halfaway",))
    ws_ = [dev_w(hip, x) for x in (c, c1, c2)]
    ad = a_operand(c["a"], K + 8)
    ws = stats_ws(hip, ad, K + 8, M, K)
    ao, (g0, g1, g2) = gathers(hip, ad, K + 8, c, ws, [(w[0], w[1], N) for w in ws_], kpad)
    kp = kpad or 0
    rng = np.random.default_rng([5, M, K, ncols])
    x0 = dyadic(rng, (M, N), 8, 16)
    out, xr, h = sentinel(M + 2, N + 8), put(sentinel(M + 2, N + 8), x0), sentinel(M + 2, N + 8)
    call(hip, "llj_gemm_i8_linear", ad.data_ptr(), K + 8, ws_[0][0].data_ptr(), ws_[0][1].data_ptr(), ws.data_ptr(), P(ao),
         P(g0), kp, out.data_ptr(), N + 8, M, N, K, st())
    call(hip, "llj_gemm_i8_resid", ad.data_ptr(), K + 8, ws_[0][0].data_ptr(), ws_[0][1].data_ptr(), ws.data_ptr(), P(ao),
         P(g0), kp, xr.data_ptr(), N + 8, M, N, K, st())
    call(hip, "llj_gemm_i8_linear", ad.data_ptr(), K + 8, ws_[1][0].data_ptr(), ws_[1][1].data_ptr(), ws.data_ptr(), P(ao),
         P(g1), kp, h.data_ptr(), N + 8, M, N, K, st())
    torch.cuda.synchronize()
    what = f"gemm int8 M {M} K {K} columns {ncols} kpad {kpad}"
    check(h, want_linear(c1), what + " c_fc1")
    call(hip, "llj_gemm_i8_silu_mul", ad.data_ptr(), K + 8, ws_[2][0].data_ptr(), ws_[2][1].data_ptr(), ws.data_ptr(), P(ao),
         P(g2), kp, h.data_ptr(), N + 8, M, N, K, st())
    torch.cuda.synchronize()
    check(out, want_linear(c), what + " linear")
    check(xr, want_resid(c, x0), what + " resid")
    sp = SwigluPool()
    sp.add(h, None, c2["y16"].astype(f64), what + " silu_mul", a1=want_linear(c1))
    sp.finish(what + " silu_mul")
    if kpad is not None:
        check_gather(ao, [g0, g1, g2], c, [(x["cb"], x["scb"]) for x in (c, c1, c2)], kpad, what)


@pytest.mark.parametrize("ncols,kpad", [(0, None), (3, None), (33, None), (33, 64)])
@pytest.mark.parametrize("B,T_,S,p0", [(2, 20, 32, 20), (1, 300, 512, 300)])
def test_gemm_int8_qkv_rope_exact(hip, B, T_, S, p0, ncols, kpad):
    """llj_gemm_i8_qkv_rope, C = 128 (two heads of 64), B T = 40 and 300, a dyadic RoPE table, ring-wrapped
    positions: the whole q buffer and both whole caches."""
    C, nh = 128, 2
    hs, M = C // nh, B * T_
    c = H.i8_gemm_case(M, 3 * C, C, ncols)
    assert sca_inside(c)
    pos = np.arange(p0, p0 + T_, dtype=np.int32)
    rope = H.dyadic_rope(np.random.default_rng([23, M]), p0 + T_, hs)
    qe, kce, vce = qkv_want(c["y16"], B, T_, nh, hs, S, pos, rope)
    cbt, scb = dev_w(hip, c)
    ac = put(sentinel(M, C), c["a"])
    ws = stats_ws(hip, ac, C, M, C)
    ao, (g0,) = gathers(hip, ac, C, c, ws, [(cbt, scb, 3 * C)], kpad)
    rd, pd = T(rope), T(pos)
    q, kc, vc = sentinel(M + 1, C), sentinel(B * nh * S, hs), sentinel(B * nh * S, hs)
    call(hip, "llj_gemm_i8_qkv_rope", ac.data_ptr(), cbt.data_ptr(), scb.data_ptr(), ws.data_ptr(), P(ao), P(g0), kpad or 0,
         q.data_ptr(), kc.data_ptr(), vc.data_ptr(), rd.data_ptr(), pd.data_ptr(), B, T_, C, nh, S, st())
    torch.cuda.synchronize()
    what = f"gemm int8 qkv B {B} T {T_} columns {ncols} kpad {kpad}"
    check(q, qe, what + " q")
    check_cache(kc, kce, what + " k cache")
    check_cache(vc, vce, what + " v cache")


@pytest.mark.parametrize("total", [0, 1, 64, 65])
def test_gathers_exact(hip, total):
    """llj_i8_gather_act / llj_i8_gather_weight read directly: M = 3, N = 32, K = 256, kpad = 128, power-of-two
    and arbitrary fp32 SCB."""
    M, N, K, kpad = 3, 32, 256, 128
    rng = np.random.default_rng([29, total])
    c = H.i8_exact_case(M, N, K, rng.choice(K, total, replace=False), (5, 6, 5), 0, mutants=False)
    scb2 = rng.uniform(0.01, 3.0, N).astype(f32)
    cbt, scb = dev_w(hip, c)
    ad = a_operand(c["a"], K + 8)
    ws = stats_ws(hip, ad, K + 8, M, K)
    ao, (g0, g1) = gathers(hip, ad, K + 8, c, ws, [(cbt, scb, N), (cbt, T(scb2), N)], kpad)
    torch.cuda.synchronize()
    check_gather(ao, [g0, g1], c, [(c["cb"], c["scb"]), (c["cb"], scb2)], kpad, f"gather total {total}")


# ================================================================== the statistics workspace, every byte
def expect_ws(a, M, K, one_launch, thr=THR):
    """Every byte of the workspace (csrc/i8ws.h) after a statistics launch on a buffer of FILL bytes: header, aq,
    part, cnt, the first cnt list entries per k-block, sca, flag, avh[0] and -- after the one-launch prep -- the
    first cnt aval entries per k-block (f16 bits of rows 0 .. 7 of the listed column, rows >= M zero);
    everything else keeps the fill."""
    o = ws_offsets(M, K)
    kb = o["kb"]
    e = np.full(o["total"], FILL, np.uint8)
    a16 = a.astype(np.float16)
    ab = np.abs(a16.astype(f32))
    big = ab >= thr
    flag = big.any(0)
    small = np.where(big, f32(0), ab)
    sca = small.max(1).astype(f32)
    e[:16] = np.array([M, K, NSB, kb], np.int32).view(np.uint8)
    inv = np.where(sca > 0, f32(127) / np.where(sca > 0, sca, f32(1)), f32(0)).astype(f32)
    q = np.clip(np.rint(a16.astype(f32) * inv[:, None]), -127, 127)
    q[:, flag] = 0
    e[16:16 + M * K] = q.astype(np.int8).view(np.uint8).ravel()
    part = np.zeros((NSB, M), f32)
    cnt = np.zeros(NSB, np.int32)
    lst = e[o["list"]:o["sca"]].view(np.int32).reshape(NSB, kb)
    aval = e[o["aval"]:o["total"]].view(np.uint16).reshape(NSB, kb, 8)
    for b in range(NSB):
        blk = small[:, b * kb:(b + 1) * kb]
        if blk.size:
            part[b] = blk.max(1)
        cols = np.nonzero(flag[b * kb:(b + 1) * kb])[0] + b * kb
        cnt[b] = cols.size
        lst[b, :cols.size] = cols
        if one_launch:
            aval[b, :cols.size, :] = 0
            aval[b, :cols.size, :M] = a16[:, cols].view(np.uint16).T
    e[o["part"]:o["cnt"]] = part.view(np.uint8).ravel()
    e[o["cnt"]:o["list"]] = cnt.view(np.uint8)
    e[o["sca"]:o["sca"] + 4 * M] = sca.view(np.uint8)
    e[o["flag"]:o["flag"] + K] = flag.astype(np.uint8)
    e[o["avh"]:o["avh"] + 4] = np.array([1 if one_launch else 0], np.int32).view(np.uint8)
    return e, o


def check_ws(ws, a, M, K, one_launch, what):
    e, o = expect_ws(a, M, K, one_launch)
    got = ws.cpu().numpy()
    assert got.size == e.size
    names = ["aq", "part", "cnt", "list", "sca", "flag", "avh", "aval", "total"]
    for lo, hi, name in zip([0] + [o[n] for n in names[:-1]], [o[n] for n in names], ["header"] + names[:-1]):
        bad = np.nonzero(got[lo:hi] != e[lo:hi])[0]
        assert not bad.size, f"{what}: {bad.size} bytes of `{name}` differ, first at byte {bad[0]} of it"


def stats_rows(rng, M, K, kind):
    """bf16 rows with outliers; 6.0 (the threshold) and 5.96875 (the bf16 value just below it); an all-zero row
    (M >= 3); kind "allbig": one row with every element >= 6 (every column an outlier, every list full)."""
    a = bf16(rng.standard_normal((M, K)) * 2.0)
    a[rng.integers(0, M, 6), rng.integers(0, K, 6)] = rng.choice([6.0, -6.0, 9.0, -40.0], 6)
    a[0, 1], a[M - 1, 5], a[M // 2, K - 1] = 6.0, 5.96875, -40.0
    a[M - 1, 6:8] = [-5.96875, 0.00390625]
    if M >= 3:
        a[1] = 0.0
    if kind == "allbig":
        a[M // 2] = rng.choice([6.0, -6.0, 7.5, -100.0], K)
    return a.astype(f32)


@pytest.mark.parametrize("kind", ["mixed", "allbig"])
@pytest.mark.parametrize("K", [16, 32, 144, 640, 3200])
@pytest.mark.parametrize("M", [1, 8, 9, 31, 32, 33])
def test_stats_workspace_every_byte(hip, M, K, kind):
    """llj_i8_stats at lda > K: the one-launch prep (M <= 8: avh = 1 and the aval table), the two passes (9, 31:
    avh = 0) and the 2-D pass with its ragged 32-row group (32, 33), every byte of the workspace."""
    a = stats_rows(np.random.default_rng([31, M, K]), M, K, kind)
    ad = a_operand(a, K + 8)
    ws = stats_ws(hip, ad, K + 8, M, K)
    torch.cuda.synchronize()
    check_ws(ws, a, M, K, M <= 8, f"llj_i8_stats M {M} K {K} {kind}")


@pytest.mark.parametrize("K", [640, 3200])
@pytest.mark.parametrize("M", [3, 8, 12, 16, 20])
def test_norm_stats_exact(hip, M, K):
    """llj_i8_norm_stats with a norm on rows whose RMSNorm is exact (helpers.norm_rows, norm weights up to +-8 so
    that normalized outliers exist, +-6 among them: the threshold itself): xn bitwise the exact operand, the
    workspace the restatement on that xn.
    M = 3, 8: the one-launch prep; 12, 16: i8_norm_stats_kernel; 20: the two ops it replaces."""
    gvals = (-8, -6, -4, -3, -2, -1, 0, 1, 2, 3, 4, 6, 8)
    x, g, opnd, _ = H.norm_rows(np.random.default_rng([37, M, K]), M, K, gvals=gvals)
    assert (np.abs(opnd) == THR).any() and (np.abs(opnd) < THR).any()
    xd, gd = put(sentinel(M, K), x), T(g, torch.bfloat16)
    xn = sentinel(M + 1, K)
    ws = torch.full((hip.llj_i8_ws_bytes(M, K),), FILL, dtype=torch.uint8, device=dev)
    call(hip, "llj_i8_norm_stats", xd.data_ptr(), gd.data_ptr(), 1e-5, xn.data_ptr(), M, K, THR, ws.data_ptr(), st())
    torch.cuda.synchronize()
    check(xn, opnd, f"llj_i8_norm_stats xn M {M} K {K}")
    check_ws(ws, opnd.astype(f32), M, K, M <= 8, f"llj_i8_norm_stats M {M} K {K}")


# ================================================================== the any-shape kernel
F32_SENT = 0x7FA5A5A5


@pytest.mark.parametrize("resid", [False, True])
@pytest.mark.parametrize("dt", [0, 1])
def test_generic_int8_linear_exact(hip, dt, resid):
    """llj_g_i8_linear at shapes outside the streaming tiling, dt 0 (bf16) and dt 1 (fp32 holding fp16 values:
    the output is the fp16 value as fp32, bitwise), plain and with the residual added in place."""
    as16 = lambda y: np.asarray(y, f32).astype(np.float16).astype(f32)  # noqa: E731
    pool = H.I8Power(out=as16 if dt else bf16)
    for M, K, N, ncols in H.I8_GENERIC_SHAPES:
        c = H.i8_generic_case(M, K, N, ncols)
        assert sca_inside(c)
        pool.add(c)
        rng = np.random.default_rng([41, M, K, N])
        x0 = dyadic(rng, (M, N), 8, 16)
        cb, scb = T(c["cb"]), T(c["scb"])
        wsb = torch.full((hip.llj_g_i8_ws_bytes(M, K),), FILL, dtype=torch.uint8, device=dev)
        what = f"g_i8_linear M {M} K {K} N {N} dt {dt} resid {resid}"
        if dt == 0:
            ldx, ldy = K + 3, N + 5
            xd = put(torch.full((M, ldx), 1000.0, dtype=torch.bfloat16, device=dev).view(torch.int16), c["a"])
            y = put(sentinel(M + 1, ldy), x0) if resid else sentinel(M + 1, ldy)
            call(hip, "llj_g_i8_linear", xd.data_ptr(), ldx, M, K, cb.data_ptr(), scb.data_ptr(), THR, wsb.data_ptr(), N,
                 y.data_ptr(), ldy, y.data_ptr() if resid else None, ldy, 0, st())
            torch.cuda.synchronize()
            check(y, want_resid(c, x0) if resid else want_linear(c), what)
        else:
            ldx, ldy = K + 3, N + 5
            xd = torch.full((M, ldx), 1000.0, dtype=torch.float32, device=dev)
            xd[:, :K] = T(c["a"])
            y = torch.full((M + 1, ldy), F32_SENT, dtype=torch.int32, device=dev)
            if resid:
                y[:M, :N] = T(x0).view(torch.int32)
            call(hip, "llj_g_i8_linear", xd.data_ptr(), ldx, M, K, cb.data_ptr(), scb.data_ptr(), THR, wsb.data_ptr(), N,
                 y.data_ptr(), ldy, y.data_ptr() if resid else None, ldy, 1, st())
            torch.cuda.synchronize()
            got = y.cpu().numpy().view(np.uint32)
            want = (x0 + c["y16"]).astype(f32) if resid else c["y16"]  # one fp32 add, as the kernel's
            live = np.zeros(got.shape, bool)
            live[:M, :N] = True
            assert (got[~live] == F32_SENT).all(), f"{what}: words written outside the result"
            g = got[:M, :N].view(f32)
            assert not np.isnan(g).any() and np.array_equal(g, want), f"{what}: {(g != want).sum()} / {g.size} elements differ"
    pool.finish(f"g_i8_linear dt {dt}", ("inner", "dropcol", "halfaway") if dt else ("inner", "outer", "dropcol", "halfaway"))
