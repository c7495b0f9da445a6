"""The LoRA entry points (include/lit_llama_amd.h "LoRA"; reference lit_llama/lora.py).

llj_lora_merge is bitwise a numpy restatement on dyadic inputs (entries multiples of 1/8 in [-2, 2],
scaling 2: every sum is exact in any order) and reproduces the reference's own merged weight
(tests/golden/lora.npz). The unmerged forms (`llj_*_lora`) are compared with the composition of existing
ops: the Linear's rounded output y and the down-projection t from the plain Linear op of the same family,
torch for the reference's rounding points
    d = bf16(t_g . B_g^T);  y = bf16(y + bf16(d * scaling))          (lora.py:318-323 on bf16 tensors)
and llj_g_rope_kv for the split, RoPE and the cache write -- within the bound
tests/test_adapter_v2_kernels_gpu.py uses for its QKV comparisons (assert_bf16_close; torch sums the r
products in another order than the epilogue). Columns of a disabled group are bitwise the base op's, and
with lora_B = 0 every form is bitwise the base entry point.
"""
import numpy as np
import pytest
import torch

from lit_llama import _hip
from oracle import llama_np as O
from oracle.weights import Cfg, make_params
from tests.helpers import assert_bf16_close, bf16
from tests.test_adapter_v2_kernels_gpu import (GEMM_FMTS, P, colblock_operands, gemm_rows, rope_kv, stream_a,
                                               tpw_one)
from tests.test_kernels_gpu import T, W4G_128, call, option, quant_operands, st

pytestmark = pytest.mark.gpu
dev = "cuda"
BF = torch.bfloat16
C = 256
MASKS = {"TFT": [True, False, True], "TTT": [True, True, True], "FFT": [False, False, True]}


def mask_bits(en):
    return sum(1 << g for g, on in enumerate(en) if on)


# ------------------------------------------------------------------ merge
def merge_np(W, A, B, r, en, scaling, sign, rnd):
    """lora.py:270-277 restated: rnd = the weight type's rounding, at the reference's three points."""
    N, _ = W.shape
    Ng = N // 3
    out = W.copy()
    gi = 0
    for g in range(3):
        if not en[g]:
            continue
        d = rnd(B[gi * Ng:(gi + 1) * Ng].astype(np.float64) @ A[gi * r:(gi + 1) * r].astype(np.float64))
        out[g * Ng:(g + 1) * Ng] = rnd(W[g * Ng:(g + 1) * Ng] + np.float32(sign) * rnd(d * np.float32(scaling)))
        gi += 1
    return out


def dyadic(rng, shape):
    return (rng.integers(-16, 17, size=shape) / 8.0).astype(np.float32)


def run_merge(hip, W, A, B, r, en, scaling, sign):
    N, Kd = W.shape
    call(hip, "llj_lora_merge", W.data_ptr(), A.data_ptr(), B.data_ptr(), N, Kd, r, mask_bits(en), scaling, sign,
         0 if W.dtype == BF else 1, st())


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("r,Kd", [(8, 256), (5, 200)])  # K = 200: a partial column tile
def test_merge_bitwise_on_dyadic_inputs(hip, dt, mask, r, Kd):
    rng = np.random.default_rng(11 + r + len(mask) + (dt == "fp32"))
    en, tt = MASKS[mask], (BF if dt == "bf16" else torch.float32)
    rnd = bf16 if dt == "bf16" else (lambda v: np.asarray(v, np.float32))
    N, n_en = 3 * 80, sum(MASKS[mask])  # 80 rows per group: 2.5 row blocks
    W0, A, B = dyadic(rng, (N, Kd)), dyadic(rng, (r * n_en, Kd)), dyadic(rng, (N // 3 * n_en, r))
    Wd, Ad, Bd = T(W0, tt), T(A, tt), T(B, tt)
    run_merge(hip, Wd, Ad, Bd, r, en, 2.0, 1)
    want = merge_np(W0, A, B, r, en, 2.0, 1, rnd)
    got = Wd.float().cpu().numpy()
    np.testing.assert_array_equal(got, want)
    assert not np.array_equal(got, W0)
    for g in range(3):  # rows of disabled groups are untouched
        if not en[g]:
            np.testing.assert_array_equal(got[g * 80:(g + 1) * 80], W0[g * 80:(g + 1) * 80])
    run_merge(hip, Wd, Ad, Bd, r, en, 2.0, -1)
    back = Wd.float().cpu().numpy()
    np.testing.assert_array_equal(back, merge_np(want, A, B, r, en, 2.0, -1, rnd))
    if dt == "fp32":  # exact sums: unmerge restores the weight
        np.testing.assert_array_equal(back, W0)


def test_merge_refuses_bad_arguments(hip):
    W, A, B = (torch.zeros(s, dtype=BF, device=dev) for s in ((48, 128), (16, 128), (32, 8)))
    args = lambda **kw: [W.data_ptr(), A.data_ptr(), B.data_ptr(), kw.get("N", 48), 128, kw.get("r", 8),  # noqa: E731
                         kw.get("mask", 5), 2.0, kw.get("sign", 1), kw.get("dt", 0), st()]
    assert hip.llj_lora_merge(*args()) == 0
    for bad in (dict(r=0), dict(r=65), dict(mask=0), dict(mask=8), dict(sign=0), dict(dt=2), dict(N=47)):
        assert hip.llj_lora_merge(*args(**bad)) == 1000, bad


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_merge_matches_reference_weight(hip, golden, dt):
    """Layer 0's c_attn of the fixture model: the reference's eval() merge in bf16 (bitwise) and fp32, on
    the rows the fixture stores (64 of q, 16 of k -- disabled, the pretrained rows --, 64 of v)."""
    g = golden("lora")
    cfg = Cfg(block_size=128, n_layer=4, n_head=4, n_embd=256, vocab_size=2048)
    W0 = make_params(cfg, int(g["seed"]))["transformer.h.0.attn.c_attn.weight"]
    tt = BF if dt == "bf16" else torch.float32
    Wd = T(W0, tt)
    Ad = T(g["lora/transformer.h.0.attn.c_attn.lora_A"], tt)
    Bd = T(g["lora/transformer.h.0.attn.c_attn.lora_B"], tt)
    r, scaling = int(g["r"]), float(g["alpha"]) / int(g["r"])
    run_merge(hip, Wd, Ad, Bd, r, MASKS["TFT"], scaling, 1)
    rows = g["merged_w0_rows"]
    got = Wd.float().cpu().numpy()[rows]
    assert not np.array_equal(got, T(W0, tt).float().cpu().numpy()[rows])
    if dt == "bf16":
        want = (g["merged_w0_bf16_bits"].astype(np.uint32) << 16).view(np.float32)
        nbad = int((got != want).sum())
        print(f"[lora] bf16 merge vs the reference's: {nbad} of {got.size} elements differ")
        np.testing.assert_array_equal(got, want)
    else:
        want = g["merged_w0_fp32"]
        rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
        print(f"[lora] fp32 merge vs the reference's: rel {rel:.2e}")
        assert rel <= 1e-6, rel


# ------------------------------------------------------------------ unmerged forms
def lora_ops(rng, r, en, Cd, tt=BF, zero_b=False, rows=16):
    """(lora_A (r n_en, Cd), its zero-padded image of a multiple of `rows` rows, lora_B (n_en Cd, r))."""
    n_en = sum(en)
    A = bf16(rng.standard_normal((r * n_en, Cd)) / np.sqrt(Cd))
    Bm = np.zeros((n_en * Cd, r), np.float32) if zero_b else bf16(0.3 * rng.standard_normal((n_en * Cd, r)))
    img = np.zeros(((r * n_en + rows - 1) // rows * rows, Cd), np.float32)
    img[:r * n_en] = A
    return T(A, tt), T(img, tt), T(Bm, tt)


def add_lora(y, t, Bd, r, en, scaling):
    """lora.py:318-323 on tensors of y's type: per enabled group d = t_g . B_g^T rounded, times scaling
    rounded, added to y's columns of that group rounded; disabled groups untouched."""
    Ng = y.shape[1] // 3
    out = y.clone()
    gi = 0
    for g in range(3):
        if not en[g]:
            continue
        d = (t[:, gi * r:(gi + 1) * r].float() @ Bd[gi * Ng:(gi + 1) * Ng].float().T).to(y.dtype)
        out[:, g * Ng:(g + 1) * Ng] = y[:, g * Ng:(g + 1) * Ng] + d * scaling
        gi += 1
    return out


def norm_linear(hip, wfmt, xd, gd, Wd, szd, N):
    M = xd.shape[0]
    out = torch.empty(M, N, dtype=BF, device=dev)
    call(hip, "llj_norm_linear", wfmt, xd.data_ptr(), gd.data_ptr(), 1e-5, Wd.data_ptr(), P(szd), out.data_ptr(), N,
         M, N, C, None, 0, None, None, 0, st())
    return out


RANK_MASKS = [(4, "TFT"), (8, "TFT"), (16, "TFT"), (8, "TTT"), (4, "FFT"), (16, "TTT"), (8, "FFT")]


@pytest.mark.parametrize("wfmt", [0, 1, 3, W4G_128])
@pytest.mark.parametrize("nh", [4, 2])  # head size 64 and 128
@pytest.mark.parametrize("B,sa", [(1, 1), (2, 1), (8, 1), (8, 0)])  # one row, streamed rows, the LDS image
def test_norm_qkv_rope_lora(hip, wfmt, nh, B, sa):
    """Cache length 16 with the position past it (ring wrap); every rank / mask pair (48 tiles: one tile per
    workgroup -- the multi-tile forms are test_norm_qkv_rope_lora_multi_tile's)."""
    rng = np.random.default_rng(1400 + wfmt + 7 * B + nh + sa)
    hs, S, p0 = C // nh, 16, 37
    _, Wd, szd = quant_operands(hip, rng, wfmt, 3 * C, C)
    xd = T(bf16(rng.standard_normal((B, C))), BF)
    gd = T(bf16(rng.uniform(0.5, 1.5, C)), BF)
    rope, pos = T(O.build_rope_cache(128, hs)), T(np.array([p0], np.int32))

    def fused(name, *tail):
        q = torch.zeros(B, C, dtype=BF, device=dev)
        kc = torch.zeros(B, nh, S, hs, dtype=BF, device=dev)
        vc = torch.zeros_like(kc)
        call(hip, name, wfmt, xd.data_ptr(), gd.data_ptr(), 1e-5, Wd.data_ptr(), P(szd), q.data_ptr(), kc.data_ptr(),
             vc.data_ptr(), rope.data_ptr(), pos.data_ptr(), B, 1, C, nh, S, 0, B, None, None, None, 0, st(), *tail)
        return q, kc, vc

    with stream_a(hip, sa):
        y = norm_linear(hip, wfmt, xd, gd, Wd, szd, 3 * C)
        base = fused("llj_norm_qkv_rope")
        for r, mask in RANK_MASKS:
            en, scaling = MASKS[mask], 16.0 / r
            _, img, Bd = lora_ops(rng, r, en, C)
            _, _, B0 = lora_ops(rng, r, en, C, zero_b=True)
            t = norm_linear(hip, 1, xd, gd, img, None, img.shape[0])
            assert t.shape[1] % 16 == 0 and (r != 4 or t.shape[1] == 16)  # r = 4: rows of t padded to 16
            # (here and below) rope_kv is llj_g_rope_kv, itself checked: tests/test_generic_kernels_gpu.py::test_rope_kv_*
            want = rope_kv(hip, add_lora(y, t, Bd, r, en, scaling).contiguous(), B, 1, nh, hs, S, rope, pos)
            tail = (t.data_ptr(), t.stride(0), Bd.data_ptr(), r, mask_bits(en), scaling)
            got = fused("llj_norm_qkv_rope_lora", *tail)
            zero = fused("llj_norm_qkv_rope_lora", t.data_ptr(), t.stride(0), B0.data_ptr(), r, mask_bits(en), scaling)
            null = fused("llj_norm_qkv_rope_lora", None, 0, None, 0, 0, 0.0)
            for gidx, (name, a, b, c) in enumerate(zip(("q", "k cache", "v cache"), got, want, base)):
                what = f"{name} r={r} mask={mask}"
                assert_bf16_close(a.float().cpu().numpy(), b.float().cpu().numpy(), what)
                assert torch.equal(zero[gidx], c), what  # lora_B = 0: the base op
                assert torch.equal(null[gidx], c), what  # no operands: the base op
                assert torch.equal(a, c) == (not en[gidx]), what  # a disabled group: bitwise the base op's
            assert got[1].abs().sum() == got[1][:, :, p0 % S].abs().sum() > 0  # only slot p0 % S written


@pytest.mark.parametrize("wfmt", [0, 3])
def test_norm_qkv_rope_lora_multi_tile(hip, wfmt):
    """The flat QKV epilogue with the LoRA term at two tiles per workgroup: C = 1408 (11 heads of 128), 264
    tiles, M = 8 rows; bitwise the one-tile-per-workgroup launch (llj_set_tpw_max 1)."""
    rng = np.random.default_rng(1450 + wfmt)
    B, nh, hs, S, p0 = 8, 11, 128, 16, 37
    Cq = nh * hs
    _, Wd, szd = quant_operands(hip, rng, wfmt, 3 * Cq, Cq)
    xd = T(bf16(rng.standard_normal((B, Cq))), BF)
    rope, pos = T(O.build_rope_cache(128, hs)), T(np.array([p0], np.int32))

    def plain(wf, Wm, sz, N):
        out = torch.empty(B, N, dtype=BF, device=dev)
        call(hip, "llj_linear", wf, xd.data_ptr(), Cq, Wm.data_ptr(), P(sz), None, out.data_ptr(), N, B, N, Cq, None, 0,
             None, st())
        return out

    y = plain(wfmt, Wd, szd, 3 * Cq)
    for r, mask in ((8, "TFT"), (16, "TTT")):
        en, scaling = MASKS[mask], 16.0 / r
        _, img, Bd = lora_ops(rng, r, en, Cq)
        t = plain(1, img, None, img.shape[0])

        def fused():
            q = torch.zeros(B, Cq, dtype=BF, device=dev)
            kc = torch.zeros(B, nh, S, hs, dtype=BF, device=dev)
            vc = torch.zeros_like(kc)
            call(hip, "llj_norm_qkv_rope_lora", wfmt, xd.data_ptr(), None, 0.0, Wd.data_ptr(), P(szd), q.data_ptr(),
                 kc.data_ptr(), vc.data_ptr(), rope.data_ptr(), pos.data_ptr(), B, 1, Cq, nh, S, 0, B, None, None, None,
                 0, st(), t.data_ptr(), t.stride(0), Bd.data_ptr(), r, mask_bits(en), scaling)
            return q, kc, vc

        want = rope_kv(hip, add_lora(y, t, Bd, r, en, scaling).contiguous(), B, 1, nh, hs, S, rope, pos)
        got, one = fused(), tpw_one(hip, fused)
        for name, a, b, c in zip(("q", "k cache", "v cache"), got, want, one):
            assert torch.equal(a, c), name
            assert_bf16_close(a.float().cpu().numpy(), b.float().cpu().numpy(), f"{name} r={r} mask={mask}")


def test_norm_qkv_rope_lora_row_slices(hip):
    """Row slices of a larger batch (row0 > 0: t is indexed by the global row)."""
    rng = np.random.default_rng(1500)
    wfmt, nh, hs, S, M, r = 0, 4, 64, 16, 12, 8
    en, scaling = MASKS["TFT"], 2.0
    _, Wd, szd = quant_operands(hip, rng, wfmt, 3 * C, C)
    xd = T(bf16(rng.standard_normal((M, C))), BF)
    gd = T(bf16(rng.uniform(0.5, 1.5, C)), BF)
    rope, pos = T(O.build_rope_cache(128, hs)), T(np.array([5], np.int32))
    _, img, Bd = lora_ops(rng, r, en, C)
    t = torch.cat([norm_linear(hip, 1, xd[i:i + 8].contiguous(), gd, img, None, 16) for i in (0, 8)])
    y = torch.cat([norm_linear(hip, wfmt, xd[i:i + 8].contiguous(), gd, Wd, szd, 3 * C) for i in (0, 8)])
    want = rope_kv(hip, add_lora(y, t, Bd, r, en, scaling).contiguous(), M, 1, nh, hs, S, rope, pos)
    q = torch.zeros(M, C, dtype=BF, device=dev)
    kc = torch.zeros(M, nh, S, hs, dtype=BF, device=dev)
    vc = torch.zeros_like(kc)
    for r0 in (0, 8):
        call(hip, "llj_norm_qkv_rope_lora", wfmt, xd.data_ptr(), gd.data_ptr(), 1e-5, Wd.data_ptr(), P(szd), q.data_ptr(),
             kc.data_ptr(), vc.data_ptr(), rope.data_ptr(), pos.data_ptr(), M, 1, C, nh, S, r0, min(8, M - r0), None,
             None, None, 0, st(), t.data_ptr(), t.stride(0), Bd.data_ptr(), r, mask_bits(en), scaling)
    for name, a, b in zip(("q", "k cache", "v cache"), (q, kc, vc), want):
        assert_bf16_close(a.float().cpu().numpy(), b.float().cpu().numpy(), name)


def test_lora_argument_rules(hip):
    """A partial operand set, a rank outside 1..64, an empty mask and wfmt 2 return LLJ_EINVAL."""
    rng = np.random.default_rng(1600)
    nh, hs, S, B, r = 4, 64, 16, 2, 8
    _, Wd, szd = quant_operands(hip, rng, 0, 3 * C, C)
    xd = T(bf16(rng.standard_normal((B, C))), BF)
    rope, pos = T(O.build_rope_cache(128, hs)), T(np.array([3], np.int32))
    _, img, Bd = lora_ops(rng, r, MASKS["TFT"], C)
    t = torch.zeros(B, 16, dtype=BF, device=dev)
    q = torch.zeros(B, C, dtype=BF, device=dev)
    kc = torch.zeros(B, nh, S, hs, dtype=BF, device=dev)
    vc = torch.zeros_like(kc)

    def rc(wfmt, *tail):
        return hip.llj_norm_qkv_rope_lora(wfmt, xd.data_ptr(), None, 0.0, Wd.data_ptr(), P(szd), q.data_ptr(),
                                          kc.data_ptr(), vc.data_ptr(), rope.data_ptr(), pos.data_ptr(), B, 1, C, nh, S,
                                          0, B, None, None, None, 0, st(), *tail)

    assert rc(0, t.data_ptr(), 16, Bd.data_ptr(), r, 5, 2.0) == 0
    assert rc(0, None, 16, Bd.data_ptr(), r, 5, 2.0) == 1000
    assert rc(0, t.data_ptr(), 16, None, r, 5, 2.0) == 1000
    assert rc(0, t.data_ptr(), 16, Bd.data_ptr(), 0, 5, 2.0) == 1000
    assert rc(0, t.data_ptr(), 16, Bd.data_ptr(), 65, 5, 2.0) == 1000
    assert rc(0, t.data_ptr(), 16, Bd.data_ptr(), r, 0, 2.0) == 1000
    assert rc(0, t.data_ptr(), 8, Bd.data_ptr(), r, 5, 2.0) == 1000  # ldt < r * n_en
    assert rc(2, t.data_ptr(), 16, Bd.data_ptr(), r, 5, 2.0) == 1000
    assert hip.llj_gemm_qkv_rope_lora(2, xd.data_ptr(), Wd.data_ptr(), P(szd), q.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                                      rope.data_ptr(), pos.data_ptr(), 1, B, C, nh, S, st(), t.data_ptr(), 16,
                                      Bd.data_ptr(), r, 5, 2.0) == 1000
    assert hip.llj_gemm_qkv_rope_lora(0, xd.data_ptr(), Wd.data_ptr(), P(szd), q.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                                      rope.data_ptr(), pos.data_ptr(), 1, B, C, nh, S, st(), t.data_ptr(), 16, None, r,
                                      5, 2.0) == 1000


@pytest.mark.parametrize("wfmt", GEMM_FMTS)
@pytest.mark.parametrize("M,glds", [(64, 0), (256, 0), (256, 1)])  # M = 256 with glds: the LDS-DMA kernel
def test_gemm_qkv_rope_lora(hip, wfmt, M, glds):
    rng = np.random.default_rng(1700 + (wfmt & 0xFFFF) + M + glds + (wfmt >> 17))
    nh, hs, S = 4, 64, 512
    _, Wq, sq = quant_operands(hip, rng, wfmt, 3 * C, C)
    xd = T(bf16(rng.standard_normal((M, C))), BF)
    rope, pos = T(O.build_rope_cache(512, hs)), T(np.arange(5, 5 + M, dtype=np.int32))

    def fused(name, *tail):
        q = torch.zeros(M, C, dtype=BF, device=dev)
        kc = torch.zeros(1, nh, S, hs, dtype=BF, device=dev)
        vc = torch.zeros_like(kc)
        call(hip, name, wfmt, xd.data_ptr(), Wq.data_ptr(), P(sq), q.data_ptr(), kc.data_ptr(), vc.data_ptr(),
             rope.data_ptr(), pos.data_ptr(), 1, M, C, nh, S, st(), *tail)
        return q, kc, vc

    with option(hip, _hip.OPT_GEMM_GLDS, glds):
        y = gemm_rows(hip, wfmt, xd, Wq, sq, 3 * C, C)
        base = fused("llj_gemm_qkv_rope")
        for r, mask in ((8, "TFT"), (16, "TTT"), (4, "FFT")):
            en, scaling = MASKS[mask], 16.0 / r
            _, img, Bd = lora_ops(rng, r, en, C, rows=128)
            _, _, B0 = lora_ops(rng, r, en, C, zero_b=True)
            t = gemm_rows(hip, 1, xd, img, None, 128, C)
            want = rope_kv(hip, add_lora(y, t, Bd, r, en, scaling).contiguous(), 1, M, nh, hs, S, rope, pos)
            got = fused("llj_gemm_qkv_rope_lora", t.data_ptr(), 128, Bd.data_ptr(), r, mask_bits(en), scaling)
            zero = fused("llj_gemm_qkv_rope_lora", t.data_ptr(), 128, B0.data_ptr(), r, mask_bits(en), scaling)
            null = fused("llj_gemm_qkv_rope_lora", None, 0, None, 0, 0, 0.0)
            for gidx, (name, a, b, c) in enumerate(zip(("q", "k cache", "v cache"), got, want, base)):
                what = f"gemm {name} r={r} mask={mask}"
                assert_bf16_close(a.float().cpu().numpy(), b.float().cpu().numpy(), what)
                assert torch.equal(zero[gidx], c) and torch.equal(null[gidx], c), what
                assert torch.equal(a, c) == (not en[gidx]), what


@pytest.mark.parametrize("kind", ["bf16", "fp32", "q4"])
def test_g_linear_lora(hip, kind):
    """The any-shape kernel at K = 780 (the 125M config's n_embd), N = 48 (16 columns per group), M = 11 (two
    row blocks): dense bf16 and fp32, and ColBlock int4 (wkind 0) with bf16 activations."""
    rng = np.random.default_rng(1800 + len(kind))
    M, N, Kd = 11, 48, 780
    dt = 1 if kind == "fp32" else 0
    tt = torch.float32 if dt else BF
    xd = T(bf16(rng.standard_normal((M, Kd))), tt)
    if kind == "q4":
        wkind, bits, group = 0, 4, 260
        W, scl, zr = colblock_operands(rng, N, Kd, bits, group)
    else:
        wkind, W, scl, zr, bits, group = 1, T(bf16(rng.standard_normal((N, Kd)) / np.sqrt(Kd)), tt), None, None, 16, Kd

    def run(name, Wm, Nn, *tail, wk=wkind, s=scl, z=zr, b=bits, gp=group):
        y = torch.empty(M, Nn, dtype=tt, device=dev)
        call(hip, name, wk, xd.data_ptr(), Kd, M, Kd, Wm.data_ptr(), P(s), P(z), b, gp, Nn, y.data_ptr(), Nn, None, 0, dt,
             st(), *tail)
        return y

    base = run("llj_g_linear", W, N)
    for r, mask in ((8, "TFT"), (5, "TTT"), (4, "FFT")):
        en, scaling = MASKS[mask], 16.0 / r
        n_en, Ng = sum(en), N // 3
        A = T(bf16(rng.standard_normal((r * n_en, Kd)) / np.sqrt(Kd)), tt)
        Bd = T(bf16(0.3 * rng.standard_normal((n_en * Ng, r))), tt)
        t = run("llj_g_linear", A, r * n_en, wk=1, s=None, z=None, b=16, gp=Kd)
        want = add_lora(base, t, Bd, r, en, scaling)
        tail = (t.data_ptr(), t.stride(0), Bd.data_ptr(), r, mask_bits(en), scaling)
        got = run("llj_g_linear_lora", W, N, *tail)
        if dt:
            torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)
        else:
            assert_bf16_close(got.float().cpu().numpy(), want.float().cpu().numpy(), f"g_linear_lora {kind} {mask}")
        for g in range(3):
            same = torch.equal(got[:, g * Ng:(g + 1) * Ng], base[:, g * Ng:(g + 1) * Ng])
            assert same == (not en[g]), (kind, mask, g)
        assert torch.equal(run("llj_g_linear_lora", W, N, t.data_ptr(), t.stride(0), torch.zeros_like(Bd).data_ptr(), r,
                               mask_bits(en), scaling), base)
        assert torch.equal(run("llj_g_linear_lora", W, N, None, 0, None, 0, 0, 0.0), base)
