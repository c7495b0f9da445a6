"""The adapter v2 entry points (`llj_*_v2`: a per-column scale and bias in the epilogue of the op of the
same name, reference lit_llama/adapter_v2.py:28-31) against the composition of the existing ops:

    llj_linear -> torch bf16 (y + adapter_bias) * adapter_scale  [-> llj_g_rope_kv | -> llj_g_silu_mul |
                                                                     -> torch bf16 residual add]

The composition rounds where the fused epilogue does (the Linear's output, the sum, the product, then
the consumer from a bf16 value), so the results are compared bitwise -- except the SwiGLU forms, whose
in-kernel SiLU uses __expf and llj_g_silu_mul expf: they take the bound of
tests/test_kernels_gpu.py::test_fused_swiglu_and_resid (assert_bf16_close, rel 3e-2), and the RoPE'd q / k
of the QKV forms, where the fused epilogue and llj_g_rope_kv contract the fp32 rotation differently (an
ulp on a bf16 rounding boundary): the bound of test_fused_qkv_rope_kv; v stays bitwise. With scale 1 and
bias 0 every form is bitwise the existing entry point. Scale (+-U(0.5, 1.5)) and bias differ per
column, so a wrong column index cannot pass.
"""
import numpy as np
import pytest
import torch

from lit_llama import _hip
from oracle import llama_np as O
from tests.helpers import assert_bf16_close, bf16
from tests.test_kernels_gpu import T, W4G_128, call, option, quant_operands, st

pytestmark = pytest.mark.gpu
dev = "cuda"
FMTS = [0, 1, 3, W4G_128]
K, C, H = 256, 256, 768
BF = torch.bfloat16


def P(t):
    return None if t is None else t.data_ptr()


def vecs(rng, N, identity=False):
    """(adapter_scale, adapter_bias) bf16 device vectors of N, distinct per column."""
    if identity:
        return torch.ones(N, dtype=BF, device=dev), torch.zeros(N, dtype=BF, device=dev)
    sc = rng.uniform(0.5, 1.5, N) * rng.choice([-1.0, 1.0], N)
    return T(bf16(sc), BF), T(bf16(0.3 * rng.standard_normal(N)), BF)


def affine(y, sc, bi):
    """adapter_v2.py:28-31 on bf16 tensors: every op rounds."""
    assert y.dtype == BF
    return sc * (y + bi)


def linear(hip, wfmt, xd, Wd, szd, N, Kd):
    M = xd.shape[0]
    out = torch.empty(M, N, dtype=BF, device=dev)
    call(hip, "llj_linear", wfmt, xd.data_ptr(), Kd, Wd.data_ptr(), P(szd), None, out.data_ptr(), N, M, N, Kd, None, 0,
         None, st())
    return out


class stream_a:
    def __init__(self, hip, mode):
        self.hip, self.mode = hip, mode

    def __enter__(self):
        self.old = self.hip.llj_set_stream_a(self.mode)

    def __exit__(self, *exc):
        self.hip.llj_set_stream_a(self.old)


# row modes of the decode GEMVs: one row, streamed 2..8 rows, the LDS image of 2..8 rows (streaming off)
ROW_MODES = [(1, 1), (2, 1), (8, 1), (8, 0)]


@pytest.mark.parametrize("wfmt", FMTS)
@pytest.mark.parametrize("M,sa", ROW_MODES + [(16, 1)])
def test_linear_v2(hip, wfmt, M, sa):
    """llj_linear_v2 / llj_norm_linear_v2 (norm_w NULL), N = 80: 5 tiles; M = 16: the global-A form."""
    rng = np.random.default_rng(wfmt + 7 * M + sa)
    N = 80
    _, Wd, szd = quant_operands(hip, rng, wfmt, N, K)
    xd = T(bf16(rng.standard_normal((M, K))), BF)
    sc, bi = vecs(rng, N)
    one, zero = vecs(rng, N, identity=True)
    with stream_a(hip, sa):
        base = linear(hip, wfmt, xd, Wd, szd, N, K)
        want = affine(base, sc, bi)
        for s_, b_, ref in ((sc, bi, want), (one, zero, base), (None, None, base)):
            out = torch.empty(M, N, dtype=BF, device=dev)
            call(hip, "llj_linear_v2", wfmt, xd.data_ptr(), K, Wd.data_ptr(), P(szd), None, out.data_ptr(), N, M, N, K,
                 None, 0, None, st(), P(s_), P(b_))
            assert torch.equal(out, ref)
            if M <= 8:
                out2 = torch.empty(M, N, dtype=BF, device=dev)
                call(hip, "llj_norm_linear_v2", wfmt, xd.data_ptr(), None, 0.0, Wd.data_ptr(), P(szd), out2.data_ptr(),
                     N, M, N, K, None, 0, None, None, 0, st(), P(s_), P(b_))
                assert torch.equal(out2, ref)
    assert not torch.equal(want, base)
    # one vector without the other is refused
    assert hip.llj_linear_v2(wfmt, xd.data_ptr(), K, Wd.data_ptr(), P(szd), None, out.data_ptr(), N, M, N, K, None, 0,
                             None, st(), sc.data_ptr(), None) == 1000


@pytest.mark.parametrize("wfmt", [0, 3])
@pytest.mark.parametrize("N", [16 * 261, 16 * 769])
def test_linear_v2_multi_tile(hip, wfmt, N):
    """Several tiles per workgroup (M = 8, more tiles than compute units: 2 and 4 per workgroup, the last
    workgroup partial): every tile slot takes its own columns' scale and bias."""
    rng = np.random.default_rng(N + wfmt)
    M = 8
    _, Wd, szd = quant_operands(hip, rng, wfmt, N, K)
    xd = T(bf16(rng.standard_normal((M, K))), BF)
    sc, bi = vecs(rng, N)
    want = affine(linear(hip, wfmt, xd, Wd, szd, N, K), sc, bi)
    out = torch.empty(M, N, dtype=BF, device=dev)
    call(hip, "llj_linear_v2", wfmt, xd.data_ptr(), K, Wd.data_ptr(), P(szd), None, out.data_ptr(), N, M, N, K, None, 0,
         None, st(), sc.data_ptr(), bi.data_ptr())
    assert torch.equal(out, want)
    old = hip.llj_set_tpw_max(1)
    try:
        out1 = torch.empty(M, N, dtype=BF, device=dev)
        call(hip, "llj_linear_v2", wfmt, xd.data_ptr(), K, Wd.data_ptr(), P(szd), None, out1.data_ptr(), N, M, N, K, None,
             0, None, st(), sc.data_ptr(), bi.data_ptr())
    finally:
        hip.llj_set_tpw_max(old)
    assert torch.equal(out1, want)


def nstat_of(x, M, N):
    """per 16-column tile and row, the fp32 sum of the bf16-rounded squares of the new x: [N / 16][16]"""
    sq = (x * x).float().view(M, N // 16, 16).sum(-1)  # x * x in bf16 (model.py:281)
    out = torch.zeros(N // 16, 16, dtype=torch.float32, device=dev)
    out[:, :M] = sq.t()
    return out


@pytest.mark.parametrize("wfmt", FMTS)
@pytest.mark.parametrize("M,sa", ROW_MODES)
def test_linear_resid_v2(hip, wfmt, M, sa):
    """mlp.c_proj shape (K = H = 768, N = C = 256): x + affine(h . W^T) and the hand-off statistics."""
    rng = np.random.default_rng(100 + wfmt + 7 * M + sa)
    _, Wd, szd = quant_operands(hip, rng, wfmt, C, H)
    hd = T(bf16(rng.standard_normal((M, H))), BF)
    x0 = T(bf16(rng.standard_normal((M, C))), BF)
    sc, bi = vecs(rng, C)
    one, zero = vecs(rng, C, identity=True)
    with stream_a(hip, sa):
        want = x0 + affine(linear(hip, wfmt, hd, Wd, szd, C, H), sc, bi)
        xe, ne = x0.clone(), torch.zeros(C // 16, 16, dtype=torch.float32, device=dev)
        call(hip, "llj_linear_resid", wfmt, hd.data_ptr(), H, Wd.data_ptr(), P(szd), xe.data_ptr(), C, M, C, H, None, 0,
             ne.data_ptr(), st())
        for s_, b_, ref, nref in ((sc, bi, want, None), (one, zero, xe, ne), (None, None, xe, ne)):
            x, ns = x0.clone(), torch.zeros(C // 16, 16, dtype=torch.float32, device=dev)
            call(hip, "llj_linear_resid_v2", wfmt, hd.data_ptr(), H, Wd.data_ptr(), P(szd), x.data_ptr(), C, M, C, H,
                 None, 0, ns.data_ptr(), st(), P(s_), P(b_))
            assert torch.equal(x, ref)
            if nref is not None:
                assert torch.equal(ns, nref)
            # sums of 16 fp32 values in another order: a few ulp
            torch.testing.assert_close(ns, nstat_of(x, M, C), rtol=1e-5, atol=1e-6)
    assert not torch.equal(want, xe)


@pytest.mark.parametrize("wfmt", [0, 1, 3])
def test_linear_resid_attn_v2(hip, wfmt):
    """attn.c_proj on the merged attention partials of one row (AM_MERGE). The Linear's own bf16 output
    is llj_linear_resid_attn on a zero residual, so x0 + affine(that) is the composition."""
    rng = np.random.default_rng(300 + wfmt)
    nh, hs, S, nsplit, p0 = 4, 64, 48, 2, 40
    kc, vc = (T(bf16(rng.standard_normal((1, nh, S, hs))), BF) for _ in range(2))
    qd, pd = T(bf16(rng.standard_normal((1, C)) * 2), BF), T(np.array([p0], np.int32))
    part = torch.full((hip.llj_attention_ws_bytes(1, nh, hs, nsplit),), 0xFF, dtype=torch.uint8, device=dev)
    call(hip, "llj_attention_part", qd.data_ptr(), kc.data_ptr(), vc.data_ptr(), pd.data_ptr(), 1, 1, nh, hs, S, nsplit,
         part.data_ptr(), st())
    _, Wd, szd = quant_operands(hip, rng, wfmt, C, C)
    x0 = T(bf16(rng.standard_normal((1, C))), BF)
    sc, bi = vecs(rng, C)
    one, zero = vecs(rng, C, identity=True)

    def old(x):
        ns = torch.zeros(C // 16, 16, dtype=torch.float32, device=dev)
        call(hip, "llj_linear_resid_attn", wfmt, part.data_ptr(), nsplit, nh, Wd.data_ptr(), P(szd), x.data_ptr(), C, C, C,
             ns.data_ptr(), st())
        return x, ns

    lin, _ = old(torch.zeros(1, C, dtype=BF, device=dev))
    xe, ne = old(x0.clone())
    want = x0 + affine(lin, sc, bi)
    for s_, b_, ref in ((sc, bi, want), (one, zero, xe), (None, None, xe)):
        x, ns = x0.clone(), torch.zeros(C // 16, 16, dtype=torch.float32, device=dev)
        call(hip, "llj_linear_resid_attn_v2", wfmt, part.data_ptr(), nsplit, nh, Wd.data_ptr(), P(szd), x.data_ptr(), C,
             C, C, ns.data_ptr(), st(), P(s_), P(b_))
        assert torch.equal(x, ref)
        torch.testing.assert_close(ns, nstat_of(x, 1, C), rtol=1e-5, atol=1e-6)
    assert not torch.equal(want, xe)


@pytest.mark.parametrize("wfmt", FMTS)
@pytest.mark.parametrize("M,sa", ROW_MODES)
def test_norm_swiglu_v2(hip, wfmt, M, sa):
    """Two independent (scale, bias) pairs for c_fc1 and c_fc2 before silu and the product."""
    rng = np.random.default_rng(200 + wfmt + 7 * M + sa)
    _, W1d, s1 = quant_operands(hip, rng, wfmt, H, C)
    _, W2d, s2 = quant_operands(hip, rng, wfmt, H, C)
    xd = T(bf16(rng.standard_normal((M, C))), BF)
    sc1, bi1 = vecs(rng, H)
    sc2, bi2 = vecs(rng, H)
    one, zero = vecs(rng, H, identity=True)
    with stream_a(hip, sa):
        a1 = affine(linear(hip, wfmt, xd, W1d, s1, H, C), sc1, bi1).contiguous()
        a2 = affine(linear(hip, wfmt, xd, W2d, s2, H, C), sc2, bi2).contiguous()
        want = torch.empty(M, H, dtype=BF, device=dev)
        # (here and below) the borrowed oracle is itself checked: tests/test_generic_kernels_gpu.py::test_silu_mul_*
        call(hip, "llj_g_silu_mul", a1.data_ptr(), a2.data_ptr(), want.data_ptr(), M * H, 0, st())
        he =torch.empty(M, H, dtype=BF, device=dev)
        call(hip, "llj_norm_swiglu", wfmt, xd.data_ptr(), None, 0.0, W1d.data_ptr(), P(s1), W2d.data_ptr(), P(s2),
             he.data_ptr(), M, H, C, None, 0, None, None, 0, st())

        def v2(p1, p2):
            h = torch.empty(M, H, dtype=BF, device=dev)
            call(hip, "llj_norm_swiglu_v2", wfmt, xd.data_ptr(), None, 0.0, W1d.data_ptr(), P(s1), W2d.data_ptr(), P(s2),
                 h.data_ptr(), M, H, C, None, 0, None, None, 0, st(), P(p1[0]), P(p1[1]), P(p2[0]), P(p2[1]))
            return h

        got = v2((sc1, bi1), (sc2, bi2))
        # in-kernel __expf SiLU vs llj_g_silu_mul's expf: test_fused_swiglu_and_resid's bound
        assert_bf16_close(got.float().cpu().numpy(), want.float().cpu().numpy(), "swiglu v2", rel=3e-2)
        assert torch.equal(v2((one, zero), (one, zero)), he)
        assert torch.equal(v2((None, None), (None, None)), he)
        # the pairs are independent: only c_fc2's affine, against silu(plain a1) * a2
        a1p = linear(hip, wfmt, xd, W1d, s1, H, C)
        want2 = torch.empty(M, H, dtype=BF, device=dev)
        call(hip, "llj_g_silu_mul", a1p.data_ptr(), a2.data_ptr(), want2.data_ptr(), M * H, 0, st())
        assert_bf16_close(v2((one, zero), (sc2, bi2)).float().cpu().numpy(), want2.float().cpu().numpy(),
                          "swiglu v2, c_fc2's pair only", rel=3e-2)
    assert not torch.equal(got, he)
    # one pair without the other is refused
    h = torch.empty(M, H, dtype=BF, device=dev)
    assert hip.llj_norm_swiglu_v2(wfmt, xd.data_ptr(), None, 0.0, W1d.data_ptr(), P(s1), W2d.data_ptr(), P(s2),
                                  h.data_ptr(), M, H, C, None, 0, None, None, 0, st(), sc1.data_ptr(), bi1.data_ptr(),
                                  None, None) == 1000


def rope_kv(hip, qkv, B, T_, nh, hs, S, rope, pos):
    Cd = nh * hs
    q = torch.zeros(B * T_, Cd, dtype=BF, device=dev)
    kc = torch.zeros(B, nh, S, hs, dtype=BF, device=dev)
    vc = torch.zeros_like(kc)
    # the borrowed oracle is itself checked against numpy: tests/test_generic_kernels_gpu.py::test_rope_kv_*
    call(hip, "llj_g_rope_kv", qkv.data_ptr(), q.data_ptr(), kc.data_ptr(), vc.data_ptr(), rope.data_ptr(), pos.data_ptr(),
         B, T_, Cd, nh, S, 0, st())
    return q, kc, vc


@pytest.mark.parametrize("wfmt", FMTS)
@pytest.mark.parametrize("nh", [4, 2])  # head size 64 and 128
@pytest.mark.parametrize("B,p0,sa", [(1, 3, 1), (2, 3, 1), (8, 3, 1), (8, 3, 0), (1, 37, 1), (8, 37, 1)])  # p0 = 37 >= S: ring wrap
def test_norm_qkv_rope_v2(hip, wfmt, nh, B, p0, sa):
    rng = np.random.default_rng(400 + wfmt + 7 * B + nh + p0 + sa)
    hs, S = C // nh, 32
    _, Wd, szd = quant_operands(hip, rng, wfmt, 3 * C, C)
    xd = T(bf16(rng.standard_normal((B, C))), BF)
    rope, pos = T(O.build_rope_cache(128, hs)), T(np.array([p0], np.int32))
    sc, bi = vecs(rng, 3 * C)
    one, zero = vecs(rng, 3 * C, identity=True)

    def fused(name, *tail):
        q = torch.zeros(B, C, dtype=BF, device=dev)
        kc = torch.zeros(B, nh, S, hs, dtype=BF, device=dev)
        vc = torch.zeros_like(kc)
        call(hip, name, wfmt, xd.data_ptr(), None, 0.0, Wd.data_ptr(), P(szd), q.data_ptr(), kc.data_ptr(), vc.data_ptr(),
             rope.data_ptr(), pos.data_ptr(), B, 1, C, nh, S, 0, B, None, None, None, 0, st(), *tail)
        return q, kc, vc

    with stream_a(hip, sa):
        qkv = affine(linear(hip, wfmt, xd, Wd, szd, 3 * C, C), sc, bi).contiguous()
        want = rope_kv(hip, qkv, B, 1, nh, hs, S, rope, pos)
        got = fused("llj_norm_qkv_rope_v2", sc.data_ptr(), bi.data_ptr())
        base = fused("llj_norm_qkv_rope")
        ident = fused("llj_norm_qkv_rope_v2", one.data_ptr(), zero.data_ptr())
        null = fused("llj_norm_qkv_rope_v2", None, None)
    for name, a, b, c, d, e in zip(("q", "k cache", "v cache"), got, want, base, ident, null):
        if name == "v cache":  # no RoPE: bitwise
            assert torch.equal(a, b), name
        else:
            # RoPE of the same bf16 values in fp32: the fused epilogue and llj_g_rope_kv contract the two
            # products of v * cos -+ partner * sin differently, so a result on a bf16 rounding boundary can
            # differ by an ulp (as the plain llj_norm_qkv_rope does from that composition today):
            # the bound of tests/test_kernels_gpu.py::test_fused_qkv_rope_kv
            assert_bf16_close(a.float().cpu().numpy(), b.float().cpu().numpy(), name)
        assert torch.equal(c, d) and torch.equal(c, e), name
        assert not torch.equal(a, c), name
    assert got[1][:, :, p0 % S].abs().sum() > 0 and got[1].abs().sum() == got[1][:, :, p0 % S].abs().sum()


@pytest.mark.parametrize("wfmt", FMTS)
@pytest.mark.parametrize("M", [2, 8])
def test_identity_with_fused_norm_and_handoff(hip, wfmt, M):
    """The norm-fused forms (RMSNorm from the producer's handed-over statistics, M = 1: from x) with an
    identity affine are bitwise the existing entry points; with a real affine they equal the affine
    applied to the existing op's own output (llj_norm_linear)."""
    rng = np.random.default_rng(500 + wfmt + M)
    V = 80
    _, Wd, szd = quant_operands(hip, rng, wfmt, V, C)
    _, Wp, szp = quant_operands(hip, rng, wfmt, C, C)
    yd = T(bf16(rng.standard_normal((M, C))), BF)
    x = T(bf16(rng.standard_normal((M, C))), BF)
    gd = T(bf16(rng.uniform(0.5, 1.5, C)), BF)
    ns = torch.zeros(C // 16, 16, dtype=torch.float32, device=dev)
    call(hip, "llj_linear_resid", wfmt, yd.data_ptr(), C, Wp.data_ptr(), P(szp), x.data_ptr(), C, M, C, C, None, 0,
         ns.data_ptr(), st())
    sc, bi = vecs(rng, V)
    one, zero = vecs(rng, V, identity=True)
    for rows, nst in ((M, ns), (1, None)):
        base = torch.empty(rows, V, dtype=BF, device=dev)
        call(hip, "llj_norm_linear", wfmt, x.data_ptr(), gd.data_ptr(), 1e-5, Wd.data_ptr(), P(szd), base.data_ptr(), V,
             rows, V, C, None, 0, None, P(nst), C // 16, st())
        for s_, b_, ref in ((one, zero, base), (sc, bi, affine(base, sc, bi))):
            out = torch.empty(rows, V, dtype=BF, device=dev)
            call(hip, "llj_norm_linear_v2", wfmt, x.data_ptr(), gd.data_ptr(), 1e-5, Wd.data_ptr(), P(szd),
                 out.data_ptr(), V, rows, V, C, None, 0, None, P(nst), C // 16, st(), s_.data_ptr(), b_.data_ptr())
            assert torch.equal(out, ref)


def tpw_one(hip, fn):
    old = hip.llj_set_tpw_max(1)
    try:
        return fn()
    finally:
        hip.llj_set_tpw_max(old)


@pytest.mark.parametrize("wfmt", [0, 3])
@pytest.mark.parametrize("N", [16 * 261, 16 * 769])
def test_swiglu_and_resid_v2_multi_tile(hip, wfmt, N):
    """llj_norm_swiglu_v2 (both pairs' per-slot selects) and llj_linear_resid_v2 at M = 8 with more tiles
    than compute units (2 and 4 tiles per workgroup; the residual op at most 2), the last workgroup
    partial: against the compositions, and bitwise one tile per workgroup."""
    rng = np.random.default_rng(700 + N + wfmt)
    M = 8
    _, W1d, s1 = quant_operands(hip, rng, wfmt, N, K)
    _, W2d, s2 = quant_operands(hip, rng, wfmt, N, K)
    xd = T(bf16(rng.standard_normal((M, K))), BF)
    sc1, bi1 = vecs(rng, N)
    sc2, bi2 = vecs(rng, N)
    a1 = affine(linear(hip, wfmt, xd, W1d, s1, N, K), sc1, bi1).contiguous()
    a2 = affine(linear(hip, wfmt, xd, W2d, s2, N, K), sc2, bi2).contiguous()
    want = torch.empty(M, N, dtype=BF, device=dev)
    call(hip, "llj_g_silu_mul", a1.data_ptr(), a2.data_ptr(), want.data_ptr(), M * N, 0, st())

    def swiglu():
        h = torch.empty(M, N, dtype=BF, device=dev)
        call(hip, "llj_norm_swiglu_v2", wfmt, xd.data_ptr(), None, 0.0, W1d.data_ptr(), P(s1), W2d.data_ptr(), P(s2),
             h.data_ptr(), M, N, K, None, 0, None, None, 0, st(), sc1.data_ptr(), bi1.data_ptr(), sc2.data_ptr(),
             bi2.data_ptr())
        return h

    got = swiglu()
    assert_bf16_close(got.float().cpu().numpy(), want.float().cpu().numpy(), "swiglu v2 multi-tile", rel=3e-2)  # __expf
    assert torch.equal(got, tpw_one(hip, swiglu))
    # the residual op: the same weight as an (N, K) projection onto an N-wide stream
    x0 = T(bf16(rng.standard_normal((M, N))), BF)
    wantr = x0 + affine(linear(hip, wfmt, xd, W1d, s1, N, K), sc1, bi1)

    def resid():
        x, ns = x0.clone(), torch.zeros(N // 16, 16, dtype=torch.float32, device=dev)
        call(hip, "llj_linear_resid_v2", wfmt, xd.data_ptr(), K, W1d.data_ptr(), P(s1), x.data_ptr(), N, M, N, K, None, 0,
             ns.data_ptr(), st(), sc1.data_ptr(), bi1.data_ptr())
        return x, ns

    x, ns = resid()
    assert torch.equal(x, wantr)
    torch.testing.assert_close(ns, nstat_of(x, M, N), rtol=1e-5, atol=1e-6)
    x1, ns1 = tpw_one(hip, resid)
    assert torch.equal(x, x1) and torch.equal(ns, ns1)


@pytest.mark.parametrize("wfmt", [0, 3])
def test_norm_qkv_rope_v2_multi_tile(hip, wfmt):
    """The flat QKV epilogue with an affine at two tiles per workgroup: C = 1408 (11 heads of 128), 264
    tiles, M = 8 rows. (3 C / 16 tiles is a multiple of 2, 3 and 4 for every C the GEMVs take, so the
    QKV form has no partial last workgroup.)"""
    rng = np.random.default_rng(800 + wfmt)
    B, nh, hs, S, p0 = 8, 11, 128, 32, 37
    Cq = nh * hs
    _, Wd, szd = quant_operands(hip, rng, wfmt, 3 * Cq, Cq)
    xd = T(bf16(rng.standard_normal((B, Cq))), BF)
    rope, pos = T(O.build_rope_cache(128, hs)), T(np.array([p0], np.int32))
    sc, bi = vecs(rng, 3 * Cq)

    def fused():
        q = torch.zeros(B, Cq, dtype=BF, device=dev)
        kc = torch.zeros(B, nh, S, hs, dtype=BF, device=dev)
        vc = torch.zeros_like(kc)
        call(hip, "llj_norm_qkv_rope_v2", wfmt, xd.data_ptr(), None, 0.0, Wd.data_ptr(), P(szd), q.data_ptr(),
             kc.data_ptr(), vc.data_ptr(), rope.data_ptr(), pos.data_ptr(), B, 1, Cq, nh, S, 0, B, None, None, None, 0, st(),
             sc.data_ptr(), bi.data_ptr())
        return q, kc, vc

    qkv = affine(linear(hip, wfmt, xd, Wd, szd, 3 * Cq, Cq), sc, bi).contiguous()
    want = rope_kv(hip, qkv, B, 1, nh, hs, S, rope, pos)
    got = fused()
    one = tpw_one(hip, fused)
    for name, a, b, c in zip(("q", "k cache", "v cache"), got, want, one):
        assert torch.equal(a, c), name  # bitwise one tile per workgroup
        if name == "v cache":
            assert torch.equal(a, b), name
        else:  # RoPE contraction: test_fused_qkv_rope_kv's bound (see test_norm_qkv_rope_v2)
            assert_bf16_close(a.float().cpu().numpy(), b.float().cpu().numpy(), name)


def colblock_operands(rng, N, Kd, bits, group):
    """ColBlockQuantizedLinear's buffers as llj_g_linear reads them: codes column-major (byte (n, j) at
    j * N + n, low bits first), fp32 scales / zeros (N, G)."""
    epb = 8 // bits
    G = (Kd + group - 1) // group
    qw = rng.integers(0, 256, size=(Kd // epb, N), dtype=np.uint8)  # physical (K / epb, N) row-major
    scales = (rng.uniform(0.5, 1.5, size=(N, G)) * 0.02).astype(np.float32)
    zeros = rng.integers(0, 2 ** bits, size=(N, G)).astype(np.float32)
    return T(qw), T(scales), T(zeros)


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("wkind", [1, 0])
@pytest.mark.parametrize("with_resid", [False, True])
def test_g_linear_v2(hip, dt, wkind, with_resid):
    """The any-shape kernel (bf16 and fp32, dense and ColBlock) at K = 780 (the 125M config's n_embd), N = 50
    (a partial last block of 4 columns), M = 11 (two row blocks): llj_g_linear -> the torch affine in the
    activation type (fp32: evaluated as written) -> the torch residual add, bitwise; an identity pair and
    a NULL pair are bitwise llj_g_linear."""
    rng = np.random.default_rng(900 + 4 * dt + 2 * wkind + with_resid)
    M, N, Kd = 11, 50, 780
    tt = BF if dt == 0 else torch.float32
    xd = T(bf16(rng.standard_normal((M, Kd))), tt)
    if wkind == 1:
        W, scl, zr, bits, group = T(bf16(rng.standard_normal((N, Kd)) / np.sqrt(Kd)), tt), None, None, 16, Kd
    else:
        bits, group = 4, 260
        W, scl, zr = colblock_operands(rng, N, Kd, bits, group)
    r0 = T(bf16(rng.standard_normal((M, N))), tt) if with_resid else None
    sc = T(bf16(rng.uniform(0.5, 1.5, N) * rng.choice([-1.0, 1.0], N)), tt)
    bi = T(bf16(0.3 * rng.standard_normal(N)), tt)
    one, zero = torch.ones(N, dtype=tt, device=dev), torch.zeros(N, dtype=tt, device=dev)

    def run(name, resid, *tail):
        y = torch.empty(M, N, dtype=tt, device=dev)
        call(hip, name, wkind, xd.data_ptr(), Kd, M, Kd, W.data_ptr(), P(scl), P(zr), bits, group, N, y.data_ptr(), N,
             P(resid), N if resid is not None else 0, dt, st(), *tail)
        return y

    lin = run("llj_g_linear", None)
    base = run("llj_g_linear", r0)
    want = sc * (lin + bi)
    if with_resid:
        want = r0 + want
    got = run("llj_g_linear_v2", r0, sc.data_ptr(), bi.data_ptr())
    assert torch.equal(got, want)
    assert not torch.equal(got, base)
    assert torch.equal(run("llj_g_linear_v2", r0, one.data_ptr(), zero.data_ptr()), base)
    assert torch.equal(run("llj_g_linear_v2", r0, None, None), base)
    y = torch.empty(M, N, dtype=tt, device=dev)
    assert hip.llj_g_linear_v2(wkind, xd.data_ptr(), Kd, M, Kd, W.data_ptr(), P(scl), P(zr), bits, group, N, y.data_ptr(), N,
                               None, 0, dt, st(), sc.data_ptr(), None) == 1000


def test_llm_int8_has_no_affine_form(hip):
    """wfmt 2 with a (scale, bias) pair is refused (LLJ_EINVAL) before any launch."""
    M, N = 2, 80
    x = torch.zeros(M, K, dtype=BF, device=dev)
    W = torch.zeros(N, K, dtype=torch.int8, device=dev)
    scb = torch.ones(N, dtype=torch.float32, device=dev)
    out = torch.empty(M, N, dtype=BF, device=dev)
    ws = torch.zeros(hip.llj_i8_ws_bytes(M, K), dtype=torch.uint8, device=dev)
    one, zero = vecs(None, N, identity=True)
    assert hip.llj_linear_v2(2, x.data_ptr(), K, W.data_ptr(), scb.data_ptr(), None, out.data_ptr(), N, M, N, K,
                             ws.data_ptr(), 0, None, st(), one.data_ptr(), zero.data_ptr()) == 1000


# ------------------------------------------------------------------ prefill GEMMs
# register-staged and LDS-DMA kernels (llj_set_option LLJ_OPT_GEMM_GLDS), int4 with and without LLJ_WF_ZINT
GEMM_FMTS = [0, _hip.WF_ZINT, 1, 3, W4G_128]


def gemm_rows(hip, wfmt, xd, Wd, szd, N, Kd):
    """The Linear's bf16 output for many rows from the decode GEMV in 16-row slices (the GEMMs sum K
    in another order, so GEMM results are compared within the bf16 bound of
    tests/test_kernels_gpu.py::test_gemm_linear_and_resid, and bitwise against their own plain form)."""
    M = xd.shape[0]
    out = torch.empty(M, N, dtype=BF, device=dev)
    call(hip, "llj_gemm_linear", wfmt, xd.data_ptr(), Kd, Wd.data_ptr(), P(szd), out.data_ptr(), N, M, N, Kd, st())
    return out


@pytest.mark.parametrize("glds", [0, 1])
@pytest.mark.parametrize("wfmt", GEMM_FMTS)
@pytest.mark.parametrize("M", [150, 256])
def test_gemm_v2(hip, wfmt, M, glds):
    """llj_gemm_linear_v2 / _resid_v2 / _silu_mul_v2 / _qkv_rope_v2 against the plain GEMM of the same
    kernel family followed by the torch / any-shape composition (bitwise: both start from the same
    accumulators), and with an identity affine against the plain entry points."""
    rng = np.random.default_rng(600 + (wfmt & 0xFFFF) + M + glds + (wfmt >> 17))
    nh, hs, S = 4, 64, 512
    _, Wq, sq = quant_operands(hip, rng, wfmt, 3 * C, C)
    _, W1, s1 = quant_operands(hip, rng, wfmt, H, C)
    _, W2, s2 = quant_operands(hip, rng, wfmt, H, C)
    _, Wp, sp = quant_operands(hip, rng, wfmt, C, H)
    xd = T(bf16(rng.standard_normal((M, C))), BF)
    hd = T(bf16(rng.standard_normal((M, H))), BF)
    x0 = T(bf16(rng.standard_normal((M, C))), BF)
    rope, pos = T(O.build_rope_cache(512, hs)), T(np.arange(5, 5 + M, dtype=np.int32))
    with option(hip, _hip.OPT_GEMM_GLDS, glds):
        # ---- store
        sc, bi = vecs(rng, H)
        one, zero = vecs(rng, H, identity=True)
        a1p = gemm_rows(hip, wfmt, xd, W1, s1, H, C)
        for s_, b_, ref in ((sc, bi, affine(a1p, sc, bi)), (one, zero, a1p), (None, None, a1p)):
            out = torch.empty(M, H, dtype=BF, device=dev)
            call(hip, "llj_gemm_linear_v2", wfmt, xd.data_ptr(), C, W1.data_ptr(), P(s1), out.data_ptr(), H, M, H, C,
                 st(), P(s_), P(b_))
            assert torch.equal(out, ref), "store"
        a1 = affine(a1p, sc, bi).contiguous()
        # ---- silu * mul on h holding c_fc1's (affine) output; the pair is c_fc2's
        sc2, bi2 = vecs(rng, H)
        a2 = affine(gemm_rows(hip, wfmt, xd, W2, s2, H, C), sc2, bi2).contiguous()
        want = torch.empty(M, H, dtype=BF, device=dev)
        call(hip, "llj_g_silu_mul", a1.data_ptr(), a2.data_ptr(), want.data_ptr(), M * H, 0, st())
        h = a1.clone()
        call(hip, "llj_gemm_silu_mul_v2", wfmt, xd.data_ptr(), C, W2.data_ptr(), P(s2), h.data_ptr(), H, M, H, C, st(),
             sc2.data_ptr(), bi2.data_ptr())
        assert_bf16_close(h.float().cpu().numpy(), want.float().cpu().numpy(), "silu_mul v2", rel=3e-2)  # __expf
        hb, hi = a1.clone(), a1.clone()
        call(hip, "llj_gemm_silu_mul", wfmt, xd.data_ptr(), C, W2.data_ptr(), P(s2), hb.data_ptr(), H, M, H, C, st())
        call(hip, "llj_gemm_silu_mul_v2", wfmt, xd.data_ptr(), C, W2.data_ptr(), P(s2), hi.data_ptr(), H, M, H, C, st(),
             one.data_ptr(), zero.data_ptr())
        assert torch.equal(hb, hi), "silu_mul identity"
        # ---- residual
        scp, bip = vecs(rng, C)
        onec, zeroc = vecs(rng, C, identity=True)
        lin = gemm_rows(hip, wfmt, hd, Wp, sp, C, H)
        xe = x0.clone()
        call(hip, "llj_gemm_resid", wfmt, hd.data_ptr(), H, Wp.data_ptr(), P(sp), xe.data_ptr(), C, M, C, H, st())
        for s_, b_, ref in ((scp, bip, x0 + affine(lin, scp, bip)), (onec, zeroc, xe), (None, None, xe)):
            x = x0.clone()
            call(hip, "llj_gemm_resid_v2", wfmt, hd.data_ptr(), H, Wp.data_ptr(), P(sp), x.data_ptr(), C, M, C, H, st(),
                 P(s_), P(b_))
            assert torch.equal(x, ref), "resid"
        # ---- QKV + RoPE + KV write (B = 1, T = M rows at positions 5 ..)
        scq, biq = vecs(rng, 3 * C)
        oneq, zeroq = vecs(rng, 3 * C, identity=True)
        qkv = affine(gemm_rows(hip, wfmt, xd, Wq, sq, 3 * C, C), scq, biq).contiguous()
        want3 = rope_kv(hip, qkv, 1, M, nh, hs, S, rope, pos)

        def fused(name, *tail):
            q = torch.zeros(M, C, dtype=BF, device=dev)
            kc = torch.zeros(1, nh, S, hs, dtype=BF, device=dev)
            vc = torch.zeros_like(kc)
            call(hip, name, wfmt, xd.data_ptr(), Wq.data_ptr(), P(sq), q.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                 rope.data_ptr(), pos.data_ptr(), 1, M, C, nh, S, st(), *tail)
            return q, kc, vc

        got3 = fused("llj_gemm_qkv_rope_v2", scq.data_ptr(), biq.data_ptr())
        base3 = fused("llj_gemm_qkv_rope")
        ident3 = fused("llj_gemm_qkv_rope_v2", oneq.data_ptr(), zeroq.data_ptr())
        for name, a, b, c, d in zip(("q", "k cache", "v cache"), got3, want3, base3, ident3):
            # the LDS-staged QKV epilogue forms RoPE from two products, llj_g_rope_kv may contract them:
            # test_gemm_qkv_rope_kv's bound
            assert_bf16_close(a.float().cpu().numpy(), b.float().cpu().numpy(), "gemm qkv v2 " + name)
            assert torch.equal(c, d), name
            assert not torch.equal(a, c), name
