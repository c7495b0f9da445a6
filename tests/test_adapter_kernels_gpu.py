"""The LLaMA-Adapter prefix-attention kernels (csrc/adapter.hip) through the C ABI, against an fp64
numpy restatement of reference lit_llama/adapter.py:145-165 written here:

    y[m, h] = softmax_causal(q . K^T / sqrt(hs)) . V + gate[h] * softmax(q . AK^T / sqrt(hs)) . AV

Inputs are seeded normals (q scaled by 2, as tests/test_kernels_gpu.py's attention cases) with
mixed-sign gates of magnitude 0.5 .. 1.5 and one head's gate 0; the prefix term is then a large part
of the output norm, so a kernel that drops it fails. bf16 outputs: helpers.assert_bf16_close at its
defaults (one fused rounding or the reference's three bf16 roundings both sit well inside); fp32
outputs: 1e-4 relative, fp32 against fp32 as tests/test_fp32_gpu.py.
"""
import numpy as np
import pytest
import torch

from lit_llama import _hip
from tests.helpers import assert_bf16_close, bf16
from tests.test_kernels_gpu import T, call, option, st

pytestmark = pytest.mark.gpu
dev = "cuda"
EINVAL = 1000


def softmax64(s):
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def prefix_term(q, ak, av, gate, nh, hs):
    """gate[h] * softmax_j(q[m, h] . ak[h, j] / sqrt(hs)) . av[h, j] in fp64, (M, nh * hs)."""
    M = q.shape[0]
    q64 = q.astype(np.float64).reshape(M, nh, hs)
    s = np.einsum("mhd,hjd->mhj", q64, ak.astype(np.float64)) / np.sqrt(hs)
    ay = np.einsum("mhj,hjd->mhd", softmax64(s), av.astype(np.float64))
    return (gate.astype(np.float64)[None, :, None] * ay).reshape(M, nh * hs)


def causal_term(q, kc, vc, pos, S, T_, nh, hs):
    """fp64 attention over the ring cache for rows m = b * T + t at positions pos[t]."""
    M = q.shape[0]
    y = np.zeros((M, nh * hs))
    for m in range(M):
        b, t = divmod(m, T_)
        p = int(pos[t])
        slots = np.arange(p + 1) if p < S else np.arange(S)
        for h in range(nh):
            qq = q[m, h * hs:(h + 1) * hs].astype(np.float64)
            s = kc[b, h, slots].astype(np.float64) @ qq / np.sqrt(hs)
            y[m, h * hs:(h + 1) * hs] = softmax64(s) @ vc[b, h, slots].astype(np.float64)
    return y


def gates(rng, nh):
    g = rng.uniform(0.5, 1.5, nh) * np.where(np.arange(nh) % 2 == 0, 1.0, -1.0)
    g[nh - 1] = 0.0  # one head without a prefix contribution
    return bf16(g)   # the model's gate is a bf16 parameter, handed over as fp32


def prefix_inputs(rng, nh, aT, hs):
    return bf16(rng.standard_normal((nh, aT, hs))), bf16(rng.standard_normal((nh, aT, hs)))


ATT_CASES = [(1, 1, 64, 0, 10), (3, 1, 64, 5, 1), (1, 1, 64, 63, 32), (2, 1, 64, 71, 33), (2, 5, 64, 20, 10)]


@pytest.mark.parametrize("B,T_,S,p0,aT", ATT_CASES)
@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("spec_full", [0, 1])
def test_attention_adapter(hip, hs, B, T_, S, p0, aT, spec_full):
    """One valid key, the last slot, the rolled ring, the key-group boundary at 32 / 33 prefix keys
    and several rows per sequence, with half and whole speculative first passes; all gates zero is
    llj_attention bit for bit."""
    nh = 3
    rng = np.random.default_rng(1000 * hs + 10 * p0 + aT)
    C = nh * hs
    kc = bf16(rng.standard_normal((B, nh, S, hs)))
    vc = bf16(rng.standard_normal((B, nh, S, hs)))
    q = bf16(rng.standard_normal((B * T_, C)) * 2)
    ak, av = prefix_inputs(rng, nh, aT, hs)
    g = gates(rng, nh)
    pos = np.arange(p0, p0 + T_, dtype=np.int32)
    bt = torch.bfloat16
    qd, kd, vd, pd = T(q, bt), T(kc, bt), T(vc, bt), T(pos)
    akd, avd, gd, g0 = T(ak, bt), T(av, bt), T(g.astype(np.float32)), torch.zeros(nh, dtype=torch.float32, device=dev)
    y, y0, yb = (torch.empty(B * T_, C, dtype=bt, device=dev) for _ in range(3))
    with option(hip, _hip.OPT_ATT_SPEC_FULL, spec_full):
        call(hip, "llj_attention_adapter", qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), y.data_ptr(), pd.data_ptr(), B,
             T_, nh, hs, S, akd.data_ptr(), avd.data_ptr(), gd.data_ptr(), aT, st())
        call(hip, "llj_attention_adapter", qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), y0.data_ptr(), pd.data_ptr(), B,
             T_, nh, hs, S, akd.data_ptr(), avd.data_ptr(), g0.data_ptr(), aT, st())
        call(hip, "llj_attention", qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), yb.data_ptr(), pd.data_ptr(), B, T_, nh,
             hs, S, st())
    torch.cuda.synchronize()
    base = causal_term(q, kc, vc, pos, S, T_, nh, hs)
    pre = prefix_term(q, ak, av, g, nh, hs)
    share = np.linalg.norm(pre) / np.linalg.norm(base + pre)
    print(f"[adapter] prefix term is {share:.2f} of the output norm")
    assert share > 0.2  # far above the tolerance: a dropped term cannot pass
    assert_bf16_close(y.float().cpu().numpy(), base + pre, "attention + prefix")
    assert torch.equal(y0.view(torch.int16), yb.view(torch.int16)), "zero gates must be llj_attention bit for bit"


@pytest.mark.parametrize("M", [1, 37])
@pytest.mark.parametrize("hs", [64, 128, 78])
@pytest.mark.parametrize("aT", [1, 10, 33])
@pytest.mark.parametrize("dt", [0, 1])
def test_adapter_prefix_add(hip, M, hs, aT, dt):
    """y += gate * prefix attention in place: one row and more rows than two row tiles, the 16-byte
    path (hs 64 / 128) and the scalar one (hs 78, the JA 125M head), bf16 with the reference's
    rounding points and fp32; gate 0 leaves y bitwise unchanged."""
    nh = 3
    rng = np.random.default_rng(100 * hs + 7 * aT + M + dt)
    C = nh * hs
    rnd = bf16 if dt == 0 else (lambda a: np.asarray(a, np.float32))
    tt = torch.bfloat16 if dt == 0 else torch.float32
    q = rnd(rng.standard_normal((M, C)) * 2)
    y_in = rnd(rng.standard_normal((M, C)))
    ak, av = rnd(rng.standard_normal((nh, aT, hs))), rnd(rng.standard_normal((nh, aT, hs)))
    g = gates(rng, nh)
    qd, akd, avd, gd = T(q, tt), T(ak, tt), T(av, tt), T(g.astype(np.float32))
    y, y0 = T(y_in, tt), T(y_in, tt)
    g0 = torch.zeros(nh, dtype=torch.float32, device=dev)
    call(hip, "llj_adapter_prefix_add", qd.data_ptr(), akd.data_ptr(), avd.data_ptr(), gd.data_ptr(), y.data_ptr(), M,
         nh, hs, aT, dt, st())
    call(hip, "llj_adapter_prefix_add", qd.data_ptr(), akd.data_ptr(), avd.data_ptr(), g0.data_ptr(), y0.data_ptr(), M,
         nh, hs, aT, dt, st())
    torch.cuda.synchronize()
    pre = prefix_term(q, ak, av, g, nh, hs)
    want = y_in.astype(np.float64) + pre
    got = y.float().cpu().numpy()
    assert np.linalg.norm(pre) / np.linalg.norm(want) > 0.2
    if dt == 0:
        assert_bf16_close(got, want, f"prefix add hs={hs}")
    else:
        rel = np.linalg.norm(got - want) / np.linalg.norm(want)
        print(f"[adapter] fp32 prefix add rel {rel:.2e}")
        assert rel < 1e-4, rel
    ref0 = T(y_in, tt)
    assert torch.equal(y0.view(torch.int16), ref0.view(torch.int16)), "gate 0 must leave y unchanged"
    # the gate-0 head of the gated call is untouched as well
    assert torch.equal(y[:, (nh - 1) * hs:].contiguous().view(torch.int16),
                       ref0[:, (nh - 1) * hs:].contiguous().view(torch.int16))


def test_adapter_argument_checks(hip):
    """Prefix lengths outside 1 .. 64, a head size the fused kernel does not take and a missing
    prefix are refused with LLJ_EINVAL before any launch: y keeps its contents."""
    nh, hs, S, aT = 2, 64, 16, 4
    bt = torch.bfloat16
    q = torch.randn(1, nh * hs, device=dev).to(bt)
    kc = torch.randn(1, nh, S, hs, device=dev).to(bt)
    vc = torch.randn(1, nh, S, hs, device=dev).to(bt)
    ak = torch.randn(nh, 65, hs, device=dev).to(bt)
    av = torch.randn(nh, 65, hs, device=dev).to(bt)
    g = torch.ones(nh, dtype=torch.float32, device=dev)
    pos = torch.tensor([3], dtype=torch.int32, device=dev)
    y = torch.full((1, nh * hs), 7.0, device=dev).to(bt)
    keep = y.clone()

    def fused(hs_=hs, aT_=aT, ak_=ak.data_ptr()):
        return hip.llj_attention_adapter(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), y.data_ptr(), pos.data_ptr(), 1, 1,
                                         nh, hs_, S, ak_, av.data_ptr(), g.data_ptr(), aT_, st())

    def add(aT_=aT, ak_=ak.data_ptr(), dt=0):
        return hip.llj_adapter_prefix_add(q.data_ptr(), ak_, av.data_ptr(), g.data_ptr(), y.data_ptr(), 1, nh, hs, aT_,
                                          dt, st())

    assert fused(aT_=0) == EINVAL and fused(aT_=65) == EINVAL
    assert fused(hs_=96) == EINVAL  # the fused kernel serves head sizes 64 and 128
    assert fused(ak_=None) == EINVAL
    assert add(aT_=0) == EINVAL and add(aT_=65) == EINVAL
    assert add(ak_=None) == EINVAL
    assert add(dt=2) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(y, keep)
    assert fused() == 0 and add() == 0  # the same operands inside the envelope are taken
    torch.cuda.synchronize()
    assert not torch.equal(y, keep)
