"""The two launches of the packed prefill on their own (GPU): llj_rope_kv_packed and llj_attention_prefill_packed
(include/lit_llama_amd_packed.h), called through lit_llama._hip.call on hand-built packed rows.

Shapes: n_head 3, head size 64 and 128, lengths LENGTHS in caches of S = 256 slots -- one token, lengths around
the 16-query wave block and around one and two 64-query / 64-key tiles, a sequence of four tiles -- and one
sequence of 320 tokens (five tiles, S = 320: the cache is full).

RoPE + KV write: small-integer qkv and a dyadic RoPE table make every fp32 intermediate exact, so the oracle
(tests.helpers.rope_bf16) is compared with tolerance zero (as values: a zero's sign is not pinned); sentinel-filled
buffers show what was written.
Attention: a float64 numpy oracle at assert_bf16_close's defaults; bit equality with llj_attention_prefill called per
sequence on the same q rows and cache row; NaN in every slot >= T_b; order and repetition of the work list.
"""
import numpy as np
import pytest
import torch

import tests.helpers as H
from tests.test_packed_abi_host import ATT_BAD, ROPE_BAD

pytestmark = pytest.mark.gpu

NH = 3
LENGTHS = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200]
CASES = [(hs, tuple(L), S) for hs in (64, 128) for L, S in ((LENGTHS, 256), ([320], 320))]
IDS = [f"hs{hs}-{'x'.join(map(str, L)) if len(L) == 1 else f'B{len(L)}'}-S{S}" for hs, L, S in CASES]
EXTRA = 4  # rows allocated past M, which no launch may touch
SENT = H.SENTINEL


def _dev(a, dtype=torch.int32):
    return torch.tensor(a, dtype=dtype).cuda()


def _sentinel(*shape):
    return torch.full(shape, SENT, dtype=torch.int16).cuda().view(torch.bfloat16)


def _is_sentinel(t):
    return t.view(torch.int16) == SENT


def layout(lengths):
    from lit_llama.engine import packed_layout

    cu, tiles = packed_layout(lengths)
    return cu, tiles, _dev(cu), _dev(tiles).reshape(-1, 2).contiguous()


def rope_call(qkv, q_out, kc, vc, rope, cu_d, B, M, hs, S):
    from lit_llama import _hip

    _hip.call("llj_rope_kv_packed", qkv.data_ptr(), q_out.data_ptr(), kc.data_ptr(), vc.data_ptr(), rope.data_ptr(),
              cu_d.data_ptr(), B, M, NH, hs, S, rope.shape[0], _hip.stream())


def att_call(q, kc, vc, y, cu_d, tiles_d, B, M, hs, S):
    from lit_llama import _hip

    _hip.call("llj_attention_prefill_packed", q.data_ptr(), kc.data_ptr(), vc.data_ptr(), y.data_ptr(), cu_d.data_ptr(),
              tiles_d.data_ptr(), tiles_d.shape[0], B, M, NH, hs, S, _hip.stream())


# ------------------------------------------------------------------ llj_rope_kv_packed
@pytest.mark.parametrize("hs,lengths,S", CASES, ids=IDS)
def test_rope_kv_packed_is_the_oracle_and_writes_only_its_slots(hs, lengths, S):
    C, B = NH * hs, len(lengths)
    cu, _, cu_d, _ = layout(lengths)
    M = cu[-1]
    rng = np.random.default_rng([5, hs, M])
    y = rng.integers(-4, 5, size=(M, 3 * C)).astype(np.float32)  # c_attn's stored output: small integers
    rope = H.dyadic_rope(rng, S + 3, hs)  # (rope_rows > S: the table is indexed by position, not by S)
    qkv = torch.from_numpy(y).cuda().to(torch.bfloat16)
    q_out, kc, vc = _sentinel(M + EXTRA, C), _sentinel(B, NH, S, hs), _sentinel(B, NH, S, hs)
    rope_call(qkv, q_out, kc, vc, torch.from_numpy(rope).cuda(), cu_d, B, M, hs, S)
    torch.cuda.synchronize()
    # the oracle: row m = cu[b] + t rotated at position t
    seq = np.repeat(np.arange(B), lengths)
    tpos = np.arange(M) - np.asarray(cu)[seq]
    cs = rope[tpos][:, None]  # (M, 1, hs / 2, 2)
    q, k, v = (y[:, i * C:(i + 1) * C].reshape(M, NH, hs) for i in range(3))
    qe, ke = H.rope_bf16(q, cs), H.rope_bf16(k, cs)
    np.testing.assert_array_equal(q_out[:M].float().cpu().numpy(), qe.reshape(M, C))
    assert _is_sentinel(q_out[M:]).all(), "q_out rows past M were written"
    kce = np.full((B, NH, S, hs), np.nan, np.float32)
    vce = np.full((B, NH, S, hs), np.nan, np.float32)
    kce[seq, :, tpos] = ke
    vce[seq, :, tpos] = v
    for got, want, what in ((kc, kce, "kcache"), (vc, vce, "vcache")):
        untouched = _is_sentinel(got).all(dim=-1).cpu().numpy()  # (B, NH, S): the slot still holds the sentinel
        want_untouched = np.isnan(want).all(-1)
        np.testing.assert_array_equal(untouched, want_untouched, err_msg=f"{what}: slots written != [0, T_b)")
        for b, t in enumerate(lengths):
            assert not untouched[b, :, :t].any() and untouched[b, :, t:].all(), (what, b)
        g = got.float().cpu().numpy()
        np.testing.assert_array_equal(g[~want_untouched], want[~want_untouched], err_msg=what)


# ------------------------------------------------------------------ llj_attention_prefill_packed
_cases = {}


def att_case(hs, lengths, S):
    """q (M + EXTRA, C), caches with random keys / values in slots [0, T_b) and zeros above, the launch's y (M + EXTRA
    rows, sentinel past M); built once per shape and left unchanged."""
    key = (hs, lengths, S)
    if key not in _cases:
        C, B = NH * hs, len(lengths)
        cu, tiles, cu_d, tiles_d = layout(lengths)
        M = cu[-1]
        g = torch.Generator().manual_seed(1000 + hs + M)
        q = torch.randn(M + EXTRA, C, generator=g).to(torch.bfloat16).cuda()
        kc = torch.randn(B, NH, S, hs, generator=g).to(torch.bfloat16).cuda()
        vc = torch.randn(B, NH, S, hs, generator=g).to(torch.bfloat16).cuda()
        for b, t in enumerate(lengths):
            kc[b, :, t:] = 0
            vc[b, :, t:] = 0
        y = _sentinel(M + EXTRA, C)
        att_call(q, kc, vc, y, cu_d, tiles_d, B, M, hs, S)
        torch.cuda.synchronize()
        _cases[key] = dict(C=C, B=B, M=M, cu=cu, tiles=tiles, cu_d=cu_d, tiles_d=tiles_d, q=q, kc=kc, vc=vc, y=y)
    return _cases[key]


def bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("hs,lengths,S", CASES, ids=IDS)
def test_attention_against_float64(hs, lengths, S):
    c = att_case(hs, lengths, S)
    q, kc, vc = (c[n].float().cpu().numpy().astype(np.float64) for n in ("q", "kc", "vc"))
    got = c["y"].float().cpu().numpy()
    assert np.isfinite(got[:c["M"]]).all()
    for b, t in enumerate(lengths):
        r0 = c["cu"][b]
        qb = q[r0:r0 + t].reshape(t, NH, hs).transpose(1, 0, 2)  # (NH, t, hs)
        s = qb @ kc[b, :, :t].transpose(0, 2, 1) / np.sqrt(hs)
        s = np.where(np.tril(np.ones((t, t), bool))[None], s, -np.inf)
        p = np.exp(s - s.max(-1, keepdims=True))
        ref = (p / p.sum(-1, keepdims=True)) @ vc[b, :, :t]  # (NH, t, hs)
        H.assert_bf16_close(got[r0:r0 + t].reshape(t, NH, hs).transpose(1, 0, 2), ref, f"sequence {b} (T = {t})")
    assert _is_sentinel(c["y"][c["M"]:]).all(), "y rows past M were written"


@pytest.mark.parametrize("hs,lengths,S", CASES, ids=IDS)
def test_attention_is_bitwise_the_per_sequence_prefill(hs, lengths, S):
    """llj_attention_prefill(B = 1, T = T_b, pos = arange(T_b)) on sequence b's q rows and cache row."""
    from lit_llama import _hip

    c = att_case(hs, lengths, S)
    for b, t in enumerate(lengths):
        r0 = c["cu"][b]
        qb = c["q"][r0:r0 + t].contiguous()
        yb = _sentinel(t, c["C"])
        pos = torch.arange(t, dtype=torch.int32).cuda()
        _hip.call("llj_attention_prefill", qb.data_ptr(), c["kc"][b].data_ptr(), c["vc"][b].data_ptr(), yb.data_ptr(),
                  pos.data_ptr(), 1, t, NH, hs, S, _hip.stream())
        torch.cuda.synchronize()
        assert torch.equal(bits(c["y"][r0:r0 + t]), bits(yb)), (b, t)


@pytest.mark.parametrize("hs,lengths,S", CASES[:3:2], ids=IDS[:3:2])
def test_attention_reads_no_slot_past_its_sequence(hs, lengths, S):
    """NaN in every slot >= T_b of both caches: the output is finite and unchanged bit for bit."""
    c = att_case(hs, lengths, S)
    kc, vc = c["kc"].clone(), c["vc"].clone()
    for b, t in enumerate(lengths):
        kc[b, :, t:] = float("nan")
        vc[b, :, t:] = float("nan")
    y = _sentinel(c["M"] + EXTRA, c["C"])
    att_call(c["q"], kc, vc, y, c["cu_d"], c["tiles_d"], c["B"], c["M"], hs, S)
    torch.cuda.synchronize()
    assert torch.isfinite(y[:c["M"]].float()).all()
    assert torch.equal(bits(y), bits(c["y"]))


@pytest.mark.parametrize("hs,lengths,S", CASES[:3:2], ids=IDS[:3:2])
def test_attention_order_and_repetition(hs, lengths, S):
    """A reversed work list and a second launch give the same bits; permuting the sequences (packing, caches, cu and
    tiles rebuilt) permutes the outputs."""
    c = att_case(hs, lengths, S)
    B, M = c["B"], c["M"]
    for tiles_d in (c["tiles_d"].flip(0).contiguous(), c["tiles_d"]):
        y = _sentinel(M + EXTRA, c["C"])
        att_call(c["q"], c["kc"], c["vc"], y, c["cu_d"], tiles_d, B, M, hs, S)
        torch.cuda.synchronize()
        assert torch.equal(bits(y), bits(c["y"]))
    perm = list(np.random.default_rng(3).permutation(B))
    plen = [lengths[i] for i in perm]
    pcu, _, pcu_d, ptiles_d = layout(plen)
    q = torch.cat([c["q"][c["cu"][i]:c["cu"][i] + lengths[i]] for i in perm] + [c["q"][M:]])
    idx = torch.tensor(perm).cuda()
    kc, vc = c["kc"][idx].contiguous(), c["vc"][idx].contiguous()
    y = _sentinel(M + EXTRA, c["C"])
    att_call(q, kc, vc, y, pcu_d, ptiles_d, B, M, hs, S)
    torch.cuda.synchronize()
    for j, i in enumerate(perm):
        assert torch.equal(bits(y[pcu[j]:pcu[j] + plen[j]]), bits(c["y"][c["cu"][i]:c["cu"][i] + lengths[i]])), (j, i)


def test_bad_arguments_launch_nothing():
    """Every LLJ_EINVAL case of the header on real buffers: 1000 comes back and every output buffer still holds its
    sentinel. (The good argument lists of tests/test_packed_abi_host.py: B 8, M 40, n_head 2, head 128, S 64.)"""
    from lit_llama import _hip

    L = _hip.lib()
    B, M, nh, hs, S = 8, 40, 2, 128, 64
    cu_d = _dev([5 * b for b in range(B + 1)])
    tiles_d = _dev([(b, 0) for b in range(B)]).contiguous()
    qkv, q = _sentinel(M, 3 * nh * hs), _sentinel(M, nh * hs)
    kc, vc, y = _sentinel(B, nh, S, hs), _sentinel(B, nh, S, hs), _sentinel(M, nh * hs)
    rope = torch.zeros(128, hs // 2, 2).cuda()
    rope_good = [qkv.data_ptr(), q.data_ptr(), kc.data_ptr(), vc.data_ptr(), rope.data_ptr(), cu_d.data_ptr(), B, M, nh,
                 hs, S, 128, _hip.stream()]
    att_good = [q.data_ptr(), kc.data_ptr(), vc.data_ptr(), y.data_ptr(), cu_d.data_ptr(), tiles_d.data_ptr(), B, B, M,
                nh, hs, S, _hip.stream()]
    for name, good, bad in (("llj_rope_kv_packed", rope_good, ROPE_BAD), ("llj_attention_prefill_packed", att_good, ATT_BAD)):
        for i, v in bad:
            a = list(good)
            a[i] = v
            assert getattr(L, name)(*a) == 1000, (name, i, v)
    torch.cuda.synchronize()
    for t in (q, kc, vc, y):
        assert _is_sentinel(t).all()
