"""llj_attention_ragged (csrc/attention_ragged.hip) against a numpy float64 oracle written here (GPU): RoPE on q and
k at each row's own position p_b = *pos - off[b], k / v into slot p_b of row b's cache, attention of row b over its
keys 0 .. p_b.

Every case gives the positions as one `pos` and an `off` vector with off = 0 for the row at the highest position.
The caches start from random bf16 values in the slots below p_b and NaN from slot p_b on, in every row, so a read
above p_b (or a missing write of slot p_b) shows as a non-finite output, and any write outside slot p_b as a changed
bit. The y and q_out buffers carry two extra rows of a sentinel.

  LONG   S = 320, 13 rows at {0, 1, 15, 16, 63, 64, 127, 128, 129, 255, 256, 300, 319}: the single-key row, the wave
         and pass boundaries of a 128-keys-per-pass block and the last slot (both head sizes)
  DEEP   S = 2048, 8 rows at {0, 1023, 2047, ...}
  others B = 1, 5, 8 at small S
"""
import functools

import numpy as np
import pytest
import torch

from oracle import llama_np as O
from tests import helpers as H

pytestmark = pytest.mark.gpu

LONG_P = (0, 1, 15, 16, 63, 64, 127, 128, 129, 255, 256, 300, 319)
# name: (head_size, n_head, S, positions)
CASES = {
    "long64": (64, 3, 320, LONG_P),
    "long128": (128, 2, 320, LONG_P),
    "deep128": (128, 4, 2048, (0, 1023, 2047, 1, 512, 1024, 2046, 100)),
    "one64": (64, 2, 40, (7,)),
    "five64": (64, 4, 64, (63, 0, 31, 32, 5)),
    "eight128": (128, 3, 130, (129, 128, 127, 2, 64, 65, 0, 16)),
}
EXTRA = 2  # rows of y / q_out past B


def bits(a):
    return O.to_bf16_bits(np.asarray(a, np.float32))


def dev_bf16(b):
    """uint16 bf16 bit patterns -> a bf16 device tensor of the same shape"""
    return torch.tensor(np.ascontiguousarray(b).view(np.int16)).cuda().view(torch.bfloat16)


def host_bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


@functools.lru_cache(maxsize=None)
def make_case(name, exact=False):
    """Inputs (bf16 bit patterns / fp32 / int32 numpy arrays) of one case; left unchanged."""
    hs, nh, S, ps = CASES[name]
    B, C = len(ps), nh * hs
    rng = np.random.default_rng([91, hs, nh, S, B, int(exact)])
    p = np.asarray(ps, np.int32)
    pos = np.asarray([p.max()], np.int32)
    off = (pos[0] - p).astype(np.int32)
    assert (off == 0).any() and (off >= 0).all()
    if exact:
        qkv = rng.integers(-4, 5, size=(B, 3 * C)).astype(np.float32)
        rope = H.dyadic_rope(rng, S, hs)
    else:
        from lit_llama.model import build_rope_cache

        qkv = H.bf16(rng.standard_normal((B, 3 * C)).astype(np.float32))
        rope = build_rope_cache(S + 5 if S < 2048 else S, hs, torch.float32, torch.device("cpu")).numpy()
    assert rope.dtype == np.float32 and rope.shape[1:] == (hs // 2, 2) and rope.shape[0] >= S
    caches = []
    for _ in range(2):
        c = bits(rng.standard_normal((B, nh, S, hs)).astype(np.float32))
        for b in range(B):
            c[b, :, p[b]:] = 0x7FC0  # NaN from slot p_b on
        caches.append(c)
    out = dict(hs=hs, nh=nh, S=S, B=B, C=C, p=p, pos=pos, off=off, qkv=bits(qkv), rope=np.ascontiguousarray(rope),
               kc=caches[0], vc=caches[1])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def launch(hip, c, perm=None):
    """One launch on fresh device buffers; rows (and off) taken in the order `perm`. Returns the bit patterns of
    (y, q_out, kcache, vcache) after it."""
    from tests.test_kernels_gpu import call, st

    B, C = c["B"], c["C"]
    perm = np.arange(B) if perm is None else np.asarray(perm)
    qkv, kc, vc = dev_bf16(c["qkv"][perm]), dev_bf16(c["kc"][perm]), dev_bf16(c["vc"][perm])
    y = dev_bf16(np.full((B + EXTRA, C), H.SENTINEL, np.uint16))
    q = dev_bf16(np.full((B + EXTRA, C), H.SENTINEL, np.uint16))
    rope = torch.tensor(c["rope"]).cuda()
    pos, off = torch.tensor(c["pos"]).cuda(), torch.tensor(c["off"][perm]).cuda()
    call(hip, "llj_attention_ragged", qkv.data_ptr(), q.data_ptr(), kc.data_ptr(), vc.data_ptr(), y.data_ptr(),
         rope.data_ptr(), pos.data_ptr(), off.data_ptr(), B, c["nh"], c["hs"], c["S"], rope.shape[0], st())
    torch.cuda.synchronize()
    return host_bits(y), host_bits(q), host_bits(kc), host_bits(vc)


@functools.lru_cache(maxsize=None)
def result(name, exact=False):
    from lit_llama import _hip

    out = launch(_hip.lib(), make_case(name, exact))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle(name, exact=False):
    """float64: (q', k', v of slot p_b as float32 holding bf16 values, each (B, nh, hs); y (B, C) float64)."""
    c = make_case(name, exact)
    B, nh, hs, p = c["B"], c["nh"], c["hs"], c["p"]
    qkv = O.from_bf16_bits(c["qkv"]).reshape(B, 3, nh, hs)
    cs = c["rope"][p][:, None]  # (B, 1, hs / 2, 2)
    q1, k1, v1 = H.rope_bf16(qkv[:, 0], cs, exact=exact), H.rope_bf16(qkv[:, 1], cs, exact=exact), qkv[:, 2]
    kc, vc = O.from_bf16_bits(c["kc"]).astype(np.float64), O.from_bf16_bits(c["vc"]).astype(np.float64)
    y = np.zeros((B, nh, hs))
    for b in range(B):
        for h in range(nh):
            K = np.concatenate([kc[b, h, :p[b]], k1[b, h][None].astype(np.float64)])
            V = np.concatenate([vc[b, h, :p[b]], v1[b, h][None].astype(np.float64)])
            s = K @ q1[b, h].astype(np.float64) / np.sqrt(hs)
            w = np.exp(s - s.max())
            y[b, h] = (w / w.sum()) @ V
    assert np.isfinite(y).all()
    return q1, k1, v1, y.reshape(B, -1)


def written_slot(c, cache_bits):
    """slot p_b of every (row, head): (B, nh, hs) bit patterns"""
    return np.stack([cache_bits[b, :, c["p"][b]] for b in range(c["B"])])


@pytest.mark.parametrize("name", list(CASES))
def test_output_matches_the_oracle(hip, name):
    c = make_case(name)
    yb, qb, kb, vb = result(name)
    q1, k1, v1, y = oracle(name)
    B = c["B"]
    got = O.from_bf16_bits(yb[:B])
    assert np.isfinite(got).all(), f"{name}: a slot above a row's position was read, or slot p was not written"
    H.assert_bf16_close(got, y, f"{name} y")
    H.assert_bf16_close(O.from_bf16_bits(qb[:B]), q1.reshape(B, -1), f"{name} q_out")
    H.assert_bf16_close(O.from_bf16_bits(written_slot(c, kb)), k1, f"{name} k slot")
    np.testing.assert_array_equal(written_slot(c, vb), bits(v1))


@pytest.mark.parametrize("name", ["long64", "long128", "five64"])
def test_rope_and_write_are_exact(hip, name):
    """Small-integer qkv and a dyadic RoPE table: fp32 products and sums are exact, so q_out and slot p_b of both
    caches have one correct bit pattern."""
    c = make_case(name, True)
    yb, qb, kb, vb = result(name, True)
    q1, k1, v1, y = oracle(name, True)
    B = c["B"]
    np.testing.assert_array_equal(qb[:B], bits(q1).reshape(B, -1))
    np.testing.assert_array_equal(written_slot(c, kb), bits(k1))
    np.testing.assert_array_equal(written_slot(c, vb), bits(v1))
    H.assert_bf16_close(O.from_bf16_bits(yb[:B]), y, f"{name} y (exact inputs)")


@pytest.mark.parametrize("name", list(CASES))
def test_nothing_outside_slot_p_is_touched(hip, name):
    c = make_case(name)
    yb, qb, kb, vb = result(name)
    B = c["B"]
    for got, pre, what in ((kb, c["kc"], "kcache"), (vb, c["vc"], "vcache")):
        changed = got != pre
        for b in range(B):
            others = np.delete(changed[b], c["p"][b], axis=1)
            assert not others.any(), f"{name} {what} row {b}: a slot other than {c['p'][b]} changed"
            assert changed[b, :, c["p"][b]].all(), f"{name} {what} row {b}: slot {c['p'][b]} (NaN before) not written"
    assert (yb[B:] == H.SENTINEL).all() and (qb[B:] == H.SENTINEL).all()
    assert (yb[:B] != H.SENTINEL).all() and (qb[:B] != H.SENTINEL).all()


@pytest.mark.parametrize("name", ["long64", "eight128"])
def test_rows_permute_bitwise(hip, name):
    """A row's result depends on its own row (and its own off) alone."""
    c = make_case(name)
    perm = np.random.default_rng(5).permutation(c["B"])
    assert (perm != np.arange(c["B"])).any()
    base, got = result(name), launch(hip, c, perm)
    B = c["B"]
    for a, b in zip(base, got):
        np.testing.assert_array_equal(b[:B], a[:B][perm])


@pytest.mark.parametrize("name", ["long128", "deep128"])
def test_two_launches_give_the_same_bits(hip, name):
    c = make_case(name)
    for a, b in zip(result(name), launch(hip, c)):
        np.testing.assert_array_equal(a, b)
