"""Exact visible-set and selected-key tests of the attention kernels added after tests/test_streaming_exact_gpu.py
Part D (GPU only): llj_attention_shared (csrc/attention_shared.hip), llj_attention_ragged
(csrc/attention_ragged.hip), llj_attention_adapter (ADP in csrc/attention.h), llj_adapter_prefix_add
(csrc/adapter.hip) and llj_attention_i8 (csrc/ops.hip), with Part D's tools:

  * visible set: q = 0 and a probe V (V[s, d] = 1 iff s == off + h hs + d) make output column h hs + d of a row
    1 / nvis if the row reads slot off + h hs + d once and exactly 0 if not; every slot the kernel must not read
    holds NaN in both caches. Nonzero exactly on the visible slots, within 2^-8 of 1 / nvis, no NaN.
  * selected key: keys are +-A codes, q = A code[target], so the target's score exceeds every other visible
    slot's by >= MIN_GAP = 110 (natural units): every other weight is exactly 0 in fp32 and y = V[target] bitwise.
  * uniform softmax: q = 0 over a power-of-two number of keys gives weights exactly 1 / n, integer values give an
    exact dyadic mean, and each documented bf16 rounding point then decides the bits alone.

Every output buffer carries a sentinel row past its end that must survive. Every input condition (gaps, exact
representability in fp32 / bf16, the share in which a wrong-rounding reference differs) is asserted by the case
builders from the references alone, before a launch; tests/test_attention_variants_exact_host.py runs the same
builders without a GPU.

Cases (the same lists and builders drive both files):
  shared   S 320: P {1, 63, 64, 65, 129, 200} x p {P - 1, P, P + 62, P + 63, P + 64, 319} x nsplit {1, 3, 64}
           (P 200 / nsplit 3: 67-key ranges that begin and end inside a 64-key pass; nsplit 64: empty ranges) x B
           {1, 9} (a second row group with one live row); S 2048: P 1500, p {1499, 1500, 1563, 1564, 2047}, nsplit
           {1, 7, 32} (215-key ranges), B 12 (four live rows in the second group); both head sizes, nh 2. The
           visible set is read from y and, merged in float64 (merge_parts), from the partial records. Selected-key
           targets cycle through 0, P - 1, P, p - 1, p, the first and last key of every prefix range and
           PASS_EDGES; rows >= 1 hold NaN below P and V differs per row, so V[0, h, t] (t < P) or V[b, h, t] is
           the only right answer.
  ragged   the long64 / long128 / deep128 position lists of tests/test_ragged_attention_kernels_gpu.py. Visible
           set: the row's v is the probe's value of slot p_b, the caches hold NaN from p_b on. Selected key through
           RoPE: a quarter-turn table ((cos, sin) in (1, 0), (0, 1), (-1, 0), (0, -1)) maps +-A codes to +-A codes
           exactly; the row's q and k are the inverse rotations of A code[target] and A code[p_b], so attention
           must read back the rotated q' and the key it has just written; targets 0, p_b - 1, p_b, PASS_EDGES
           below p_b; y, q_out and both caches (slot p_b written, nothing else changed) bitwise.
  adapter  aT {1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64} x head size x LLJ_OPT_ATT_SPEC_FULL 0 / 1, grids of
           36 and 120 blocks (the spec_ok switch at 64). Two selected keys at once: cache keys live in the first
           hs / 2 dims, prefix keys in the last, V / av integers |v| <= 4, gates in {0, +-0.5, +-1, +-2}: y =
           bf16(V[t] + g av[ta]) has one bit pattern. Uniform softmax (aT 16 / 64, p + 1 16 / 128, integers up to
           127): bf16(O / L + g Oa / La), one rounding; the three-rounding result is the wrong reference. Probe av
           for every aT: columns nonzero exactly for d < aT, g / aT within 2^-8.
  prefix add   the uniform case (aT 16 / 64, M 1 / 37, head sizes 64 / 128 / 78, bf16 and fp32): bf16 bitwise
           bf16(bf16(y) + bf16(g bf16(ay))), the one-rounding result is the wrong reference; fp32 the float64
           value rounded once. Gates include 1.5, -0.75, 1.25 and -3: with a power-of-two gate bf16(g bf16(ay)) =
           bf16(g ay) and the inner rounding could not be seen. Selected prefix key over the aT list: y_in +
           g av[ta] bitwise.
  i8       Part D's selected-key inputs (S 2048, p 2047, M 8), nsplit 1 and 16: y bitwise llj_attention's /
           llj_attention_split's and V[target]; the clear block zeroed.

Measured (this file's inputs; gaps and shares from the references alone, on the CPU). Smallest selected-key gap:
shared 224 (hs 64: 224 - 288, hs 128: 430 - 498), ragged 304 / 498 / 464 (long64 / long128 / deep128), adapter
cache side 256 (hs 64) and 679 (hs 128), prefix side 384 and 815, prefix add 320 / 453 / 319 (hs 64 / 128 / 78),
attention_i8 240 / 475. Wrong-reference shares: the three-rounding result against the fused kernel's 0.25 - 0.38,
the one-rounding result against prefix add's 0.18 - 0.28, prefix add without the inner bf16(ay) 0.04 - 0.09; seed 0
everywhere. 160 cases, 6 s for the file on an MI355X (the slowest case 0.8 s); the host file 30 cases, 11 s.

Mutations of the kernels that this file catches (scratch builds, each run once on the GPU; the first test to fail):
shared, the prefix range's end min(pe, jcap) - 1 (test_shared_visible_set, P 1 p 0: no key left, NaN); shared, the
suffix from pe + 1 (test_shared_visible_set, P 1 p 1: slot 1 missing); shared, the mask `<= jend`
(test_shared_visible_set, P 1 p 63: weights off by 0.97); shared, the prefix read from the row group's own cache rows
instead of row 0's (test_shared_visible_set B 9: NaN in the second group); ragged, pl = max(p - 1, 0)
(test_ragged_visible_set: slot p_b missing in 8 rows); adapter, `li + 16 * k <= aT` in the prefix softmax
(test_adapter_two_selected_keys, aT 1: the unwritten score slot gives NaN); prefix add, round_bf(ay) removed
(test_prefix_add_rounding_points: 11 of 192 elements differ at aT 16, M 1).
"""
import functools

import numpy as np
import pytest
import torch

from lit_llama import _hip
from tests import helpers as H
from tests.helpers import bf16
from tests.test_kernels_gpu import T, call, option, st
from tests.test_ragged_attention_kernels_gpu import CASES as RAGGED_CASES
from tests.test_ragged_attention_kernels_gpu import EXTRA as RAGGED_EXTRA
from tests.test_ragged_attention_kernels_gpu import bits
from tests.test_ragged_attention_kernels_gpu import launch as ragged_launch
from tests.test_streaming_exact_gpu import (MIN_GAP, PASS_EDGES, SENT, check, check_visible, merge_parts, probe_values,
                                            rand_keys, read_rows, selected_key_case, sentinel, words)

pytestmark = pytest.mark.gpu
dev = "cuda"
f32 = np.float32
NAN = float("nan")
NAN_BITS, ONE_BITS = 0x7FC0, 0x3F80  # bf16 bit patterns
HEADS = [64, 128]
MIN_DIFFER = 0.10  # floor on the share in which a wrong-rounding reference differs from the right one
SEEDS = 16         # bound of every seed search


def codes(rng, *shape):
    return rng.choice(np.array([-1.0, 1.0], f32), size=shape)


def key_gap(keys, qv, t, hs):
    """(score of key t - the largest other score) / sqrt(hs) in float64 over the visible keys (n, d)."""
    s = keys.astype(np.float64) @ qv.astype(np.float64)
    assert s[t] == s.max()
    return np.inf if len(s) == 1 else (s[t] - np.delete(s, t).max()) / np.sqrt(hs)


def assert_bf16_values(a, what):
    a = np.asarray(a, f32)
    assert np.array_equal(bf16(a), a), f"{what}: not bf16 values"
    return a


def first_seed(build, what):
    """The first of SEEDS seeds whose case meets its conditions (build(seed) -> case or None)."""
    for seed in range(SEEDS):
        c = build(seed)
        if c is not None:
            return c
    raise AssertionError(f"{what}: none of {SEEDS} seeds meets the input conditions")


# ================================================================== 1. llj_attention_shared
SH_NH = 2
SH_GRID = [(320, B, ns) for ns in (1, 3, 64) for B in (1, 9)] + [(2048, 12, ns) for ns in (1, 7, 32)]  # (S, B, nsplit)


def sh_shapes(S):
    """(P, p) of a cache size; the kernel's contract is P - 1 <= p < S."""
    if S == 2048:
        return [(1500, p) for p in (1499, 1500, 1563, 1564, 2047)]
    return [(P, p) for P in (1, 63, 64, 65, 129, 200)
            for p in sorted({p for p in (P - 1, P, P + 62, P + 63, P + 64, S - 1) if p < S})]


def sh_ranges(P, nsplit):
    """The non-empty prefix key ranges [lo, hi) of llj_attention_shared."""
    chunk = max(-(-P // nsplit), 64)
    return [(y * chunk, min(P, (y + 1) * chunk)) for y in range(nsplit) if y * chunk < P]


def sh_dead(B, S, P, p):
    """(B, S) bool: the slots the kernel must not read (rows >= 1 below P, every row above p)."""
    s = np.arange(S)[None, :]
    return (s > p) | ((s < P) & (np.arange(B)[:, None] >= 1))


def run_shared(hip, q, kd, vd, B, P, p, hs, S, nsplit):
    """One launch -> (y (B, C) float32, partial records (B, nh, nsplit + 1, hs + 4)); y and the workspace each
    carry one more row / record, which must survive."""
    nh = SH_NH
    nrec = B * nh * (nsplit + 1)
    assert hip.llj_attention_shared_ws_bytes(B, nh, hs, nsplit) == nrec * (hs + 4) * 4
    y = sentinel(B + 1, nh * hs)
    ws = torch.full((nrec + 1, hs + 4), NAN, dtype=torch.float32, device=dev)
    pd = T(np.array([p], np.int32))
    call(hip, "llj_attention_shared", q.data_ptr(), kd.data_ptr(), vd.data_ptr(), y.data_ptr(), pd.data_ptr(), B, P, nh,
         hs, S, nsplit, ws.data_ptr(), st())
    torch.cuda.synchronize()
    part = ws.cpu().numpy()
    assert np.isnan(part[nrec]).all(), "wrote past the last partial record"
    return y, part[:nrec].reshape(B, nh, nsplit + 1, hs + 4)


@pytest.mark.parametrize("S,B,nsplit", SH_GRID)
@pytest.mark.parametrize("hs", HEADS)
def test_shared_visible_set(hip, hs, S, B, nsplit):
    """Every slot <= p is read exactly once -- the prefix from row 0, the rest from the row's own cache -- and no
    other slot at all, from y and from the partial records."""
    nh = SH_NH
    C = nh * hs
    q = torch.zeros(B, C, dtype=torch.bfloat16, device=dev)
    k0 = rand_keys(np.random.default_rng([59, hs, S]), B, nh, S, hs)
    for off in range(0, S, C):
        v0 = probe_values(B, nh, S, hs, off)
        for P, p in sh_shapes(S):
            dead = T(sh_dead(B, S, P, p))[:, None, :, None]
            y, part = run_shared(hip, q, k0.masked_fill(dead, NAN), v0.masked_fill(dead, NAN), B, P, p, hs, S, nsplit)
            what = f"shared attention hs {hs} S {S} B {B} nsplit {nsplit} P {P} p {p}"
            check_visible(read_rows(y, B), off, [p + 1] * B, what)
            assert not np.isnan(part[..., :hs + 2]).any(), f"{what}: partial records not written"
            mx = part[..., hs]
            assert ((mx == 0) | np.isneginf(mx)).all(), what
            live = len(sh_ranges(P, nsplit))
            assert (mx[:, :, :live] == 0).all() and np.isneginf(mx[:, :, live:nsplit]).all(), f"{what}: empty ranges"
            assert (np.isneginf(mx[:, :, nsplit]) == (p < P)).all(), f"{what}: the suffix record"
            check_visible(merge_parts(part, hs).astype(f32), off, [p + 1] * B, what + " (partial records)")


@functools.lru_cache(maxsize=None)
def sh_base(hs, S, B):
    rng = np.random.default_rng([61, hs, S, B])
    code = codes(rng, SH_NH, S, hs)
    V = bf16(rng.standard_normal((B, SH_NH, S, hs)).astype(f32))
    for a in (code, V):
        a.setflags(write=False)
    return code, V


def sh_selected_case(hs, S, B, P, p, nsplit):
    """selected_key_case's construction for the shared kernel: ([(q, want)] per launch, the smallest gap, the
    targets). The candidates (in a seeded order, so that every row meets prefix and suffix targets) are spread over
    as many launches as it takes for every one to be some (row, head)'s target."""
    nh = SH_NH
    code, V = sh_base(hs, S, B)
    edges = [e for lo, hi in sh_ranges(P, nsplit) for e in (lo, hi - 1)]
    cand = sorted({c for c in [0, P - 1, P, p - 1, p] + edges + PASS_EDGES if 0 <= c <= p})
    cand = [int(c) for c in np.random.default_rng([63, P, p, nsplit]).permutation(cand)]
    launches, gap, seen = [], np.inf, set()
    for r in range(-(-len(cand) // (B * nh))):
        q = np.zeros((B, nh * hs), f32)
        want = np.zeros((B, nh * hs), f32)
        for b in range(B):
            for h in range(nh):
                t = cand[(r * B * nh + b * nh + h) % len(cand)]
                seen.add(t)
                q[b, h * hs:(h + 1) * hs] = 8 * code[h, t]
                want[b, h * hs:(h + 1) * hs] = V[0 if t < P else b, h, t]
                gap = min(gap, key_gap(8 * code[h, :p + 1], q[b, h * hs:(h + 1) * hs], t, hs))
        launches.append((q, want))
    assert seen == set(cand)
    assert gap >= MIN_GAP, gap
    return launches, gap, cand


@pytest.mark.parametrize("S,B,nsplit", SH_GRID)
@pytest.mark.parametrize("hs", HEADS)
def test_shared_selected_key(hip, hs, S, B, nsplit):
    """y[b, h] = V[0, h, t] (t < P) or V[b, h, t] bitwise, with the targets on every key-range and pass boundary."""
    nh = SH_NH
    code, V = sh_base(hs, S, B)
    k0 = T(np.broadcast_to(8 * code[None], (B, nh, S, hs)), torch.bfloat16)
    v0 = T(V, torch.bfloat16)
    gap = np.inf
    for P, p in sh_shapes(S):
        dead = T(sh_dead(B, S, P, p))[:, None, :, None]
        kd, vd = k0.masked_fill(dead, NAN), v0.masked_fill(dead, NAN)
        launches, g, _ = sh_selected_case(hs, S, B, P, p, nsplit)
        gap = min(gap, g)
        for i, (q, want) in enumerate(launches):
            y, _ = run_shared(hip, T(q, torch.bfloat16), kd, vd, B, P, p, hs, S, nsplit)
            check(y, want, f"shared attention selected key hs {hs} S {S} B {B} nsplit {nsplit} P {P} p {p} launch {i}")
    print(f"shared attention hs {hs} S {S} B {B} nsplit {nsplit}: selected-key gap {gap:.0f}")


# ================================================================== 2. llj_attention_ragged
RG_NAMES = ["long64", "long128", "deep128"]


def rg_shape(name):
    hs, nh, S, ps = RAGGED_CASES[name]
    p = np.asarray(ps, np.int32)
    pos = np.asarray([p.max()], np.int32)
    return hs, nh, S, p, pos, (pos[0] - p).astype(np.int32)


def rg_dict(name, qkv_bits, kc_bits, vc_bits, rope):
    """The case dictionary tests/test_ragged_attention_kernels_gpu.py's launch() takes."""
    hs, nh, S, p, pos, off = rg_shape(name)
    return dict(hs=hs, nh=nh, S=S, B=len(p), C=nh * hs, p=p, pos=pos, off=off, qkv=qkv_bits,
                rope=np.ascontiguousarray(rope, f32), kc=kc_bits, vc=vc_bits)


def quarter_rope(rng, n_pos, hs):
    """A RoPE table (n_pos, hs / 2, 2) of quarter turns: (cos, sin) in (1, 0), (0, 1), (-1, 0), (0, -1)."""
    k = rng.integers(0, 4, size=(n_pos, hs // 2))
    return np.stack([np.array([1, 0, -1, 0], f32)[k], np.array([0, 1, 0, -1], f32)[k]], -1)


def unrotate(v, cs):
    """The bf16 vector that H.rope_bf16 (the kernel's RoPE) maps to v: the rotation by the opposite angle."""
    back = H.rope_bf16(v, cs * np.array([1, -1], f32))
    assert np.array_equal(H.rope_bf16(back, cs), v)
    return back


def rg_launch(hip, c):
    """(y, q_out) float32 (B, C) and the caches' bit patterns after one launch; the rows past B keep the sentinel."""
    B = c["B"]
    yb, qb, kb, vb = ragged_launch(hip, c)
    assert yb.shape[0] == B + RAGGED_EXTRA and (yb[B:] == SENT).all() and (qb[B:] == SENT).all(), "wrote past row B"
    return yb[:B], qb[:B], kb, vb


def rg_visible_case(name, off):
    hs, nh, S, p, pos, _ = rg_shape(name)
    B, C = len(p), nh * hs
    rng = np.random.default_rng([71, hs, S, off])
    probe = np.zeros((nh, S, hs), np.uint16)
    c = np.arange(C)
    c = c[off + c < S]
    probe[c // hs, off + c, c % hs] = ONE_BITS
    kc = bits(rng.standard_normal((B, nh, S, hs)).astype(f32))
    vc = np.broadcast_to(probe, (B, nh, S, hs)).copy()
    qkv = np.zeros((B, 3, C), np.uint16)
    qkv[:, 1] = bits(rng.standard_normal((B, C)).astype(f32))
    for b in range(B):
        qkv[b, 2] = probe[:, p[b]].reshape(C)
        kc[b, :, p[b]:] = NAN_BITS
        vc[b, :, p[b]:] = NAN_BITS
    return rg_dict(name, qkv.reshape(B, 3 * C), kc, vc, quarter_rope(rng, S, hs))


@pytest.mark.parametrize("name", RG_NAMES)
def test_ragged_visible_set(hip, name):
    """Row b reads the slots below p_b and the slot it has just written, each once, and nothing from p_b + 1 on."""
    hs, nh, S, p, _, _ = rg_shape(name)
    for off in range(0, S, nh * hs):
        yb, _, _, _ = rg_launch(hip, rg_visible_case(name, off))
        check_visible(H.f32_of_bits(yb), off, p + 1, f"ragged attention {name}")


@functools.lru_cache(maxsize=None)
def rg_selected_case(name):
    """Per launch r: the case dictionary and the expected (y, q_out, k slot, v slot) as float32 (B, nh, hs); the
    smallest gap. Cache keys hold 8 code[s] below p_b (NaN from p_b on), the row's q / k are the inverse rotations
    at p_b of 8 code[target] / 8 code[p_b]; row b's targets cycle over its candidates with the launch."""
    hs, nh, S, p, pos, _ = rg_shape(name)
    B, C = len(p), nh * hs
    rng = np.random.default_rng([73, hs, S])
    code = codes(rng, nh, S, hs)
    rope = quarter_rope(rng, S, hs)
    V = bf16(rng.standard_normal((B, nh, S, hs)).astype(f32))
    kc = bits(np.broadcast_to(8 * code, (B, nh, S, hs))).copy()
    vc = bits(V).copy()
    for b in range(B):
        kc[b, :, p[b]:] = NAN_BITS
        vc[b, :, p[b]:] = NAN_BITS
    cands = [sorted({c for c in [0, int(pb) - 1, int(pb)] + [e for e in PASS_EDGES if e < pb] if 0 <= c <= pb}) for pb in p]
    launches, gap = [], np.inf
    for r in range(-(-max(len(c) for c in cands) // nh)):
        vrow = bf16(rng.standard_normal((B, nh, hs)).astype(f32))
        q1, k1, want = (np.zeros((B, nh, hs), f32) for _ in range(3))
        qkv = np.zeros((B, 3, nh, hs), f32)
        for b in range(B):
            cs = rope[p[b]]
            for h in range(nh):
                t = cands[b][(r * nh + h) % len(cands[b])]
                q1[b, h], k1[b, h] = 8 * code[h, t], 8 * code[h, p[b]]
                qkv[b, 0, h], qkv[b, 1, h], qkv[b, 2, h] = unrotate(q1[b, h], cs), unrotate(k1[b, h], cs), vrow[b, h]
                want[b, h] = vrow[b, h] if t == p[b] else V[b, h, t]
                gap = min(gap, key_gap(8 * code[h, :p[b] + 1], q1[b, h], t, hs))
        c = rg_dict(name, bits(qkv.reshape(B, 3 * C)), kc, vc, rope)
        launches.append((c, want, q1, k1, vrow))
    assert gap >= MIN_GAP, gap
    return launches, gap


@pytest.mark.parametrize("name", RG_NAMES)
def test_ragged_selected_key_through_rope(hip, name):
    """The only test in which attention must read back the rotated q' and the key written in the same block, not
    merely finite numbers: y = V[b, h, t] (or the row's own v at t = p_b), q_out = 8 code[t], slot p_b of the
    caches = (8 code[p_b], v), every other slot unchanged, all bitwise."""
    launches, gap = rg_selected_case(name)
    print(f"ragged attention {name}: selected-key gap {gap:.0f}")
    for r, (c, want, q1, k1, vrow) in enumerate(launches):
        B, p = c["B"], c["p"]
        yb, qb, kb, vb = rg_launch(hip, c)
        what = f"ragged attention selected key {name} launch {r}"
        np.testing.assert_array_equal(qb, bits(q1).reshape(B, -1), err_msg=what + " q_out")
        kw, vw = c["kc"].copy(), c["vc"].copy()
        for b in range(B):
            kw[b, :, p[b]], vw[b, :, p[b]] = bits(k1[b]), bits(vrow[b])
        np.testing.assert_array_equal(kb, kw, err_msg=what + " k cache")
        np.testing.assert_array_equal(vb, vw, err_msg=what + " v cache")
        got = H.f32_of_bits(yb)
        assert not np.isnan(got).any(), f"{what}: y not written, or a NaN slot read"
        np.testing.assert_array_equal(got, want.reshape(B, -1), err_msg=what + " y")


# ================================================================== 3. llj_attention_adapter
ADP_AT = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64]
ADP_NH = 3
ADP_A = 16.0
GATES = (0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0)
GATES_R = (0.5, -1.0, 2.0, 1.5, -0.75, 1.25, -3.0)  # the rounding cases: not only powers of two, never 0
# (S, B, T, positions): 36 blocks (speculative first pass) and 120 (none unless LLJ_OPT_ATT_SPEC_BATCH)
ADP_LAUNCHES = [(2048, 12, 1, (2047,)), (2048, 12, 1, (2048 + 5,)), (2048, 12, 1, (130,)), (144, 12, 1, (300,)),
                (2048, 5, 8, (2047, 130, 2048 + 5, 63, 64, 0, 1999, 129)), (144, 5, 8, (143, 300, 80, 0, 31, 32, 33, 1))]


def gates_of(table, i, nh=ADP_NH):
    return np.array([table[(i + 3 * h) % len(table)] for h in range(nh)], f32)


@functools.lru_cache(maxsize=None)
def adp_cache_side(hs, S, B, T_, pos):
    """Cache keys 16 code[s] in the first hs / 2 dims (zeros after: adp_keys), V integers |v| <= 4 (int8), Part
    D's targets per (row, head): (code, V, target, q half (rows, nh, hs / 2), gap). The first of SEEDS seeds with
    gap >= MIN_GAP."""
    nh, hh, rows = ADP_NH, hs // 2, B * T_

    def build(seed):
        rng = np.random.default_rng([67, hs, S, B, T_, seed])
        code = codes(rng, nh, S, hh)
        target = np.zeros((rows, nh), np.int64)
        qh = np.zeros((rows, nh, hh), f32)
        gap = np.inf
        for m in range(rows):
            p = int(pos[m % T_])
            last = p if p < S else S - 1
            cand = [0, last, max(last - 1, 0)] + PASS_EDGES
            for h in range(nh):
                t = min(cand[(m + 5 * h) % len(cand)], last)
                target[m, h] = t
                qh[m, h] = ADP_A * code[h, t]
                gap = min(gap, key_gap(ADP_A * code[h, :last + 1], qh[m, h], t, hs))
        if gap < MIN_GAP:
            return None
        V = rng.integers(-4, 5, size=(B, nh, S, hs)).astype(np.int8)
        return code, V, target, qh, gap

    return first_seed(build, f"adapter cache side hs {hs} S {S}")


def adp_keys(code, B, hs):
    K = np.zeros((B,) + code.shape[:2] + (hs,), f32)
    K[..., :hs // 2] = ADP_A * code[None]
    return K


@functools.lru_cache(maxsize=None)
def adp_prefix_side(hs, aT, rows):
    """Prefix keys 16 codeA[j] in the last hs / 2 dims, av integers |v| <= 4, prefix targets per (row, head) over
    0, aT - 1 and 15 / 16 / 17 where below aT: (ak, av, target, q half, gap)."""
    nh, hh = ADP_NH, hs // 2
    cand = sorted({0, aT - 1} | {c for c in (15, 16, 17) if c < aT})

    def build(seed):
        rng = np.random.default_rng([69, hs, aT, seed])
        code = codes(rng, nh, aT, hh)
        av = rng.integers(-4, 5, size=(nh, aT, hs)).astype(f32)
        ta = np.array([[cand[(m + 2 * h) % len(cand)] for h in range(nh)] for m in range(rows)])
        qh = np.stack([[ADP_A * code[h, ta[m, h]] for h in range(nh)] for m in range(rows)])
        gap = min(key_gap(ADP_A * code[h], qh[m, h], ta[m, h], hs) for m in range(rows) for h in range(nh))
        if gap < MIN_GAP:
            return None
        ak = np.zeros((nh, aT, hs), f32)
        ak[..., hh:] = ADP_A * code
        assert {int(t) for t in ta.ravel()} == set(cand) or rows * nh < len(cand)
        return ak, av, ta, qh, gap

    return first_seed(build, f"adapter prefix side hs {hs} aT {aT}")


def adp_two_keys_case(hs, aT, i):
    """Launch i of ADP_LAUNCHES at prefix length aT: (q, code, V, ak, av, gate, want, cache gap, prefix gap)."""
    S, B, T_, pos = ADP_LAUNCHES[i]
    nh, rows = ADP_NH, B * T_
    code, V, t, qk, gap_k = adp_cache_side(hs, S, B, T_, pos)
    ak, av, ta, qa, gap_a = adp_prefix_side(hs, aT, rows)
    g = gates_of(GATES, i + aT)
    q = np.concatenate([qk, qa], -1).reshape(rows, nh * hs)
    want = np.zeros((rows, nh, hs))
    for m in range(rows):
        for h in range(nh):
            want[m, h] = V[m // T_, h, t[m, h]].astype(np.float64) + float(g[h]) * av[h, ta[m, h]]
    want = assert_bf16_values(H._exact32(want, "V[t] + g av[ta]"), "V[t] + g av[ta]").reshape(rows, nh * hs)
    return q, code, V, ak, av, g, want, gap_k, gap_a


_adp_dev = {}


def adp_dev(key, build):
    """Read-only device operands shared by the cases of this file."""
    if key not in _adp_dev:
        _adp_dev[key] = tuple(T(a, torch.bfloat16) for a in build())
        torch.cuda.synchronize()
    return _adp_dev[key]


def run_adapter(hip, qd, kd, vd, pos, B, T_, hs, S, akd, avd, g, aT, nh=ADP_NH):
    y = sentinel(B * T_ + 1, nh * hs)
    pd, gd = T(np.asarray(pos, np.int32)), T(np.asarray(g, f32))
    call(hip, "llj_attention_adapter", qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), y.data_ptr(), pd.data_ptr(), B, T_,
         nh, hs, S, akd.data_ptr(), avd.data_ptr(), gd.data_ptr(), aT, st())
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("spec_full", [0, 1])
@pytest.mark.parametrize("aT", ADP_AT)
@pytest.mark.parametrize("hs", HEADS)
def test_adapter_two_selected_keys(hip, hs, aT, spec_full):
    """One cache key and one prefix key carry all the weight of their softmaxes: y = bf16(V[t] + g av[ta])."""
    with option(hip, _hip.OPT_ATT_SPEC_FULL, spec_full):
        for i, (S, B, T_, pos) in enumerate(ADP_LAUNCHES):
            q, code, V, ak, av, g, want, gap_k, gap_a = adp_two_keys_case(hs, aT, i)
            kd, vd = adp_dev(("kv", hs, i), lambda: (adp_keys(code, B, hs), V.astype(f32)))
            akd, avd = adp_dev(("a", hs, aT, B * T_), lambda: (ak, av))
            y = run_adapter(hip, T(q, torch.bfloat16), kd, vd, pos, B, T_, hs, S, akd, avd, g, aT)
            print(f"adapter hs {hs} aT {aT} S {S}: cache gap {gap_k:.0f}, prefix gap {gap_a:.0f}")
            check(y, want, f"adapter two selected keys hs {hs} aT {aT} S {S} B {B} T {T_} spec_full {spec_full}")


def rounding_case(hs, aT, nkeys, M, fused, dt=0, nh=ADP_NH):
    """Both softmaxes exactly uniform (q = 0, power-of-two key counts), V / av integers up to 127, so y = mean V
    and ay = mean av are exact dyadic numbers. fused: y from the cache (M, nh, nkeys, hs), expected the one
    rounding bf16(y + g ay), wrong the three roundings bf16(bf16(y) + bf16(g bf16(ay))). Otherwise (prefix add):
    y is the input (bf16 values for dt 0), expected the three roundings (which must also differ wherever the
    inner bf16(ay) is dropped, in >= 1 %), wrong the one rounding; dt 1: the float64 value rounded once to fp32.
    The first of SEEDS seeds whose wrong reference differs in >= MIN_DIFFER."""
    assert aT & (aT - 1) == 0 and nkeys & (nkeys - 1) == 0

    def build(seed):
        rng = np.random.default_rng([79, hs, aT, nkeys, M, int(fused), dt, seed])
        av = rng.integers(-127, 128, size=(nh, aT, hs)).astype(f32)
        g = gates_of(GATES_R, seed + aT + M, nh)
        if fused:
            V = rng.integers(-127, 128, size=(M, nh, nkeys, hs)).astype(f32)
            y = H._exact32(V.astype(np.float64).mean(2), "O / L").astype(np.float64)
        else:
            V = None
            if dt == 0:  # bf16 values that are multiples of 1 / 64, so that the fp32 sums below are exact
                y = bf16(rng.integers(-2048, 2049, size=(M, nh, hs)) / 64.0).astype(np.float64)
            else:
                y = (rng.standard_normal((M, nh, hs)) * 8).astype(f32).astype(np.float64)
        ay = H._exact32(av.astype(np.float64).mean(1), "Oa / La").astype(np.float64)[None]
        g64 = g.astype(np.float64)[None, :, None]
        H._exact32(g64 * ay, "g ay")
        inner = H._exact32(g64 * bf16(ay), "g bf16(ay)")
        if dt == 1:
            out = dict(want=(y + g64 * ay).astype(f32))  # one fp32 rounding of the exact float64 sum
            return dict(out, av=av, g=g, y_in=y.astype(f32), seed=seed, share=None)
        one = bf16(H._exact32(y + g64 * ay, "y + g ay"))
        three = bf16(H._exact32(bf16(y).astype(np.float64) + bf16(inner), "bf16(y) + bf16(g bf16(ay))"))
        share = float(np.mean(one != three))
        if share < MIN_DIFFER:
            return None
        if fused:
            return dict(want=one, wrong=three, V=V, av=av, g=g, seed=seed, share=share)
        no_inner = bf16(H._exact32(y + bf16(H._exact32(g64 * ay, "g ay")), "y + bf16(g ay)"))
        share_inner = float(np.mean(no_inner != three))
        if share_inner < 0.01:
            return None
        return dict(want=three, wrong=one, av=av, g=g, y_in=y.astype(f32), seed=seed, share=share, share_inner=share_inner)

    return first_seed(build, f"rounding case hs {hs} aT {aT} keys {nkeys} M {M} fused {fused} dt {dt}")


@pytest.mark.parametrize("spec_full", [0, 1])
@pytest.mark.parametrize("B", [3, 24])
@pytest.mark.parametrize("nkeys", [16, 128])
@pytest.mark.parametrize("aT", [16, 64])
@pytest.mark.parametrize("hs", HEADS)
def test_adapter_single_rounding(hip, hs, aT, nkeys, B, spec_full):
    """The fused kernel rounds once, bf16(O / L + g Oa / La); 9 and 72 blocks."""
    nh, S = ADP_NH, 128
    c = rounding_case(hs, aT, nkeys, B, True)
    rng = np.random.default_rng([83, hs, aT])
    V = np.full((B, nh, S, hs), np.nan, f32)
    V[:, :, :nkeys] = c["V"]
    K = bf16(rng.standard_normal((B, nh, S, hs)).astype(f32))
    K[:, :, nkeys:] = np.nan
    ak = bf16(rng.standard_normal((nh, aT, hs)).astype(f32))
    q = torch.zeros(B, nh * hs, dtype=torch.bfloat16, device=dev)
    with option(hip, _hip.OPT_ATT_SPEC_FULL, spec_full):
        y = run_adapter(hip, q, T(K, torch.bfloat16), T(V, torch.bfloat16), [nkeys - 1], B, 1, hs, S,
                        T(ak, torch.bfloat16), T(c["av"], torch.bfloat16), c["g"], aT)
    print(f"adapter single rounding hs {hs} aT {aT} keys {nkeys} B {B}: three roundings differ in {c['share']:.3f}, "
          f"seed {c['seed']}")
    check(y, c["want"].reshape(B, nh * hs), f"adapter single rounding hs {hs} aT {aT} keys {nkeys} B {B}")


@pytest.mark.parametrize("spec_full", [0, 1])
@pytest.mark.parametrize("hs", HEADS)
def test_adapter_prefix_visible_set(hip, hs, spec_full):
    """Probe av (av[h, j, d] = 1 iff j == d) over a zero V cache: column d of a head is g / aT for d < aT and
    exactly 0 from aT on (a prefix key past aT, or the unwritten score slots in LDS, would show), every aT."""
    nh, S, B, p = ADP_NH, 64, 2, 40
    rng = np.random.default_rng([89, hs])
    q = torch.zeros(B, nh * hs, dtype=torch.bfloat16, device=dev)
    kd = T(bf16(rng.standard_normal((B, nh, S, hs)).astype(f32)), torch.bfloat16)
    vd = torch.zeros(B, nh, S, hs, dtype=torch.bfloat16, device=dev)
    with option(hip, _hip.OPT_ATT_SPEC_FULL, spec_full):
        for aT in ADP_AT:
            av = np.zeros((nh, aT, hs), f32)
            j = np.arange(min(aT, hs))
            av[:, j, j] = 1.0
            ak = bf16(rng.standard_normal((nh, aT, hs)).astype(f32))
            g = gates_of(GATES_R, aT)
            y = run_adapter(hip, q, kd, vd, [p], B, 1, hs, S, T(ak, torch.bfloat16), T(av, torch.bfloat16), g, aT)
            got = read_rows(y, B).reshape(B, nh, hs)
            for h in range(nh):
                check_visible(got[:, h] / g[h], 0, [aT] * B, f"adapter prefix probe hs {hs} aT {aT} head {h}")


# ================================================================== 4. llj_adapter_prefix_add
PA_HEADS = [64, 128, 78]  # 78: the scalar path


def run_prefix_add(hip, q, ak, av, g, y_in, M, hs, aT, dt, nh=ADP_NH):
    """y (M + 1, C) after the in-place add: rows < M from y_in, the last row a sentinel. Returns the host array
    (uint16 bf16 bit patterns for dt 0, float32 for dt 1) of the M rows."""
    tt = torch.bfloat16 if dt == 0 else torch.float32
    C = nh * hs
    if dt == 0:
        y = sentinel(M + 1, C)
        y[:M] = T(assert_bf16_values(y_in, "y_in"), tt).view(torch.int16)
    else:
        y = torch.full((M + 1, C), NAN, dtype=tt, device=dev)
        y[:M] = T(y_in)
    qd, akd, avd, gd = T(q, tt), T(ak, tt), T(av, tt), T(np.asarray(g, f32))
    call(hip, "llj_adapter_prefix_add", qd.data_ptr(), akd.data_ptr(), avd.data_ptr(), gd.data_ptr(), y.data_ptr(), M, nh,
         hs, aT, dt, st())
    torch.cuda.synchronize()
    if dt == 0:
        return read_rows(y, M)
    out = y.cpu().numpy()
    assert np.isnan(out[M]).all(), "wrote past the last row"
    return out[:M]


def assert_same(got, want, what):
    assert not np.isnan(got).any(), f"{what}: not written (or NaN)"
    bad = got != want
    assert not bad.any(), (f"{what}: {bad.sum()} / {bad.size} elements differ; first at {tuple(np.argwhere(bad)[0])}: got "
                           f"{got[tuple(np.argwhere(bad)[0])]!r}, want {want[tuple(np.argwhere(bad)[0])]!r}")


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("hs", PA_HEADS)
@pytest.mark.parametrize("M", [1, 37])
@pytest.mark.parametrize("aT", [16, 64])
def test_prefix_add_rounding_points(hip, aT, M, hs, dt):
    """bf16: the reference's three roundings, bf16(bf16(y) + bf16(g bf16(ay))), bitwise; fp32: the float64 value
    rounded once."""
    nh = ADP_NH
    c = rounding_case(hs, aT, 1, M, False, dt)
    rng = np.random.default_rng([97, hs, aT, M])
    rnd = bf16 if dt == 0 else (lambda a: a)
    ak = rnd(rng.standard_normal((nh, aT, hs)).astype(f32))
    got = run_prefix_add(hip, np.zeros((M, nh * hs), f32), ak, c["av"], c["g"], c["y_in"].reshape(M, -1), M, hs, aT, dt)
    if dt == 0:
        print(f"prefix add hs {hs} aT {aT} M {M}: one rounding differs in {c['share']:.3f}, without the inner "
              f"bf16(ay) in {c['share_inner']:.3f}, seed {c['seed']}")
    assert_same(got, c["want"].reshape(M, -1), f"prefix add rounding hs {hs} aT {aT} M {M} dt {dt}")


def pa_selected_case(hs, aT, M, nh=ADP_NH):
    """Full-width codes: ak = 8 codeA[j], q = 8 codeA[ta]; y_in and av integers |v| <= 4, gates in GATES:
    y_in + g av[ta] is a bf16 value. Prefix targets as adp_prefix_side."""
    cand = sorted({0, aT - 1} | {c for c in (15, 16, 17) if c < aT})

    def build(seed):
        rng = np.random.default_rng([101, hs, aT, M, seed])
        code = codes(rng, nh, aT, hs)
        av = rng.integers(-4, 5, size=(nh, aT, hs)).astype(f32)
        y_in = rng.integers(-4, 5, size=(M, nh, hs)).astype(f32)
        g = gates_of(GATES, aT + seed, nh)
        ta = np.array([[cand[(m + 2 * h) % len(cand)] for h in range(nh)] for m in range(M)])
        q = np.stack([[8 * code[h, ta[m, h]] for h in range(nh)] for m in range(M)])
        gap = min(key_gap(8 * code[h], q[m, h], ta[m, h], hs) for m in range(M) for h in range(nh))
        if gap < MIN_GAP:
            return None
        want = y_in.astype(np.float64) + g.astype(np.float64)[None, :, None] * np.stack(
            [[av[h, ta[m, h]] for h in range(nh)] for m in range(M)])
        want = assert_bf16_values(H._exact32(want, "y_in + g av[ta]"), "y_in + g av[ta]")
        return dict(q=q.reshape(M, -1), ak=8 * code, av=av, g=g, y_in=y_in.reshape(M, -1), want=want.reshape(M, -1), gap=gap)

    return first_seed(build, f"prefix add selected key hs {hs} aT {aT}")


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("hs", PA_HEADS)
def test_prefix_add_selected_key(hip, hs, dt):
    M = 37
    for aT in ADP_AT:
        c = pa_selected_case(hs, aT, M)
        got = run_prefix_add(hip, c["q"], c["ak"], c["av"], c["g"], c["y_in"], M, hs, aT, dt)
        print(f"prefix add hs {hs} aT {aT}: selected-key gap {c['gap']:.0f}")
        assert_same(got, c["want"], f"prefix add selected key hs {hs} aT {aT} dt {dt}")


# ================================================================== 5. llj_attention_i8
I8_S, I8_P, I8_M, I8_NH = 2048, 2047, 8, 2


@pytest.mark.parametrize("nsplit", [1, 16])
@pytest.mark.parametrize("hs", HEADS)
def test_attention_i8_is_the_plain_kernel_bitwise(hip, hs, nsplit):
    """y of llj_attention_i8 on Part D's selected-key inputs is V[target], bitwise llj_attention's (nsplit 1) /
    llj_attention_split's (nsplit 16), and the clear block comes back zero."""
    nh, S, M = I8_NH, I8_S, I8_M
    C = nh * hs
    q, K, V, want, gap, _ = selected_key_case(hs, nh, S, M, 1, [I8_P], I8_P)
    qd, kd, vd, pd = T(q, torch.bfloat16), T(K, torch.bfloat16), T(V, torch.bfloat16), T(np.array([I8_P], np.int32))
    ws = torch.empty(max(hip.llj_attention_ws_bytes(M, nh, hs, nsplit), 16), dtype=torch.uint8, device=dev)
    y, y_ref = sentinel(M + 1, C), sentinel(M + 1, C)
    y_st = torch.zeros(hip.llj_i8_rowstats_bytes(C) // 4, dtype=torch.int32, device=dev)
    clr = torch.full((600,), 7, dtype=torch.int32, device=dev)
    call(hip, "llj_attention_i8", qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), y.data_ptr(), pd.data_ptr(), M, 1, nh, hs, S,
         nsplit, ws.data_ptr(), y_st.data_ptr(), clr.data_ptr(), clr.numel() - 1, H.I8_THR, st())
    if nsplit == 1:
        call(hip, "llj_attention", qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), y_ref.data_ptr(), pd.data_ptr(), M, 1, nh,
             hs, S, st())
    else:
        call(hip, "llj_attention_split", qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), y_ref.data_ptr(), pd.data_ptr(), M,
             1, nh, hs, S, nsplit, ws.data_ptr(), st())
    torch.cuda.synchronize()
    what = f"attention_i8 hs {hs} nsplit {nsplit}"
    c = clr.cpu().numpy()
    assert not c[:-1].any(), f"{what}: the clear block is not zero"
    assert c[-1] == 7, f"{what}: cleared past clr_words"
    assert np.array_equal(words(y), words(y_ref)), f"{what}: y differs from the plain kernel's"
    check(y, want, what)
