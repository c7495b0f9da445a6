"""The input conditions of tests/test_attention_variants_exact_gpu.py, on the CPU: for every case that file runs,
the selected-key gaps (>= MIN_GAP, over the visible keys only), the exact representability of every expected
value (fp32 for the intermediate sums, bf16 where one bit pattern is claimed), the share in which each
wrong-rounding reference differs (>= 10 %, the first of 16 seeds that meets it) and the coverage of the key-range
boundaries by the targets are decided by the references alone, before any GPU run. Each group prints its figures."""
import numpy as np
import pytest

from tests import helpers as H
from tests import test_attention_variants_exact_gpu as V
from tests.test_streaming_exact_gpu import MIN_GAP, PASS_EDGES, selected_key_case


def test_shared_key_ranges():
    """The shapes reach what they are there for: ranges that begin and end inside a 64-key pass, empty ranges, a
    second row group with live rows, and p on either side of P and of the passes after it."""
    assert V.sh_ranges(200, 3) == [(0, 67), (67, 134), (134, 200)]
    assert len(V.sh_ranges(200, 64)) == 4 and V.sh_ranges(200, 64)[-1] == (192, 200)
    assert V.sh_ranges(1500, 7)[1] == (215, 430) and len(V.sh_ranges(1500, 7)) == 7
    assert len(V.sh_ranges(1500, 32)) == 24 and V.sh_ranges(1, 64) == [(0, 1)]
    for S, B, nsplit in V.SH_GRID:
        assert 1 <= nsplit <= 64 and (B == 1 or B % 8 in (1, 4))
        for P, p in V.sh_shapes(S):
            assert 1 <= P <= S and P - 1 <= p < S  # the kernel's contract
            r = V.sh_ranges(P, nsplit)
            assert r[0][0] == 0 and r[-1][1] == P and all(a[1] == b[0] for a, b in zip(r, r[1:]))
            dead = V.sh_dead(B, S, P, p)
            assert not dead[0, :p + 1].any() and dead[:, p + 1:].all() and dead[1:, :P].all() and not dead[:, P:p + 1].any()
    assert {p - P for P, p in V.sh_shapes(320) if P == 129} == {-1, 0, 62, 63, 64, 190}
    assert len(V.sh_shapes(320)) == 36


@pytest.mark.parametrize("S,B,nsplit", V.SH_GRID)
@pytest.mark.parametrize("hs", V.HEADS)
def test_shared_selected_key_conditions(hs, S, B, nsplit):
    gap = np.inf
    for P, p in V.sh_shapes(S):
        launches, g, cand = V.sh_selected_case(hs, S, B, P, p, nsplit)
        gap = min(gap, g)
        edges = {e for lo, hi in V.sh_ranges(P, nsplit) for e in (lo, hi - 1)}
        assert {c for c in edges | {0, P - 1, P, p - 1, p} | set(PASS_EDGES) if 0 <= c <= p} == set(cand)
        code, val = V.sh_base(hs, S, B)
        for q, want in launches:
            assert np.array_equal(H.bf16(q), q) and np.array_equal(H.bf16(want), want)
        if B > 1:  # the rows' values differ, so the row a value is taken from matters
            assert (val[0, :, :p + 1] != val[1, :, :p + 1]).mean() > 0.99
    print(f"shared hs {hs} S {S} B {B} nsplit {nsplit}: smallest selected-key gap {gap:.0f}")
    assert gap >= MIN_GAP


@pytest.mark.parametrize("name", V.RG_NAMES)
def test_ragged_conditions(name):
    hs, nh, S, p, pos, off = V.rg_shape(name)
    B, C = len(p), nh * hs
    for o in range(0, S, C):
        c = V.rg_visible_case(name, o)
        qkv = c["qkv"].reshape(B, 3, nh, hs)
        assert not qkv[:, 0].any()  # q = 0
        for b in range(B):
            assert (c["kc"][b, :, p[b]:] == V.NAN_BITS).all() and (c["vc"][b, :, p[b]:] == V.NAN_BITS).all()
            assert not np.isnan(H.f32_of_bits(c["kc"][b, :, :p[b]])).any()
            cols = np.flatnonzero(qkv[b, 2].reshape(C))  # the row's v: the probe's value of slot p_b
            assert list(cols) == ([p[b] - o] if 0 <= p[b] - o < C else [])
    launches, gap = V.rg_selected_case(name)
    seen = [set() for _ in range(B)]
    for c, want, q1, k1, vrow in launches:
        rope = c["rope"]
        assert set(map(tuple, rope.reshape(-1, 2))) == {(1, 0), (0, 1), (-1, 0), (0, -1)}
        qkv = H.f32_of_bits(c["qkv"]).reshape(B, 3, nh, hs)
        for b in range(B):
            # the kernel's RoPE at p_b gives back the +-8 codes exactly, and the inputs are not the codes themselves
            assert np.array_equal(H.rope_bf16(qkv[b, 0], rope[p[b]][None]), q1[b])
            assert np.array_equal(H.rope_bf16(qkv[b, 1], rope[p[b]][None]), k1[b])
            assert (np.abs(q1[b]) == 8).all() and (qkv[b, 0] != q1[b]).any()
        for b in range(B):
            kc = H.f32_of_bits(c["kc"][b])
            for h in range(nh):
                hit = np.flatnonzero((kc[h, :p[b]] == q1[b, h]).all(-1))
                seen[b].add(int(hit[0]) if len(hit) else int(p[b]))
    for b in range(B):
        assert seen[b] == {s for s in [0, p[b] - 1, p[b]] + [e for e in PASS_EDGES if e < p[b]] if 0 <= s <= p[b]}
    print(f"ragged {name}: smallest selected-key gap {gap:.0f}, {len(launches)} launches")
    assert gap >= MIN_GAP


@pytest.mark.parametrize("hs", V.HEADS)
def test_adapter_two_selected_keys_conditions(hs):
    gk, ga = np.inf, np.inf
    for aT in V.ADP_AT:
        for i, (S, B, T_, pos) in enumerate(V.ADP_LAUNCHES):
            q, code, val, ak, av, g, want, gap_k, gap_a = V.adp_two_keys_case(hs, aT, i)
            gk, ga = min(gk, gap_k), min(ga, gap_a)
            assert np.array_equal(H.bf16(want), want) and np.array_equal(H.bf16(q), q)
            assert not ak[..., :hs // 2].any() and (np.abs(ak[..., hs // 2:]) == V.ADP_A).all()
            assert np.abs(val).max() <= 4 and np.abs(av).max() <= 4 and set(g) <= set(V.GATES)
            assert (3 * B * T_ <= 64) == (T_ == 1)  # both sides of the speculative-pass switch
        ta = V.adp_prefix_side(hs, aT, 12)[2]
        assert {int(t) for t in ta.ravel()} == {0, aT - 1} | {c for c in (15, 16, 17) if c < aT}
    print(f"adapter hs {hs}: smallest cache-side gap {gk:.0f}, prefix-side gap {ga:.0f}")
    assert min(gk, ga) >= MIN_GAP


def test_rounding_conditions():
    """The uniform-softmax cases: every expected value exact (asserted inside), the wrong-rounding references
    differ in >= 10 % (prefix add: also >= 1 % where only the inner bf16(ay) is dropped)."""
    fused, add, inner, seeds = [], [], [], set()
    for hs in V.HEADS:
        for aT in (16, 64):
            for nkeys in (16, 128):
                for B in (3, 24):
                    c = V.rounding_case(hs, aT, nkeys, B, True)
                    fused.append(c["share"])
                    seeds.add(c["seed"])
                    assert np.array_equal(H.bf16(c["want"]), c["want"])
    for hs in V.PA_HEADS:
        for aT in (16, 64):
            for M in (1, 37):
                c = V.rounding_case(hs, aT, 1, M, False, 0)
                add.append(c["share"])
                inner.append(c["share_inner"])
                seeds.add(c["seed"])
                assert np.array_equal(H.bf16(c["y_in"]), c["y_in"]) and not set(c["g"]) <= {0.5, -1.0, 2.0}
                c = V.rounding_case(hs, aT, 1, M, False, 1)
                assert c["want"].dtype == np.float32
    print(f"fused kernel: the three-rounding result differs in {min(fused):.3f} - {max(fused):.3f}; prefix add: the "
          f"one-rounding result in {min(add):.3f} - {max(add):.3f}, without the inner rounding {min(inner):.3f} - "
          f"{max(inner):.3f}; seeds {sorted(seeds)}")
    assert min(fused + add) >= V.MIN_DIFFER and min(inner) >= 0.01


@pytest.mark.parametrize("hs", V.PA_HEADS)
def test_prefix_add_selected_key_conditions(hs):
    gap = min(V.pa_selected_case(hs, aT, 37)["gap"] for aT in V.ADP_AT)
    print(f"prefix add hs {hs}: smallest selected-key gap {gap:.0f}")
    assert gap >= MIN_GAP


@pytest.mark.parametrize("hs", V.HEADS)
def test_attention_i8_conditions(hs):
    gap = selected_key_case(hs, V.I8_NH, V.I8_S, V.I8_M, 1, [V.I8_P], V.I8_P)[4]
    print(f"attention_i8 hs {hs}: selected-key gap {gap:.0f}")
    assert gap >= MIN_GAP
