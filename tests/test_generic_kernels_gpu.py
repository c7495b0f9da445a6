"""The any-shape kernels (csrc/generic.hip, and the fp32 sampler of csrc/ops.hip) one entry point at a
time against plain numpy in float64 -- bitwise wherever the inputs make fp32 arithmetic exact (small
integers, powers of two: no dependence on summation order or FMA contraction), otherwise within a bound
derived from the number formats. These kernels run every model the streaming kernels do not tile (the
125M: n_embd 780 / head 78; the reference test's n_embd 32 / head 2; every float32 model), and
tests/test_adapter_v2_kernels_gpu.py and tests/test_lora_kernels_gpu.py take their expected values
from two of them: llj_g_rope_kv and llj_g_silu_mul are pinned here (test_rope_kv_*, test_silu_mul_*), so
those files compare the fused epilogues with kernels that are themselves checked.

    entry point       direct tests in this file
    llj_g_linear      test_linear_dense_exact, test_linear_quant_exact, test_linear_strides_and_residual,
                      test_linear_argument_rules, test_linear_random_vs_float64
    llj_g_rmsnorm     test_rmsnorm_fp32_vs_float64, test_rmsnorm_bf16_vs_oracle, test_rmsnorm_exact
    llj_g_rope_kv     test_rope_kv_exact, test_rope_kv_real_table, test_rope_kv_argument_rules
    llj_g_attention   test_attention_visible_set, test_attention_random_vs_float64, test_attention_score_spread,
                      test_attention_lds_guard, test_attention_largest_accepted
    llj_g_silu_mul    test_silu_mul_vs_float64, test_silu_mul_in_place
    llj_g_argmax      test_argmax_ties_and_edges
    llj_g_embedding   test_embedding_rows_and_pos_inc (and llj_embedding at C % 8 != 0)
    llj_g_sample      test_sample_fp32_vs_restatement
    (llj_g_i8_linear: tests/test_generic_gpu.py::test_generic_int8_linear_vs_oracle; llj_g_linear_v2 /
    llj_g_linear_lora: bitwise against numpy on exact operands in tests/test_epilogue_exact_gpu.py
    (test_g_linear_v2_exact, test_g_linear_lora_exact) -- the adapter v2 / LoRA kernel tests compare them with
    llj_g_linear followed by torch arithmetic, which covers their argument rules and identity forms only;
    llj_g_nll: tests/test_nll_kernels_gpu.py)

dt = 0 is bf16 (inputs are bf16 values, outputs compared after the reference's rounding points), dt = 1
fp32. Padding columns and untouched cache slots are pre-filled with a sentinel and compared too.

Measured on the MI355X (llj_g_attention, dt = 1, error per (row, head) as max |d| / max |ref|; the bound
is 4 x the error of the same attention in numpy float32 with the keys in reversed order, floor 2^-20;
printed by test_attention_random_vs_float64 / test_attention_largest_accepted):
    case (hs, S, p0, T)        kernel err   bound      (numpy float32, keys reversed)
    2, 8, 0, 4                 1.84e-07     9.54e-07   1.43e-07
    78, 16, 15, 1              5.19e-07     1.07e-06   2.68e-07
    78, 16, 16, 1              8.23e-07     2.03e-06   5.08e-07
    78, 16, 37, 1              2.57e-07     9.54e-07   1.85e-07
    6, 300, 299, 1             3.82e-07     1.51e-06   3.78e-07
    6, 300, 255, 3             1.27e-06     2.82e-06   7.06e-07
    scores to +-60             1.17e-07     9.54e-07   1.13e-07
    scores to +-120            1.00e-07     9.54e-07   7.71e-08
    78, 16302, 16301, 1        2.85e-06     1.69e-05   4.21e-06
The whole file takes about 3 s on the MI355X.
"""
import numpy as np
import pytest
import torch

from oracle import llama_np as O
from tests.helpers import assert_bf16_close, bf16
from tests.test_kernels_gpu import T, call, st

pytestmark = pytest.mark.gpu
dev = "cuda"
EINVAL = 1000
SENT = -32768.0  # bf16-representable, outside every value the tests produce
F64 = np.float64
TD = {0: torch.bfloat16, 1: torch.float32}
DT = pytest.mark.parametrize("dt", [0, 1], ids=["bf16", "fp32"])


def D(a, dt):
    return T(np.asarray(a, np.float32), TD[dt])


def H(t):
    torch.cuda.synchronize()
    return t.float().cpu().numpy()


def rnd(a, dt):
    """The values a tensor of type dt holds / the rounding of an output of type dt."""
    return bf16(a) if dt == 0 else np.asarray(a, np.float32)


def filled(shape, dt, v=SENT):
    return torch.full(shape, v, dtype=TD[dt], device=dev)


def _ordered(a):
    b = O.to_bf16_bits(np.asarray(a, np.float32)).astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7FFF), b)


def bf16_steps(a, b):
    """Distance of two arrays of bf16 values in bf16 ulps (+0 and -0 coincide)."""
    return np.abs(_ordered(a) - _ordered(b))


# ---------------------------------------------------------------------------------------- llj_g_linear
def quant_weight(rng, N, K, bits, group, exact):
    """Random ColBlock codes packed as include/lit_llama_amd.h describes (byte (n, j) at j*N + n, 8 / bits
    codes per byte, low bits first), scales / zeros (N, G). exact: integer zeros and power-of-two scales.
    Returns (device operands, the fp32 weight (q - zero) * scale)."""
    epb, G = 8 // bits, (K + group - 1) // group
    q = rng.integers(0, 1 << bits, (N, K)).astype(np.uint8)
    logical = np.zeros((N, K // epb), np.uint8)
    for r in range(epb):
        logical |= (q[:, r::epb] << (r * bits)).astype(np.uint8)
    np.testing.assert_array_equal(O.colblock_unpack_q(logical, bits), q)  # the packing, against the oracle's unpack
    if exact:
        zr = rng.integers(0, 1 << bits, (N, G)).astype(np.float32)
        sc = (2.0 ** rng.integers(-3, 0, (N, G))).astype(np.float32)
    else:
        zr = rng.uniform(0, (1 << bits) - 1, (N, G)).astype(np.float32)
        sc = (rng.uniform(0.5, 1.5, (N, G)) * 0.05 / (1 << (bits - 1))).astype(np.float32)
    Wd = (q.astype(np.float32) - np.repeat(zr, group, 1)[:, :K]) * np.repeat(sc, group, 1)[:, :K]
    np.testing.assert_array_equal(Wd, O.colblock_get_weight(logical, sc, zr, bits, tile_cols=group))
    ops = dict(wkind=0, W=T(logical.T.copy()), sc=T(sc), zr=T(zr), bits=bits, group=group)
    return ops, Wd


def dense_weight(W, dt):
    return dict(wkind=1, W=D(W, dt), sc=None, zr=None, bits=0, group=0)


def P(t):
    return None if t is None else t.data_ptr()


def run_linear(hip, dt, x, w, N, ldx=None, ldy=None, resid=None, ldr=None, alias=False):
    """llj_g_linear on host values x (M, K); returns the whole (M, ldy) output buffer, padding included.
    resid: host values (M, N), in a buffer of its own (row stride ldr) or, alias, in y itself."""
    M, K = x.shape
    ldx, ldy = ldx or K, ldy or N
    xd = filled((M + 1, ldx), dt)  # x, y and resid carry one more row of sentinels: row M is nobody's
    xd[:M, :K] = D(x, dt)
    y = filled((M + 1, ldy), dt)
    rd = None
    if resid is not None and alias:
        y[:M, :N] = D(resid, dt)
        rd, ldr = y, ldy
    elif resid is not None:
        rd = filled((M + 1, ldr), dt)
        rd[:M, :N] = D(resid, dt)
    call(hip, "llj_g_linear", w["wkind"], xd.data_ptr(), ldx, M, K, w["W"].data_ptr(), P(w["sc"]), P(w["zr"]),
         w["bits"], w["group"], N, y.data_ptr(), ldy, P(rd), ldr or 0, dt, st())
    got = H(y)
    np.testing.assert_array_equal(got[M], np.full(ldy, SENT, np.float32), err_msg="a row past M was written")
    return got[:M]


def exact_x(rng, M, K):
    return rng.integers(-4, 5, (M, K)).astype(np.float32)


def assert_exact_range(x, W, unit=1.0):
    """Every partial sum of x . W, in any order, is a multiple of `unit` below 2^24 of them: exact in fp32."""
    assert (np.abs(x).astype(F64) @ np.abs(W).astype(F64).T).max() / unit < 2 ** 24


@DT
@pytest.mark.parametrize("M,K,N", [(1, 2, 6), (8, 32, 96), (9, 780, 37), (17, 2304, 10)])
def test_linear_dense_exact(hip, dt, M, K, N):
    """Dense weights, integer x in [-4, 4] and W in [-8, 8]: bitwise. K below one wave; a second row
    block with one row; N % 4 != 0 (one live wave in the last workgroup); the 125M's n_hidden as K."""
    rng = np.random.default_rng(M * 1000 + K + N)
    x, W = exact_x(rng, M, K), rng.integers(-8, 9, (N, K)).astype(np.float32)
    assert_exact_range(x, W)
    got = run_linear(hip, dt, x, dense_weight(W, dt), N)
    np.testing.assert_array_equal(got, rnd(x.astype(F64) @ W.astype(F64).T, dt))


@DT
@pytest.mark.parametrize("group", [780, 256, 100], ids=["tile-1", "g256", "g100"])
@pytest.mark.parametrize("bits", [2, 4, 8])
def test_linear_quant_exact(hip, dt, bits, group):
    """ColBlock codes of 2 / 4 / 8 bits, one group (tile_cols = -1), groups of 256 (the last partial) and
    of 100, integer zeros and scales in {2^-3, 2^-2, 2^-1}: every product and sum is exact, so bitwise."""
    M, K, N = 9, 780, 37
    rng = np.random.default_rng(bits * 1000 + group)
    x = exact_x(rng, M, K)
    w, Wd = quant_weight(rng, N, K, bits, group, exact=True)
    assert_exact_range(x, Wd, unit=2.0 ** -3)
    got = run_linear(hip, dt, x, w, N)
    np.testing.assert_array_equal(got, rnd(x.astype(F64) @ Wd.astype(F64).T, dt))


@DT
@pytest.mark.parametrize("resid", ["none", "distinct", "alias"])
@pytest.mark.parametrize("kind", ["dense", "int4"])
def test_linear_strides_and_residual(hip, dt, kind, resid):
    """Row strides ldx = K + 3, ldy = N + 5 (the padding of y keeps its sentinel; that of x is never
    read: it holds the sentinel too), the residual from a buffer of its own (ldr = N + 1) or from y
    itself: bf16(resid + bf16(sum)) on the bf16 path, resid + sum in fp32. Exact inputs: bitwise."""
    M, K, N = 9, 780, 37
    rng = np.random.default_rng(len(kind) * 10 + len(resid) + dt)
    x = exact_x(rng, M, K)
    if kind == "dense":
        Wd = rng.integers(-8, 9, (N, K)).astype(np.float32)
        w = dense_weight(Wd, dt)
        assert_exact_range(x, Wd)
    else:
        w, Wd = quant_weight(rng, N, K, 4, 256, exact=True)
        assert_exact_range(x, Wd, unit=2.0 ** -3)
    res = None if resid == "none" else rng.integers(-16, 17, (M, N)).astype(np.float32)
    got = run_linear(hip, dt, x, w, N, ldx=K + 3, ldy=N + 5, resid=res, ldr=N + 1, alias=resid == "alias")
    want = rnd(x.astype(F64) @ Wd.astype(F64).T, dt)
    if res is not None:
        want = rnd(res.astype(F64) + want, dt)
    np.testing.assert_array_equal(got[:, :N], want)
    np.testing.assert_array_equal(got[:, N:], np.full((M, 5), SENT, np.float32))


@pytest.mark.parametrize("rule", ["bits=3", "K%epb(4)", "K%epb(2)", "ldy<N", "dt=2", "no scales", "no zeros", "ldx<K",
                                  "ldr<N"])
def test_linear_argument_rules(hip, rule):
    """What the entry point refuses: LLJ_EINVAL and nothing launched (y keeps its sentinel)."""
    M, K, N = 2, 16, 8
    x, y, res = filled((M, 32), 0, 1.0), filled((M, N), 0), filled((M, N), 0, 1.0)
    codes = torch.zeros(32 * N, dtype=torch.uint8, device=dev)
    sc, zr = torch.ones(N, 4, device=dev), torch.zeros(N, 4, device=dev)
    a = dict(wkind=0, x=x.data_ptr(), ldx=32, M=M, K=K, W=codes.data_ptr(), sc=sc.data_ptr(), zr=zr.data_ptr(), bits=4,
             group=K, N=N, y=y.data_ptr(), ldy=N, resid=None, ldr=0, dt=0)
    assert hip.llj_g_linear(*a.values(), st()) == 0  # the base arguments are accepted
    y.fill_(SENT)
    a.update({"bits=3": dict(bits=3), "K%epb(4)": dict(K=15), "K%epb(2)": dict(bits=2, K=18), "ldy<N": dict(ldy=N - 1),
              "dt=2": dict(dt=2), "no scales": dict(sc=None), "no zeros": dict(zr=None), "ldx<K": dict(ldx=K - 1),
              "ldr<N": dict(resid=res.data_ptr(), ldr=N - 1)}[rule])
    assert hip.llj_g_linear(*a.values(), st()) == EINVAL
    np.testing.assert_array_equal(H(y), np.full((M, N), SENT, np.float32))


@DT
@pytest.mark.parametrize("kind", ["dense", "int4-g256"])
def test_linear_random_vs_float64(hip, dt, kind):
    """Standard-normal x, weights of scale 0.05 (dense, or 4-bit codes in groups of 256 with non-integer
    zeros; the weight element (q - zero) * scale evaluated in fp32 as the header says) against the float64
    product. bf16: one output rounding (assert_bf16_close's defaults). fp32: |d| <= K 2^-23 sum_k |x||w|,
    the forward bound of an fp32 dot product of length K in any order (gamma_K = K u / (1 - K u) with
    u = 2^-24, times sum |x||w|; K 2^-23 is twice K u)."""
    M, K, N = 9, 780, 37
    rng = np.random.default_rng(7 + len(kind))
    x = rnd(rng.standard_normal((M, K)), dt)
    if kind == "dense":
        Wd = rnd(rng.standard_normal((N, K)) * 0.05, dt)
        w = dense_weight(Wd, dt)
    else:
        w, Wd = quant_weight(rng, N, K, 4, 256, exact=False)
    ref = x.astype(F64) @ Wd.astype(F64).T
    got = run_linear(hip, dt, x, w, N)
    if dt == 0:
        assert_bf16_close(got, ref, f"g_linear {kind}")
    else:
        bound = K * 2.0 ** -23 * (np.abs(x).astype(F64) @ np.abs(Wd).astype(F64).T)
        err = np.abs(got - ref)
        print(f"[g_linear {kind} fp32] max err / bound {(err / bound).max():.3e}")
        assert (err <= bound).all()


# --------------------------------------------------------------------------------------- llj_g_rmsnorm
RMS_C = [2, 32, 780, 1000]  # below one wave; not a multiple of 256; not a multiple of 8
EPS = float(np.float32(1e-5))


def run_rmsnorm(hip, dt, x, w, eps=EPS):
    """llj_g_rmsnorm with ldx = C + 2, ldy = C + 4; returns the (M, C) result after checking the padding."""
    M, C = x.shape
    xd = filled((M, C + 2), dt)
    xd[:, :C] = D(x, dt)
    wd, y = D(w, dt), filled((M, C + 4), dt)
    call(hip, "llj_g_rmsnorm", xd.data_ptr(), C + 2, wd.data_ptr(), eps, y.data_ptr(), C + 4, M, C, dt, st())
    got = H(y)
    np.testing.assert_array_equal(got[:, C:], np.full((M, 4), SENT, np.float32))
    return got[:, :C]


@pytest.mark.parametrize("C", RMS_C)
def test_rmsnorm_fp32_vs_float64(hip, C):
    """fp32 rows of three magnitudes against O.rmsnorm's formula in float64: relative error per element
    <= 2^-21 (a C-term fp32 mean, one rsqrtf and two products; an allowance, not a measurement)."""
    rng = np.random.default_rng(C)
    x = (rng.standard_normal((3, C)) * np.array([[0.1], [1.0], [30.0]])).astype(np.float32)
    w = rng.uniform(0.5, 1.5, C).astype(np.float32)
    x64 = x.astype(F64)
    ref = w.astype(F64) * x64 / np.sqrt((x64 * x64).mean(-1, keepdims=True) + EPS)
    np.testing.assert_allclose(O.rmsnorm(x, w, EPS), ref, rtol=1e-5)  # the restatement is the oracle's formula
    got = run_rmsnorm(hip, 1, x, w)
    rel = np.abs(got - ref) / np.abs(ref)
    print(f"[g_rmsnorm fp32 C={C}] max rel err {rel.max():.3e} (bound {2.0 ** -21:.3e})")
    assert (rel <= 2.0 ** -21).all()


def rms_bf16_inputs(C):
    """bf16 rows whose mean of squares lies within 1e-3 of a value with an exact bf16 square root (2.25,
    0.5625, 6.25; the bf16 interval around each reaches 2.5e-3 or more to either side): there the
    oracle's two rsqrt variants (one rounding, or torch's CPU sqrt-then-reciprocal) agree, and no
    summation order moves the rounded mean."""
    rng = np.random.default_rng(100 + C)
    rows = []
    for target in (2.25, 0.5625, 6.25):
        while True:  # a narrow row's mean moves with the rounding of x: draw until it is within 1e-3 of the target
            x = rng.standard_normal(C)
            x = bf16(x * np.sqrt(target / (bf16(x).astype(F64) ** 2).mean()))
            means = (x.astype(F64) ** 2).mean(), bf16(x * x).astype(F64).mean()  # exact squares; squares rounded
            if max(abs(m / target - 1) for m in means) < 1e-3:
                break
        rows.append(x)
    return np.array(rows), bf16(rng.uniform(0.5, 1.5, C))


@pytest.mark.parametrize("C", RMS_C)
def test_rmsnorm_bf16_vs_oracle(hip, C):
    """bf16 rows against O.rmsnorm_bf16 (every op of model.py:276-283 rounded to bf16): at most 1 bf16 ulp
    per element and at most 2 % of the elements different at all. The inputs hold the reference's own
    two rsqrt variants to the same 2 % (checked here on the host)."""
    x, w = rms_bf16_inputs(C)
    ref, ref_cpu = O.rmsnorm_bf16(x, w, EPS), O.rmsnorm_bf16(x, w, EPS, cpu_rsqrt=True)
    assert (ref != ref_cpu).mean() <= 0.02 and bf16_steps(ref, ref_cpu).max() <= 1
    got = run_rmsnorm(hip, 0, x, w)
    steps = bf16_steps(got, ref)
    print(f"[g_rmsnorm bf16 C={C}] {np.count_nonzero(steps)} / {steps.size} elements differ, max {steps.max()} ulp")
    assert steps.max() <= 1 and (steps != 0).mean() <= 0.02


@DT
@pytest.mark.parametrize("C", [32, 320])
def test_rmsnorm_exact(hip, dt, C):
    """x = +-2^j, w = 1, eps = 0, the mean of squares an exact power of four (an eighth of the row at
    2^(j+1), half at 2^(j-1), the rest at 2^j): the sum, the mean, rsqrt and both products are exact."""
    rng = np.random.default_rng(C)
    a = C // 8
    rows = []
    for j in (0, 3, -2):
        mag = np.concatenate([np.full(a, 2.0 ** (j + 1)), np.full(4 * a, 2.0 ** (j - 1)), np.full(C - 5 * a, 2.0 ** j)])
        rows.append(rng.permutation(mag) * rng.choice([-1.0, 1.0], C))
    x = np.array(rows, np.float32)
    assert [(r.astype(F64) ** 2).mean() for r in x] == [1.0, 64.0, 0.0625]
    got = run_rmsnorm(hip, dt, x, np.ones(C, np.float32), eps=0.0)
    np.testing.assert_array_equal(got, x / np.array([[1.0], [8.0], [0.25]], np.float32))


# --------------------------------------------------------------------------------------- llj_g_rope_kv
ROPE_CASES = [(2, 16, 3, 4, 8, [0, 1, 2, 3]), (78, 10, 2, 5, 16, [3, 4, 5, 6, 7]), (78, 2, 2, 1, 6, [20]),
              (6, 1, 1, 3, 8, [5, 1, 6])]  # hs, nh, B, T, S, pos: head 2; the 125M; a ring wrap; scattered positions
ROPE_IDS = ["head2", "125m", "wrap", "scattered"]


def synthetic_rope(n_pos, hs):
    """(cos, sin) pairs from {0, +-1, +-0.5, +-0.25}, no two positions of a pair and no two pairs of a
    position alike (index 13 p + 5 i modulo the 49 combinations; n_pos, hs / 2 <= 49)."""
    vals = np.array([0, 1, -1, 0.5, -0.5, 0.25, -0.25], np.float32)
    assert n_pos <= 49 and hs // 2 <= 49
    k = (13 * np.arange(n_pos)[:, None] + 5 * np.arange(hs // 2)[None, :]) % 49
    return np.stack([vals[k // 7], vals[k % 7]], -1)


def rope_ref(qkv, rope, pos, B, T_, nh, hs, S):
    """float64 restatement of O.apply_rope on the q and k thirds and of the cache write at slot pos % S.
    Returns (q, k cache, v cache, the written-slot mask) and for q / k cache the magnitudes |a c| + |b s|
    of the two products of each element; untouched cache slots hold the sentinel."""
    C = nh * hs
    x = qkv.astype(F64).reshape(B, T_, 3, nh, hs // 2, 2)
    r = rope.astype(F64)[np.asarray(pos)]
    c, s = r[None, :, None, :, 0], r[None, :, None, :, 1]

    def rot(a):
        return np.stack([a[..., 0] * c - a[..., 1] * s, a[..., 1] * c + a[..., 0] * s], -1).reshape(B, T_, nh, hs)

    def mag(a):
        a = np.abs(a)
        return np.stack([a[..., 0] * np.abs(c) + a[..., 1] * np.abs(s), a[..., 1] * np.abs(c) + a[..., 0] * np.abs(s)],
                        -1).reshape(B, T_, nh, hs)

    kc, vc = np.full((B, nh, S, hs), SENT, F64), np.full((B, nh, S, hs), SENT, F64)
    kmag, written = np.zeros((B, nh, S, hs)), np.zeros((B, nh, S, hs), bool)
    k, km, v = rot(x[:, :, 1]), mag(x[:, :, 1]), x[:, :, 2].reshape(B, T_, nh, hs)
    for t, p in enumerate(pos):
        kc[:, :, p % S], vc[:, :, p % S], kmag[:, :, p % S], written[:, :, p % S] = k[:, t], v[:, t], km[:, t], True
    return rot(x[:, :, 0]).reshape(B * T_, C), kc, vc, written, mag(x[:, :, 0]).reshape(B * T_, C), kmag


def run_rope_kv(hip, dt, qkv, rope, pos, B, T_, nh, hs, S):
    C = nh * hs
    q, kc, vc = filled((B * T_, C), dt), filled((B, nh, S, hs), dt), filled((B, nh, S, hs), dt)
    qd, rd, pd = D(qkv, dt), T(rope), T(np.asarray(pos, np.int32))
    call(hip, "llj_g_rope_kv", qd.data_ptr(), q.data_ptr(), kc.data_ptr(), vc.data_ptr(), rd.data_ptr(), pd.data_ptr(),
         B, T_, C, nh, S, dt, st())
    return H(q), H(kc), H(vc)


@DT
@pytest.mark.parametrize("hs,nh,B,T_,S,pos", ROPE_CASES, ids=ROPE_IDS)
def test_rope_kv_exact(hip, dt, hs, nh, B, T_, S, pos):
    """Integer qkv and a synthetic table of dyadic (cos, sin): every rotation is exact with or without
    contraction, so q and the WHOLE K and V caches are bitwise -- which slot of which (batch, head) was
    written, and that every other slot still holds the sentinel. V is a bit copy of the input third."""
    rng = np.random.default_rng(hs + S + pos[0])
    qkv = rng.integers(-8, 9, (B * T_, 3 * nh * hs)).astype(np.float32)
    rope = synthetic_rope(max(pos) + 1, hs)
    q, kc, vc, written, _, _ = rope_ref(qkv, rope, pos, B, T_, nh, hs, S)
    assert written.reshape(B * nh, S, hs).all(-1).sum(-1).tolist() == [T_] * (B * nh)
    gq, gk, gv = run_rope_kv(hip, dt, qkv, rope, pos, B, T_, nh, hs, S)
    np.testing.assert_array_equal(gq, rnd(q, dt))
    np.testing.assert_array_equal(gk, rnd(kc, dt))
    np.testing.assert_array_equal(gv, rnd(vc, dt))


@DT
@pytest.mark.parametrize("hs,nh,B,T_,S,pos", ROPE_CASES, ids=ROPE_IDS)
def test_rope_kv_real_table(hip, dt, hs, nh, B, T_, S, pos):
    """O.build_rope_cache and random qkv against the float64 rotation. fp32: |d| <= 2^-22 (|a c| + |b s|),
    the two products and the sum rounded once each (or one product exact, under an fma) with u = 2^-24.
    bf16: within 1 bf16 ulp of the rounded float64 value. V bitwise; untouched slots keep the sentinel."""
    rng = np.random.default_rng(hs + S + pos[0] + 1)
    qkv = rnd(rng.standard_normal((B * T_, 3 * nh * hs)), dt)
    rope = O.build_rope_cache(32, hs)
    q, kc, vc, written, qmag, kmag = rope_ref(qkv, rope, pos, B, T_, nh, hs, S)
    gq, gk, gv = run_rope_kv(hip, dt, qkv, rope, pos, B, T_, nh, hs, S)
    np.testing.assert_array_equal(gv, rnd(vc, dt))
    np.testing.assert_array_equal(gk[~written], np.float32(SENT))
    if dt == 1:
        assert (np.abs(gq - q) <= 2.0 ** -22 * qmag).all()
        assert (np.abs(gk - kc) <= 2.0 ** -22 * kmag).all()
    else:
        assert bf16_steps(gq, bf16(q)).max() <= 1
        assert bf16_steps(gk, bf16(kc)).max() <= 1


@pytest.mark.parametrize("C,nh", [(6, 2), (7, 2)], ids=["odd head", "C % n_head"])
def test_rope_kv_argument_rules(hip, C, nh):
    """An odd head size and C % n_head != 0: LLJ_EINVAL, nothing written."""
    bufs = [filled((2, 3 * C), 0, 1.0), filled((2, C), 0), filled((2, nh, 4, 4), 0), filled((2, nh, 4, 4), 0)]
    rope, pos = torch.ones(8, 4, 2, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    rc = hip.llj_g_rope_kv(*(b.data_ptr() for b in bufs), rope.data_ptr(), pos.data_ptr(), 2, 1, C, nh, 4, 0, st())
    assert rc == EINVAL
    for b in bufs[1:]:
        assert (H(b) == SENT).all()


# ------------------------------------------------------------------------------------- llj_g_attention
ATT_CASES = [(2, 16, 1, 4, 8, 0), (78, 2, 2, 1, 16, 15), (78, 2, 2, 1, 16, 16), (78, 2, 1, 1, 16, 37),
             (6, 1, 1, 1, 300, 299), (6, 1, 2, 3, 300, 255)]  # hs, nh, B, T, S, p0
ATT_IDS = ["head2-prefill", "last-before-wrap", "first-past-wrap", "wrapped", "300-keys", "around-256"]


def attn_ref(q, kc, vc, pos, S, T_, nh, hs, ft=F64, reverse=False):
    """tests/test_kernels_gpu.py's _attn_oracle in the float type ft: row m = b T + t at position pos[t]
    attends slots 0..p, or all S slots once p >= S. reverse: the keys taken in the opposite order."""
    q, kc, vc = q.astype(ft), kc.astype(ft), vc.astype(ft)
    y = np.zeros(q.shape, ft)
    for m in range(q.shape[0]):
        b, t = divmod(m, T_)
        slots = np.arange(min(int(pos[t]) + 1, S))
        slots = slots[::-1] if reverse else slots
        for h in range(nh):
            s = (kc[b, h, slots] @ q[m, h * hs:(h + 1) * hs]) * ft(1.0 / np.sqrt(hs))
            e = np.exp(s - s.max())
            y[m, h * hs:(h + 1) * hs] = (e / e.sum(dtype=ft)) @ vc[b, h, slots]
    assert y.dtype == ft
    return y


def run_attention(hip, dt, q, kc, vc, pos, B, T_, nh, hs, S):
    y = filled((B * T_, nh * hs), dt)
    qd, kd, vd, pd = D(q, dt), D(kc, dt), D(vc, dt), T(np.asarray(pos, np.int32))
    rc = hip.llj_g_attention(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), y.data_ptr(), pd.data_ptr(), B, T_, nh * hs,
                             nh, S, dt, st())
    return rc, H(y)


def head_rel(got, ref, nh, hs):
    """max over (row, head) of max |d| / max |ref| of that head's output vector."""
    d = np.abs(got.astype(F64) - ref).reshape(-1, nh, hs).max(-1)
    return float((d / np.abs(ref).reshape(-1, nh, hs).max(-1)).max())


@DT
@pytest.mark.parametrize("hs,nh,B,T_,S,p0", ATT_CASES, ids=ATT_IDS)
def test_attention_visible_set(hip, dt, hs, nh, B, T_, S, p0):
    """Which slots a row sees. q = 0, so every score is 0 and the output is the plain mean of the visible
    V rows; V carries an integer marker per slot (2^(j % 20) + j, j, ...; every sum below 2^24, so the fp32
    sum is exact) and the keys are random. With a power-of-two count of visible slots the division is
    exact too: bitwise. Otherwise 2 fp32 ulps (1 / l and the product round once each), on the bf16 path
    1 bf16 ulp. Slots past the last visible one hold NaN in K and V: reading one of them shows.
    Rows of T > 1 use positions that do not wrap, which is what the Python layer sends (a prompt is
    prefilled from position 0; past the ring's end the session decodes one token at a time)."""
    rng = np.random.default_rng(S + p0)
    pos = np.arange(p0, p0 + T_)
    assert T_ == 1 or pos[-1] < S
    j = np.arange(S)
    vc = np.zeros((B, nh, S, hs))
    vc[..., 0], vc[..., 1] = 2.0 ** (j % 20) + j, j
    for d in range(2, hs):
        vc[..., d] = (j * d + np.arange(B * nh).reshape(B, nh, 1)) % 7
    vc = rnd(vc, dt)  # bf16: the markers as the cache holds them (still integers, still distinct sums)
    kc = rnd(rng.standard_normal((B, nh, S, hs)), dt)
    if pos[-1] + 1 < S:
        kc[:, :, pos[-1] + 1:], vc[:, :, pos[-1] + 1:] = np.nan, np.nan
    rc, got = run_attention(hip, dt, np.zeros((B * T_, nh * hs)), kc, vc, pos, B, T_, nh, hs, S)
    assert rc == 0
    for m in range(B * T_):
        b, t = divmod(m, T_)
        nvis = min(int(pos[t]) + 1, S)
        tot = vc[b, :, :nvis].astype(F64).sum(1).reshape(-1)
        assert tot.max() < 2 ** 24
        want, row = tot / nvis, got[m]
        if nvis & (nvis - 1) == 0:
            np.testing.assert_array_equal(row, rnd(want, dt), err_msg=f"row {m} nvis {nvis}")
        elif dt == 1:
            assert (np.abs(row - want) <= 2 * np.spacing(np.abs(want).astype(np.float32))).all(), (m, nvis)
        else:
            assert bf16_steps(row, bf16(want)).max() <= 1, (m, nvis)


def attention_random(hip, dt, hs, nh, B, T_, S, p0, spread=None, what=""):
    rng = np.random.default_rng(hs + S + p0 + 1)
    pos = np.arange(p0, p0 + T_)
    q = rng.standard_normal((B * T_, nh * hs)) * 2
    kc, vc = rnd(rng.standard_normal((B, nh, S, hs)), dt), rnd(rng.standard_normal((B, nh, S, hs)), dt)
    if spread:  # the largest |score| of any (row, head, visible key) becomes `spread`
        smax = max(np.abs(kc[m // T_, h, :min(pos[m % T_] + 1, S)].astype(F64) @ q[m, h * hs:(h + 1) * hs]).max()
                   for m in range(B * T_) for h in range(nh)) / np.sqrt(hs)
        q *= spread / smax
    q = rnd(q, dt)
    ref = attn_ref(q, kc, vc, pos, S, T_, nh, hs)
    rc, got = run_attention(hip, dt, q, kc, vc, pos, B, T_, nh, hs, S)
    assert rc == 0
    if dt == 0:
        assert_bf16_close(got, ref, f"g_attention {what}")
        return
    noise = head_rel(attn_ref(q, kc, vc, pos, S, T_, nh, hs, ft=np.float32, reverse=True), ref, nh, hs)
    bound, err = max(4 * noise, 2.0 ** -20), head_rel(got, ref, nh, hs)
    print(f"[g_attention fp32 {what}] kernel err {err:.3e}, bound {bound:.3e} "
          f"(numpy float32, keys reversed: {noise:.3e})")
    assert err <= bound


@DT
@pytest.mark.parametrize("hs,nh,B,T_,S,p0", ATT_CASES, ids=ATT_IDS)
def test_attention_random_vs_float64(hip, dt, hs, nh, B, T_, S, p0):
    """Random q, K, V against float64 over the ring. bf16: one output rounding (assert_bf16_close's
    defaults). fp32: the kernel's __expf leaves no derivable bound, so the bound is 4 x the error of the
    same attention in numpy float32 with the keys in reversed order (the reference's own noise, computed
    here), floor 2^-20; the factor 4 is for the fast exponential. Measured: the module docstring."""
    attention_random(hip, dt, hs, nh, B, T_, S, p0, what=f"hs={hs} S={S} p0={p0} T={T_}")


@DT
@pytest.mark.parametrize("spread", [60, 120])
def test_attention_score_spread(hip, dt, spread):
    """q scaled until the scores reach +-60, and +-120: exp(120) is past fp32 (exp(60) is not), so a
    softmax that did not subtract the maximum gives inf / inf there."""
    attention_random(hip, dt, 78, 2, 2, 1, 16, 15, spread=spread, what=f"spread {spread}")


ATT_LDS_WORDS = 16 * 1024 - 4  # 64 KiB of LDS less the kernel's 4 static words: S + hs at the most


@pytest.mark.parametrize("words", [16 * 1024 + 1, ATT_LDS_WORDS + 1], ids=["16385", "16381"])
def test_attention_lds_guard(hip, words):
    """S + hs floats of scores and query beyond the LDS a launch may take: LLJ_EINVAL, y untouched
    (the buffers have their full size all the same)."""
    hs = 78
    S = words - hs
    kc = torch.zeros(1, 1, S, hs, device=dev)
    q, y, pos = torch.zeros(1, hs, device=dev), filled((1, hs), 1), torch.tensor([S - 1], dtype=torch.int32, device=dev)
    rc = hip.llj_g_attention(q.data_ptr(), kc.data_ptr(), kc.data_ptr(), y.data_ptr(), pos.data_ptr(), 1, 1, hs, 1, S,
                             1, st())
    assert rc == EINVAL
    assert (H(y) == SENT).all()


@DT
def test_attention_largest_accepted(hip, dt):
    """The largest accepted size: S + hs = 16380 floats (with the 4 static words exactly 64 KiB), one
    row at the last position, every slot visible."""
    attention_random(hip, dt, 78, 1, 1, 1, ATT_LDS_WORDS - 78, ATT_LDS_WORDS - 78 - 1, what="largest S")


# -------------------------------------------------------------------------------------- llj_g_silu_mul
SILU_N = [1, 255, 257, 780 * 9, 256 * 4096 + 7]  # the last: past the 4096-block grid cap (grid-stride loop)
SILU_EDGES = [-100.0, 100.0, 0.0, -0.0, 1e-3, -1e-3, 1.0, -1.0, 20.0, -20.0]


def silu_inputs(n, dt):
    rng = np.random.default_rng(n)
    a1, a2 = rng.standard_normal(n) * 3, rng.standard_normal(n)
    a1[:min(n, 10)] = SILU_EDGES[:n]
    return rnd(a1, dt), rnd(a2, dt)


def run_silu_mul(hip, dt, a1, a2, in_place=False):
    a1d, a2d = D(a1, dt), D(a2, dt)
    h = a1d if in_place else filled((a1.size + 3,), dt)
    call(hip, "llj_g_silu_mul", a1d.data_ptr(), a2d.data_ptr(), h.data_ptr(), a1.size, dt, st())
    got = H(h)
    if not in_place:
        assert (got[a1.size:] == SENT).all()
    return got[:a1.size]


@DT
@pytest.mark.parametrize("n", SILU_N)
def test_silu_mul_vs_float64(hip, dt, n):
    """silu(a1) * a2 against float64, a1 random and +-{0, 1e-3, 1, 20, 100}. At a1 = -100 expf(100)
    is inf: the result is a zero of either sign, not NaN. fp32: relative error <= 2^-21 (expf, the
    sum, the quotient and the product), plus 2^-126 absolute for results below the normal range (the
    float64 value -100 / (1 + e^100) is an fp32 subnormal, the kernel's 0). bf16: within 1 bf16 ulp of
    bf16(bf16(silu(a1)) * a2) and at most 1 % of the elements different."""
    a1, a2 = silu_inputs(n, dt)
    got = run_silu_mul(hip, dt, a1, a2)
    s64 = a1.astype(F64) / (1.0 + np.exp(-a1.astype(F64)))
    assert not np.isnan(got).any() and got[0] == 0.0  # a1[0] = -100
    if dt == 1:
        ref = s64 * a2.astype(F64)
        assert (np.abs(got - ref) <= 2.0 ** -21 * np.abs(ref) + 2.0 ** -126).all()
    else:
        steps = bf16_steps(got, bf16(bf16(s64).astype(F64) * a2.astype(F64)))
        print(f"[g_silu_mul bf16 n={n}] {np.count_nonzero(steps)} / {n} elements differ, max {steps.max()} ulp")
        assert steps.max() <= 1 and (steps != 0).mean() <= 0.01


@DT
def test_silu_mul_in_place(hip, dt):
    """h aliasing a1 (as LLaMA's any-shape MLP calls it): the same bits as into a buffer of its own."""
    a1, a2 = silu_inputs(780 * 9, dt)
    np.testing.assert_array_equal(run_silu_mul(hip, dt, a1, a2, in_place=True), run_silu_mul(hip, dt, a1, a2))


# ------------------------------------------------------------------- llj_g_argmax, llj_g_embedding
def run_argmax(hip, L, V, pos=4, stride=12, tokens=True):
    M = L.shape[0]
    Ld = T(np.ascontiguousarray(L, np.float32))
    out = torch.full((M,), -1, dtype=torch.int32, device=dev)
    toks = torch.full((M, stride), -1, dtype=torch.int32, device=dev)
    pd = torch.tensor([pos], dtype=torch.int32, device=dev)
    call(hip, "llj_g_argmax", Ld.data_ptr(), L.shape[1], M, V, out.data_ptr(), toks.data_ptr() if tokens else None,
         stride, pd.data_ptr() if tokens else None, st())
    torch.cuda.synchronize()
    return out.cpu().numpy(), toks.cpu().numpy()


@pytest.mark.parametrize("V", [5, 1024, 1025, 35000])
def test_argmax_ties_and_edges(hip, V):
    """fp32 rows of stride V + 3 whose padding holds a value above every logit. Exact ties: across two
    waves (the lower index in the higher wave where V allows it), inside one thread's stride (v and
    v + 1024) and between neighbours -- the lowest index wins; the maximum in the last column; a row of
    -inf (index 0) and a row of NaN (0, as the kernel documents). tokens_out: column pos + 1 only."""
    rng = np.random.default_rng(V)
    ties = [(1, 3)] + ([(3, 70), (5, 6)] if V > 70 else []) + ([(0, 1024)] if V > 1024 else []) + \
           ([(70, 1027), (2000, 2000 + 3 * 1024)] if V > 6000 else [])
    rows, want = [], []
    for lo, hi in ties:
        r = rng.standard_normal(V)
        r[lo] = r[hi] = 9.0
        rows.append(r), want.append(lo)
    r = rng.standard_normal(V)
    r[V - 1] = 9.0
    rows += [r, np.full(V, -np.inf), np.full(V, np.nan), rng.standard_normal(V)]
    want += [V - 1, 0, 0, int(np.argmax(rows[-1].astype(np.float32)))]
    for i in range(0, len(rows), 3):  # M = 3 rows a call (the last call may hold fewer)
        L = np.full((len(rows[i:i + 3]), V + 3), 1e30, np.float32)
        L[:, :V] = rows[i:i + 3]
        out, toks = run_argmax(hip, L, V)
        np.testing.assert_array_equal(out, want[i:i + 3])
        exp = np.full_like(toks, -1)
        exp[:, 5] = want[i:i + 3]
        np.testing.assert_array_equal(toks, exp)
    out, toks = run_argmax(hip, L, V, tokens=False)  # tokens_out NULL: the index alone
    np.testing.assert_array_equal(out, want[i:i + 3])
    assert (toks == -1).all()


@DT
@pytest.mark.parametrize("C", [2, 780])
def test_embedding_rows_and_pos_inc(hip, dt, C):
    """Rows of any width copied bit for bit (the last row, row 0, an index twice); *pos_inc bumped once a
    call whatever M is; NULL accepted. With C = 780 also llj_embedding, whose C % 8 != 0 kernel runs."""
    rng = np.random.default_rng(C)
    wte = rnd(rng.standard_normal((7, C)), dt)
    wd = D(wte, dt)
    fns = [("llj_g_embedding", (dt,))] + ([("llj_embedding", ())] if dt == 0 and C == 780 else [])
    for name, extra in fns:
        for idx in ([6, 0, 3, 3], [6]):
            for bump in (True, False):
                out, pos = filled((len(idx) + 1, C), dt), torch.tensor([7, -5], dtype=torch.int32, device=dev)
                idd = T(np.array(idx, np.int32))
                call(hip, name, idd.data_ptr(), wd.data_ptr(), out.data_ptr(), len(idx), C,
                     pos.data_ptr() if bump else None, *extra, st())
                got = H(out)
                np.testing.assert_array_equal(got[:-1], wte[idx])
                assert (got[-1] == SENT).all()
                assert pos.cpu().tolist() == [8 if bump else 7, -5]


# ---------------------------------------------------------------------------------------- llj_g_sample
SAMPLE_SETTINGS = [(0.8, 50), (1.0, 0), (0.5, 2), (1.3, 2048), (1.0, 5000)]  # the last: top_k > V
SAMPLE_U = [0.0, 0.5, 1.0 - 2.0 ** -24]
SAMPLE_SEED = 0


def sample_logits():
    """3 rows of 2048 fp32 logits; row 1 ties its 2nd with its 3rd and its 50th with its 51st largest
    (exact ties at the k-th value for top_k = 2 and 50: both are kept)."""
    L = (np.random.default_rng(SAMPLE_SEED).standard_normal((3, 2048)) * 2).astype(np.float32)
    order = np.argsort(-L[1])
    L[1, order[2]], L[1, order[50]] = L[1, order[1]], L[1, order[49]]
    return L


def sample_ref64(logits, temperature, top_k, u):
    """O.sample_inverse_cdf_fp32's keep set (fp32 x = logits / temperature, ties kept) with the softmax
    and the CDF in float64. Returns (index, distance of u to the nearest step of the normalised CDF)."""
    x = (logits.astype(np.float32) / np.float32(temperature)).astype(np.float32)
    V = x.shape[-1]
    k = V if top_k < 1 or top_k > V else top_k
    keep = x >= np.sort(x)[::-1][k - 1]
    cdf = np.cumsum(np.where(keep, np.exp((x - x.max()).astype(F64)), 0.0))
    cdf /= cdf[-1]
    hit = np.nonzero(cdf > float(np.float32(u)))[0]
    return (int(hit[0]) if hit.size else int(np.nonzero(keep)[0][-1])), float(np.abs(cdf - float(np.float32(u))).min())


def test_sample_fp32_vs_restatement(hip):
    """llj_g_sample at given uniforms against O.sample_inverse_cdf_fp32: 5 (temperature, top_k) settings
    x 3 rows (stride V + 8, the padding above every logit) x u in {0, 0.5, 1 - 2^-24} = 45 draws. The
    pick is the restatement's, unless u lies within 1e-6 of a step of the restatement's float64 CDF (the
    running sums are associated differently), which at most 1 draw may claim; the seed is one at which
    the restatement itself, fp32 CDF against float64 CDF, claims none (asserted here on the host)."""
    V, M = 2048, 3
    L = sample_logits()
    Lp = np.full((M, V + 8), 1e30, np.float32)
    Lp[:, :V] = L
    Ld, out = T(Lp), torch.full((M,), -1, dtype=torch.int32, device=dev)
    excused, draws = 0, 0
    for temperature, top_k in SAMPLE_SETTINGS:
        for u in SAMPLE_U:
            ud = T(np.full(M, u, np.float32))
            call(hip, "llj_g_sample", Ld.data_ptr(), V + 8, M, V, temperature, top_k, ud.data_ptr(), 0, out.data_ptr(),
                 None, 0, None, st())
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            for m in range(M):
                want, p = O.sample_inverse_cdf_fp32(L[m], temperature, top_k, u)
                want64, gap = sample_ref64(L[m], temperature, top_k, u)
                assert want == want64, "the restatement alone needs the exception: choose another seed"
                assert 0 <= got[m] < V and p[got[m]] > 0, "picked a filtered index"
                draws += 1
                if got[m] != want:
                    assert gap < 1e-6, (temperature, top_k, u, m, int(got[m]), want, gap)
                    excused += 1
    row1 = np.sort(L[1])[::-1]
    assert row1[1] == row1[2] and row1[49] == row1[50] and draws == 45
    assert excused <= 1, excused
