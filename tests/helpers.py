"""Shared test helpers: host-side statements of the device layouts and tolerance rules."""
import functools

import numpy as np

from oracle import llama_np as O


def w4p_pack_np(qw_logical: np.ndarray) -> np.ndarray:
    """Host restatement of the W4P layout (csrc/w4pack.hip) from the reference's logical
    (N, K/2) int4 byte array. Returns the packed bytes as uint8 (N*K/2,)."""
    N, Kh = qw_logical.shape
    K = 2 * Kh
    q = O.colblock_unpack_q(qw_logical, 4).astype(np.uint32)  # (N, K) codes
    KC = K // 128
    # index tiles: [nt][kc][lane][t] dwords; lane = 16*g + n_local; codes k = 128kc + 32g + 8t + j
    q = q.reshape(N // 16, 16, KC, 4, 4, 8)  # nt, n_local, kc, g, t, j
    bits = np.array([4 * (j >> 1) + 16 * (j & 1) for j in range(8)], np.uint32)
    d = (q << bits).sum(-1, dtype=np.uint64).astype(np.uint32)  # nt, n_local, kc, g, t
    d = d.transpose(0, 2, 3, 1, 4)  # nt, kc, g, n_local, t
    return np.ascontiguousarray(d).reshape(-1).view(np.uint8)


def w8p_pack_np(qw_logical: np.ndarray) -> np.ndarray:
    """Host restatement of the W8P layout (csrc/w4pack.hip) from the reference's logical (N, K)
    int8-code byte array (ColBlock bits=8): per (16-column tile, 128-k chunk) the W4P tile of
    the low nibbles, then the W4P tile of the high nibbles. Returns uint8 (N*K,)."""
    N, K = qw_logical.shape

    def as_w4_logical(nib):  # (N, K) nibbles -> the (N, K/2) int4 byte array of the same codes
        return (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8)

    lo = w4p_pack_np(as_w4_logical(qw_logical & 0xF)).reshape(-1, 1024)
    hi = w4p_pack_np(as_w4_logical(qw_logical >> 4)).reshape(-1, 1024)
    return np.ascontiguousarray(np.stack([lo, hi], 1)).reshape(-1)


def bf16(x):
    return O.bf16_round(np.asarray(x, np.float32))


def assert_bf16_close(got, ref, what="", rel=1.2e-2, abs_frac=4e-3):
    """bf16 outputs against an fp32 reference: per element |d| <= rel*|ref| + abs_frac*max|ref|
    (one bf16 rounding of the output is 2^-9 relative; accumulation-order noise is far below)."""
    got = np.asarray(got, np.float32)
    ref = np.asarray(ref, np.float32)
    scale = float(np.abs(ref).max()) or 1.0
    err = np.abs(got - ref)
    bound = rel * np.abs(ref) + abs_frac * scale
    bad = err > bound
    assert not bad.any(), f"{what}: {bad.sum()} / {bad.size} outside bf16 tolerance; max err {err.max():.4g} (scale {scale:.4g})"


# ------------------------------------------------------------------ exact operands
# Inputs for which every fp32 intermediate of a linear layer is exact in any summation order
# (tests/test_streaming_exact_gpu.py): small-integer activations, integer codes and zeros,
# power-of-two scales. The reference is then integer arithmetic and the tolerance zero.
SENTINEL = 0x7FA5  # bf16 bit pattern (a NaN payload) no kernel result takes


def f32_of_bits(b):
    return O.from_bf16_bits(np.asarray(b, np.uint16))


def exact_acts(rng, M, K, amax=4, density=1.0, phase=0):
    """(M, K) integers in [-amax, amax] as float32. density < 1: each row is nonzero (+-amax) on that
    share of the positions only, row m on the positions k = (m + phase) mod round(1 / density), so that
    the supports of round(1 / density) rows (or calls with successive phases) cover every k."""
    if density >= 1.0:
        return rng.integers(-amax, amax + 1, size=(M, K)).astype(np.float32)
    step = int(round(1.0 / density))
    a = np.zeros((M, K), np.float32)
    for m in range(M):
        k = np.arange((m + phase) % step, K, step)
        a[m, k] = amax * rng.choice([-1.0, 1.0], size=k.size)
    return a


def exact_weight(rng, wfmt, N, K, e_lo=3, e_hi=9):
    """Exact weight operands of format wfmt (0 int4, 1 bf16, 3 gptq.int8, 4 | (g / 128) << 8 grouped
    int4; flag bits above 16 ignored). Returns a dict: `W` the dequantized weight (N, K) float64, exact;
    `cmax` the largest magnitude the kernel's accumulator sees per unit of |a| (143 int4: 128 + q;
    2431 gptq.int8: 128 + lo + 2048 + 16 hi; max |w| bf16); `spread` the ratio of the largest possible
    |w| to the smallest scale within one output column (what one fp32 accumulator must span); and the
    buffers the device operands are made from (`qw`, `scales`, `zeros` or `wb`)."""
    wf = wfmt & 0xFF
    if wf == 1:
        e = rng.integers(e_lo - 3, e_hi - 2, size=(N, 1))  # 2^0 .. 2^-6 by default
        wi = rng.integers(-127, 128, size=(N, K))  # 7 bits and a sign: exact in bf16
        W = wi * 2.0 ** -e
        return dict(W=W, wb=W.astype(np.float32), cmax=float(np.abs(W).max()), spread=127.0, e=e[:, 0])
    bits = 8 if wf == 3 else 4
    G = 1
    if wf == 4:
        g = 128 * ((wfmt >> 8) & 0xFF)
        G = (K + g - 1) // g
    if bits == 4:
        qw = rng.integers(0, 256, size=(N, K // 2), dtype=np.uint8)
    else:
        qw = rng.integers(0, 256, size=(N, K), dtype=np.uint8)
    q = O.colblock_unpack_q(qw, bits).astype(np.int64)
    zeros = rng.integers(0, 1 << bits, size=(N, G)).astype(np.float32)
    scales = (2.0 ** -rng.integers(e_lo, e_hi + 1, size=(N, G))).astype(np.float32)
    if G == 1:
        zk, sk = zeros.astype(np.int64), scales.astype(np.float64)
    else:
        grp = np.arange(K) // g
        zk, sk = zeros.astype(np.int64)[:, grp], scales.astype(np.float64)[:, grp]
    W = (q - zk) * sk
    qmax = (1 << bits) - 1
    spread = float(qmax * (scales.max(1) / scales.min(1)).max()) if G > 1 else float(qmax)
    return dict(W=W, qw=qw, scales=scales, zeros=zeros, cmax=143.0 if bits == 4 else 2431.0, spread=spread)


def assert_exact_condition(a, w, what=""):
    """The issue's input condition, sum_k |a| * cmax < 2^24 per row, and for accumulators that mix scales
    (grouped int4) the same with the column's largest |w| over its smallest scale. Returns the margin
    2^24 / (the larger of the two figures)."""
    sa = float(np.abs(np.asarray(a, np.float64)).sum(1).max())
    worst = sa * max(w["cmax"], w["spread"])
    assert worst < 2.0 ** 24, f"{what}: sum|a| * cmax = {worst:.4g} >= 2^24"
    return 2.0 ** 24 / max(worst, 1.0)


def exact_linear(a, w):
    """y = a . W^T in float64 on integer / dyadic arrays (exact: every partial sum is below 2^53 units)."""
    return np.asarray(a, np.float64) @ w["W"].T


def inexact_share(y):
    """Share of the elements of the exact result that bf16 cannot hold (more than 8 significant bits)."""
    y = np.asarray(y, np.float64)
    return float(np.mean(bf16(y.astype(np.float32)).astype(np.float64) != y))


def rms_rstd_bf16(mean, eps=1e-5):
    """The fused RMSNorm's statistics chain on bf16 tensors (csrc/gemv_impl.h rms_rstd) from the mean of
    the squares: bf16(rsqrt(bf16(bf16(mean) + eps)))."""
    t = bf16(bf16(np.asarray(mean, np.float32)) + np.float32(eps))
    return bf16((1.0 / np.sqrt(t.astype(np.float64))).astype(np.float32))


def norm_rows(rng, M, K, gvals=(-4, -3, -2, -1, 0, 1, 2, 3, 4)):
    """Rows x[m, k] = +-c_m (c_m in 0.5, 1, 2) and an integer norm weight for which the fused RMSNorm is
    exact: rstd = 1 / c_m, so the MFMA operand is sign(x) * norm_w. Returns (x, norm_w, operand, c)."""
    c = np.array([0.5, 1.0, 2.0], np.float32)[np.arange(M) % 3]
    sign = rng.choice([-1.0, 1.0], size=(M, K)).astype(np.float32)
    x = sign * c[:, None]
    g = rng.choice(np.asarray(gvals, np.float32), size=K)
    r = rms_rstd_bf16((x.astype(np.float64) ** 2).mean(1))  # the exact mean is c^2
    assert np.array_equal(r, 1.0 / c), (r, c)
    xn = bf16(x * r[:, None])
    assert np.array_equal(xn, sign)
    return x, g, bf16(g[None, :] * xn), c


def dyadic_rope(rng, n_pos, hs):
    """A RoPE table (n_pos, hs / 2, 2) fp32 whose entries are multiples of 1 / 8 in [-1, 1]."""
    return (rng.integers(-8, 9, size=(n_pos, hs // 2, 2)) / 8.0).astype(np.float32)


def rope_bf16(v, cs, exact=True):
    """bf16(v * cos -+ partner * sin) on interleaved pairs (reference model.py:312-329): v (..., hs),
    cs (..., hs / 2, 2) broadcastable. Exact in fp32 for bf16 v and a dyadic table (asserted when `exact`)."""
    p = v.reshape(v.shape[:-1] + (v.shape[-1] // 2, 2)).astype(np.float64)
    c, s = cs[..., 0].astype(np.float64), cs[..., 1].astype(np.float64)
    o = np.stack([p[..., 0] * c - p[..., 1] * s, p[..., 1] * c + p[..., 0] * s], -1)
    o32 = o.astype(np.float32)
    assert not exact or np.array_equal(o32.astype(np.float64), o)
    return bf16(o32).reshape(v.shape)


def bf16_neighbours(s):
    """(lo, hi, nearest): the bf16 values around float64 s (lo <= s <= hi, equal when s is a bf16 value)
    and the round-to-nearest-even one, as float32."""
    s = np.asarray(s, np.float64)
    # the bf16 patterns as ordered integers (k and k + 1 are adjacent values, across binades and zero): the
    # truncation of float32(s) and its two neighbours bracket s whichever way the conversion rounded
    u = (s.astype(np.float32).view(np.uint32) >> 16).astype(np.int64)
    k = np.where(u & 0x8000, -(u & 0x7FFF), u & 0x7FFF)

    def value(k):
        bits = np.where(k < 0, 0x8000 | -k, k).astype(np.uint32) << 16
        return bits.astype(np.uint32).view(np.float32).astype(np.float64)

    cands = np.stack([value(k - 1), value(k), value(k + 1)])
    below = np.where(cands <= s, cands, -np.inf).max(0)
    above = np.where(cands >= s, cands, np.inf).min(0)
    assert np.isfinite(below).all() and np.isfinite(above).all()
    lo, hi = below.astype(np.float32), above.astype(np.float32)
    dl, dh = s - below, above - s
    even_lo = ((lo.view(np.uint32) >> 16) & 1) == 0
    near = np.where((dl < dh) | ((dl == dh) & even_lo), lo, hi)
    return lo, hi, near


def silu64(x):
    x = np.asarray(x, np.float64)
    return x / (1.0 + np.exp(-x))


def swiglu_candidates(y1, y2):
    """The SwiGLU rule for exact y1, y2 (float64): a1 = bf16(y1), a2 = bf16(y2), silu(a1) rounded to one of
    its two bf16 neighbours, the product rounded to bf16. Returns (cand_lo, cand_hi, cand_nearest, a1)."""
    a1, a2 = bf16(y1.astype(np.float32)), bf16(y2.astype(np.float32))
    lo, hi, near = bf16_neighbours(silu64(a1))
    return bf16(lo * a2), bf16(hi * a2), bf16(near * a2), a1


def exact_sum_mask(v, width=16):
    """For v (M, N) non-negative float32: per (row, group of `width` columns) whether the fp32 sum of the
    group is exact in any order (every element a multiple of one unit, the total below 2^24 units)."""
    M, N = v.shape
    t = v.reshape(M, N // width, width).astype(np.float64)
    m, e = np.frexp(t)
    low = np.where(t > 0, e - 24, 10000)  # float32 values: the lowest set bit is at or above e - 24
    mi = np.abs(m * 2.0 ** 24).astype(np.int64)
    tz = np.zeros_like(mi)
    for s in range(24):
        tz += ((mi & ((1 << (s + 1)) - 1)) == 0) & (mi != 0)
    unit = (low + tz).min(-1)
    return t.sum(-1) < np.ldexp(1.0, (unit + 24).clip(-1000, 1000))


# ------------------------------------------------------------------ exact epilogue operands
# The adapter v2 affine and the unmerged LoRA term on top of an exact Linear (tests/test_epilogue_exact_gpu.py,
# conditions checked on the CPU by tests/test_epilogue_exact_host.py): operands for which every fp32 sum and
# product between two bf16 roundings is exact, so each rounding point alone decides the bits.
def _col_mag(y):
    """Per column of the exact y (M, N): the power of two nearest the mean |y| (1 for a column of zeros)."""
    m = np.abs(np.asarray(y, np.float64)).mean(0)
    return np.where(m > 0, 2.0 ** np.rint(np.log2(np.where(m > 0, m, 1.0))), 1.0)


def _exact32(v64, what):
    v32 = v64.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), v64), f"{what}: {(v32.astype(np.float64) != v64).sum()} values are not exact in fp32"
    return v32


def exact_affine(rng, y):
    """(adapter_scale, adapter_bias) per column of the exact y (M, N), float32 holding bf16 values: scale =
    +-(odd integer) / 128 in [0.5, 1.5) (7 or 8 significant bits, never a power of two), bias = an integer in
    [-255, 255] times mag_n / 128 (mag_n: the power of two nearest the column's mean |y|), of the size of y's
    bf16 rounding step."""
    N = np.asarray(y).shape[1]
    scale = (2 * rng.integers(32, 96, size=N) + 1) / 128.0 * rng.choice([-1.0, 1.0], size=N)
    bias = rng.integers(-255, 256, size=N) * _col_mag(y) / 128.0
    scale, bias = scale.astype(np.float32), bias.astype(np.float32)
    assert np.array_equal(bf16(scale), scale) and np.array_equal(bf16(bias), bias)
    assert (np.abs(scale) >= 0.5).all() and (np.abs(scale) < 1.5).all()
    return scale, bias


def affine_bf16(y32, scale, bias, skip=None, parts=False):
    """The adapter v2 epilogue bf16(bf16(bf16(y) + bias) * scale) (adapter_v2.py:28-31 on bf16 tensors) in
    numpy float32. The fp32 sum and the fp32 product are asserted equal to their float64 values (no double
    rounding). skip: "y" / "sum" = that rounding left out (the wrong-rounding variants; nothing asserted); any
    other value, such as "none": every rounding kept, nothing asserted (vectors made for another y).
    parts: also return the fp32 product before its rounding."""
    y32 = np.asarray(y32, np.float32)
    s64, b64 = scale.astype(np.float64)[None, :], bias.astype(np.float64)[None, :]
    a = y32 if skip == "y" else bf16(y32)
    s = a.astype(np.float64) + b64
    s32 = _exact32(s, "affine sum") if skip is None else s.astype(np.float32)
    t = s32 if skip == "sum" else bf16(s32)
    p = t.astype(np.float64) * s64
    p32 = _exact32(p, "affine product") if skip is None else p.astype(np.float32)
    return (bf16(p32), p32) if parts else bf16(p32)


LORA_SCALING = 0.75  # lora_alpha 6 / r 8: not a power of two


def exact_lora(rng, y, M, r, n_en):
    """(t, B) for the exact y (M, n_en Ng) of the enabled groups' columns, in group order: t (M, r n_en) integers
    in [-8, 8]; B[n, j] (n_en Ng, r) = an integer in [-127, 127] times mag_n / 512. Every product is a multiple of
    mag_n / 512 and |sum| <= 8 * 127 * 64 units < 2^24: d is exact in fp32 in any fmaf order for r <= 64."""
    assert r <= 64 and np.asarray(y).shape == (M, np.asarray(y).shape[1]) and y.shape[1] % n_en == 0
    t = rng.integers(-8, 9, size=(M, r * n_en)).astype(np.float32)
    B = (rng.integers(-127, 128, size=(y.shape[1], r)) * (_col_mag(y) / 512.0)[:, None]).astype(np.float32)
    assert np.array_equal(bf16(B), B)
    return t, B


def lora_delta(t, B, r, n_en):
    """d[m, n] = sum_j t[m, g_i r + j] B[n, j] in float64 (exact), for the enabled groups' columns; asserted
    exact in fp32."""
    Ng = B.shape[0] // n_en
    d = np.concatenate([t[:, gi * r:(gi + 1) * r].astype(np.float64) @ B[gi * Ng:(gi + 1) * Ng].astype(np.float64).T
                        for gi in range(n_en)], 1)
    _exact32(d, "LoRA d")
    return d


def lora_bf16(y32, d, scaling, enabled_cols, skip=None):
    """The unmerged LoRA epilogue y = bf16(bf16(y) + bf16(bf16(d) * scaling)) on the columns `enabled_cols`
    (lora.py:318-323 on bf16 tensors), bf16(y) elsewhere, in numpy float32; d (M, len(enabled_cols)) float64.
    Product and sum are asserted exact in fp32. skip: "y" / "d" / "ds" = that rounding left out."""
    y32 = np.asarray(y32, np.float32)
    out = bf16(y32)
    yb = (y32 if skip == "y" else out)[:, enabled_cols].astype(np.float64)
    d32 = d.astype(np.float32)
    db = d32 if skip == "d" else bf16(d32)
    ds = db.astype(np.float64) * scaling
    ds32 = _exact32(ds, "LoRA d * scaling") if skip is None else ds.astype(np.float32)
    dsb = ds32 if skip == "ds" else bf16(ds32)
    s = yb + dsb.astype(np.float64)
    s32 = _exact32(s, "LoRA sum") if skip is None else s.astype(np.float32)
    out = out.copy()
    out[:, enabled_cols] = bf16(s32)
    return out


class RoundingPower:
    """Test power over the cases of one test, from the references alone: the share of the pooled expected
    elements in which each wrong-rounding variant differs from the right result (floor 10 %), and the share in
    which the right result differs from the base expectation without the affine / the term (floor 99 %)."""

    def __init__(self):
        self.d, self.noop, self.extra = {}, [], {}

    def require(self, name, arr, floor):
        """A further input condition of the test: the mean of the pooled `arr` must exceed `floor`."""
        self.extra.setdefault(name, ([], floor))[0].append(np.asarray(arr).ravel())

    def extras(self):
        return {k: (float(np.mean(np.concatenate(v))), fl) for k, (v, fl) in self.extra.items()}

    def add(self, want, wrong, base=None, count=True):
        """count False: the case adds to the no-op share only (a shape outside the pool, K < 640)."""
        if count:
            for k, v in wrong.items():
                self.d.setdefault(k, []).append((np.asarray(v) != want).ravel())
        if base is not None:
            self.noop.append((np.asarray(base) != want).ravel())

    def shares(self):
        return {k: float(np.mean(np.concatenate(v))) for k, v in self.d.items()}

    def changed(self):
        return float(np.mean(np.concatenate(self.noop))) if self.noop else None

    def ok(self, exempt=()):
        ch = self.changed()
        return (all(s >= 0.10 for k, s in self.shares().items() if k not in exempt) and (ch is None or ch >= 0.99)
                and all(v > fl for v, fl in self.extras().values()))

    def finish(self, what, exempt=(), seed=None):
        s, ch = self.shares(), self.changed()
        print(f"{what}: wrong-rounding shares " + ", ".join(f"{k} {v:.3f}" for k, v in s.items())
              + (f"; exempt {tuple(exempt)}" if exempt else "") + (f"; differs from the base in {ch:.4f}" if ch is not None else "")
              + "".join(f"; {k} {v:.3f}" for k, (v, fl) in self.extras().items())
              + (f"; seed {seed}" if seed is not None else ""))
        for k, (v, fl) in self.extras().items():
            assert v > fl, f"{what}: {k} is {v:.4f}, not above {fl}"
        for k, v in s.items():
            assert k in exempt or v >= 0.10, f"{what}: variant {k} differs in only {v:.4f} of the elements"
        assert ch is None or ch >= 0.99, f"{what}: the epilogue changes only {ch:.4f} of the elements"
        return s


# ------------------------------------------------------------------ exact LLM.int8 operands
# Inputs for which the LLM.int8 kernels (wfmt 2) have one correct bit pattern (tests/test_int8_exact_gpu.py):
# with SCA = 127 * 2^-j and SCB = 127 * 2^-e the fp32 dequantization constant SCA * SCB / 127^2 is exactly
# 2^-(j + e) however it is associated, 127 / SCA = 2^j, SCB / 127 = 2^-e, so acc * const is exact in fp32
# while |acc| < 2^24 and both fp16 roundings and the bf16 one are decided by the reference alone.
I8_THR = 6.0
I8_SUB = {5: 15, 6: 7, 14: 0}  # largest sub-threshold entry of an outlier column, in quarters, per SCA class


def f16_bits(x):
    return np.asarray(x).astype(np.float16).view(np.uint16)


def _dyadic_unit(v):
    """Per row of v (float64, dyadic): the largest power of two that every entry is a multiple of (1 for a
    row of zeros)."""
    u = np.ones(v.shape[0])
    for p in range(1, 40):
        frac = v * 2.0 ** (p - 1)
        u = np.where((frac != np.rint(frac)).any(1), 2.0 ** -p, u)
    return u


def i8_reference(a, cb, e, thr=I8_THR, mutate=None):
    """LLM.int8 of activations a (M, K) on codes cb (N, K) int8 and SCB[n] = 127 * 2^-e[n], in integers and
    float64: outlier set O = columns with any |a| >= thr, SCA[m] = max |a| over the elements below thr (which
    must be 127 * 2^-j or 0), codes = rint-even(a * 127 / SCA) with O zeroed, main16 = f16(acc * 2^-(j + e)),
    side = sum_{k in O} a CB 2^-e, y16 = f16(main16 + side). Asserts the conditions under which a correct
    kernel has exactly these bits. mutate: None, or the wrong reference "inner" / "outer" (that fp16 rounding
    dropped), "dropcol" (the last outlier column left out of the side product), "halfaway" (code ties rounded
    away from zero). Returns a dict; `y16` float32 (fp16 values; "outer": not rounded to fp16)."""
    f32, f64 = np.float32, np.float64
    a = np.asarray(a, f32)
    assert np.array_equal(bf16(a), a) and np.array_equal(a.astype(np.float16).astype(f32), a), "a: not bf16 and fp16 values"
    a64, cb64, e = a.astype(f64), np.asarray(cb, f64), np.asarray(e)
    big = np.abs(a64) >= thr
    O = big.any(0)
    sca = np.where(big, 0.0, np.abs(a64)).max(1)
    mant, ex = np.frexp(sca)
    assert np.all((sca == 0) | (mant == 127.0 / 128)), f"SCA is not 127 * 2^-j: {sca}"
    j = np.where(sca > 0, 7 - ex, 0)
    inv = np.where(sca > 0, 2.0 ** j, 0.0)
    # the fp32 constants the kernels form, in each association
    sa32, scb32, kq = sca.astype(f32)[:, None], (127.0 * 2.0 ** -e).astype(f32)[None, :], f32(1.0) / (f32(127.0) * f32(127.0))
    const = np.where(sca > 0, 2.0 ** -j, 0.0)[:, None] * 2.0 ** -e[None, :]
    assert np.array_equal(scb32.astype(f64), 127.0 * 2.0 ** -e[None, :])
    for got in ((sa32 * scb32) * kq, sa32 * (scb32 * kq), (sa32 * scb32) / f32(16129.0)):
        assert got.dtype == f32 and np.array_equal(got.astype(f64), const), "the dequantization constant is not 2^-(j + e)"
    assert np.array_equal((f32(127.0) / np.where(sca > 0, sca, 1.0).astype(f32)).astype(f64), np.where(sca > 0, inv, 127.0))
    assert np.array_equal((scb32 / f32(127.0)).astype(f64), 2.0 ** -e[None, :])
    x = a64 * inv[:, None]
    codes = np.sign(x) * np.floor(np.abs(x) + 0.5) if mutate == "halfaway" else np.rint(x)
    codes[:, O] = 0
    assert np.abs(codes).max(initial=0) <= 127
    acc = codes @ cb64.T
    assert np.abs(acc).max() < 2.0 ** 24, f"|acc| = {np.abs(acc).max()} >= 2^24"
    main = acc * const
    main16 = main.astype(np.float16).astype(f64)
    cols = np.nonzero(O)[0]
    if mutate == "dropcol":
        cols = cols[:-1]
    w = cb64 * 2.0 ** -e[:, None]
    assert np.array_equal(w.astype(np.float16).astype(f64), w)
    ao = a64[:, cols]
    side = ao @ w[:, cols].T
    unit = _dyadic_unit(ao)
    worst = ((np.abs(ao) / unit[:, None]) @ np.abs(cb64[:, cols]).T).max(initial=0)
    assert worst < 2.0 ** 24, f"side product: sum |a| |CB| = {worst} units >= 2^24"
    if mutate == "inner":
        s32 = (main.astype(f32) + side.astype(f32)).astype(f32)
    else:
        s32 = (main16 + side).astype(f32)
        assert np.array_equal(s32.astype(f64), main16 + side), "main16 + side is not exact in fp32"
    y16 = s32 if mutate == "outer" else s32.astype(np.float16).astype(f32)
    assert np.abs(s32).max() < 65504.0
    return dict(O=O, cols=np.nonzero(O)[0], sca=sca.astype(f32), j=j, codes=codes.astype(np.int8), acc=acc, main=main,
                side=side, y16=y16)


def i8_exact_case(M, N, K, ocols, j_rows, seed, hot=None, rowmax_in_outlier=False, e_lo=3, e_hi=9, mutants=True,
                  wseed=0):
    """Exact LLM.int8 operands. Row m has SCA class j_rows[m] in {5, 6, 14} (SCA = 127 * 2^-j; 14: below 1 / 64,
    the GEMV's quant8f rule): elements n * 2^-(j + 1), |n| <= 254 (bf16 values; about half the codes are ties,
    which pins round-to-nearest-even), one element +-127 * 2^-j off the outlier columns. Outlier columns
    `ocols`: one or two rows (`hot`: a list of row lists per column; never a class-14 row) hold +-6 (the
    threshold itself), +-8 or +-12, the others sub-threshold multiples of 1 / 4 no larger than their SCA (0 in a
    class-14 row: its main term reaches down to 2^-23, which no fp32 sum with a side term holds exactly).
    rowmax_in_outlier: a row's only +-127 * 2^-j sits in the first outlier column, below the threshold, where
    another row sets the outlier, and the rest of that row stays strictly below it (asserted; `rowmax_row` names
    the row): that element alone decides SCA, and its code is zeroed. CB: int8 over -127 .. 127;
    SCB[n] = 127 * 2^-e, e in e_lo .. e_hi (drawn from (N, K, seed, wseed) only: the activations do not depend on
    N or wseed). Returns the operands, i8_reference's fields and, with `mutants`,
    `wrong`: the y16 of each wrong reference."""
    rng = np.random.default_rng([61, M, K, len(ocols), seed])
    j = np.asarray(j_rows, np.int64)
    assert j.shape == (M,) and set(j.tolist()) <= set(I8_SUB)
    ocols = np.unique(np.asarray(ocols, np.int64))
    assert ocols.size == 0 or (0 <= ocols[0] and ocols[-1] < K)
    free = np.setdiff1d(np.arange(K), ocols)
    a = rng.integers(-254, 255, size=(M, K)) * 2.0 ** -(j + 1)[:, None]
    kmax = rng.choice(free, M)
    a[np.arange(M), kmax] = 127 * 2.0 ** -j * rng.choice([-1.0, 1.0], M)
    setters = np.nonzero(j != 14)[0]
    assert ocols.size == 0 or setters.size, "outlier columns need a row of class 5 or 6 to set them"
    lim = np.array([I8_SUB[v] for v in j.tolist()])
    hots = []
    for i, c in enumerate(ocols):
        a[:, c] = rng.integers(-lim, lim + 1) / 4.0
        nh = 1 if (rowmax_in_outlier and i == 0) else min(setters.size, int(rng.integers(1, 3)))
        h = np.asarray(hot[i]) if hot is not None else rng.choice(setters, nh, replace=False)
        a[h, c] = rng.choice([6.0, -6.0, 8.0, -8.0, 12.0, -12.0], h.size)
        hots.append(h)
    rowmax_row = None
    if rowmax_in_outlier:
        # every other element of that row stays strictly below the maximum (|n| <= 253; |n| = 254 is 127 * 2^-j
        # too), so the element inside the outlier column alone decides the row's SCA
        r = rowmax_row = [m for m in setters if m not in hots[0]][0]
        top = 127 * 2.0 ** -j[r]
        a[r, free] = np.where(np.abs(a[r, free]) >= top, np.sign(a[r, free]) * 253 * 2.0 ** -(j[r] + 1), a[r, free])
        a[r, ocols[0]] = top * rng.choice([-1.0, 1.0])
        inside = np.abs(a[r, ocols])
        assert inside[inside < I8_THR].max() == top > np.abs(a[r, free]).max(), "the row maximum is not inside O alone"
    a = a.astype(np.float32)
    rng = np.random.default_rng([62, N, K, seed, wseed])
    cb = rng.integers(-127, 128, size=(N, K)).astype(np.int8)
    e = rng.integers(e_lo, e_hi + 1, size=N)
    c = dict(a=a, cb=cb, e=e, scb=(127.0 * 2.0 ** -e).astype(np.float32), M=M, N=N, K=K, rowmax_row=rowmax_row)
    c.update(i8_reference(a, cb, e))
    assert np.array_equal(c["cols"], ocols) and np.array_equal(c["j"], j)
    if mutants:
        c["wrong"] = {m: i8_reference(a, cb, e, mutate=m)["y16"] for m in ("inner", "outer", "halfaway")
                      + (("dropcol",) if ocols.size else ())}
    return c


class I8Power:
    """Test power over the cases of one test, from the references alone: the share of the pooled bf16 (or, dt 1,
    fp16) outputs in which each wrong reference differs from the right one. The floors: a dropped fp16 rounding
    >= 1 % and >= 8 elements (fp16 output, inner: >= 10 %), a dropped outlier column or ties rounded half away
    >= 50 %. The fp16 roundings and the dropped column count over the cases with outlier columns only
    (without a side term the two fp16 roundings are one)."""

    def __init__(self, out=bf16):
        self.out, self.d = out, {}

    def add(self, c):
        right = self.out(c["y16"])
        for m, y in c["wrong"].items():
            if m in ("inner", "outer") and not c["cols"].size:
                continue
            self.d.setdefault(m, []).append((self.out(y) != right).ravel())

    def shares(self):
        return {m: (float(np.mean(np.concatenate(v))), int(np.sum(np.concatenate(v)))) for m, v in self.d.items()}

    def finish(self, what, need=("inner", "outer", "dropcol", "halfaway")):
        s = self.shares()
        print(f"{what}: wrong-reference shares " + ", ".join(f"{m} {s[m][0]:.3f} ({s[m][1]})" for m in s))
        for m in need:
            share, n = s[m]
            if m in ("inner", "outer"):
                floor = 0.10 if (m == "inner" and self.out is not bf16) else 0.01
                assert share >= floor and n >= 8, f"{what}: {m} fp16 rounding dropped differs in {share:.4f} ({n} elements)"
            else:
                assert share >= 0.5, f"{what}: {m} differs in only {share:.4f}"
        return s


# The input families of tests/test_int8_exact_gpu.py (tests/test_int8_exact_host.py checks every one against
# the oracle on the CPU). GEMV side-product regimes: name -> (K, outlier columns); each is the smallest shape
# that reaches the code named (csrc/gemv_impl.h).
def _i8_gemv_layouts():
    rng = np.random.default_rng(77)
    pick = lambda lo, width, n: sorted((lo + rng.choice(width, n, replace=False)).tolist())  # noqa: E731
    ins = [0, 127, 128 + 15, 256 + 16, 256 + 63, 640 + 64, 3072 + 63, 3072 + 127]
    walk = [3, 16 + 2, 64 + 16 + 5, 32 + 0, 32 + 15, 64 + 32 + 7, 64 + 48 + 9]  # lane groups 0..3: 1, 2, 3, 1 columns
    return {
        "none": (128, []),
        # K = 3200: k-block width 128 = the chunk, so the side product runs inside the weight stream from the
        # one-launch prep's aval table: 0, 1 and 2 columns per chunk, the first and the last chunk
        "instream": (3200, ins),
        "instream_over": (3200, ins + [896 + 1, 896 + 40, 896 + 100]),  # a chunk with 3: after the stream
        # one k-block of 32 with exactly SPC = 8 columns (4 waves: the fast path), then 9 (the general list walk)
        "spc8": (128, pick(32, 32, 8)),
        "spc9": (128, pick(32, 32, 9)),
        # K = 8192: 8-wave residual form, SPC = 32 of a k-block of 256
        "spc32w8": (8192, pick(768, 256, 32)),
        "spc33w8": (8192, pick(768, 256, 33)),
        # one full kSideChunk = 256 round, one entry into the second, 300
        "rounds256": (640, pick(0, 640, 256)),
        "rounds257": (640, pick(0, 640, 257)),
        "rounds300": (640, pick(0, 640, 300)),
        # AM_I8Q's walk over the weight registers: lane group g holds k = 64 t + 16 g + 0..15 of a chunk; groups
        # with 1, 2 and 3 columns (two per trip plus an odd one), every group, both MFMA steps t; 32 in a chunk
        "walk128": (128, walk),
        "walk128x32": (128, pick(0, 128, 32)),
        "walk640": (640, [walk[0]] + [128 + k for k in walk[1:3]] + [256 + k for k in walk[3:6]] + [384 + walk[6]]
                    + pick(512, 128, 32)),
    }


I8_GEMV_LAYOUTS = _i8_gemv_layouts()
I8_ROW_CLASSES = (5, 6, 14, 5, 6, 5, 6, 5)


def i8_rows(M, with14=True):
    """SCA classes of M rows: 5 and 6 alternating, every eighth row from the third on 14 (M >= 3)."""
    if M <= 2 or not with14:
        return tuple(np.resize((5, 6), M).tolist())
    return tuple(np.resize(I8_ROW_CLASSES, M).tolist())


@functools.lru_cache(maxsize=None)
def i8_gemv_case(layout, M, N, seed=0, e_lo=3, e_hi=9, wseed=0, with14=True):
    K, ocols = I8_GEMV_LAYOUTS[layout]
    return i8_exact_case(M, N, K, ocols, i8_rows(M, with14), seed, rowmax_in_outlier=M > 1 and len(ocols) > 0, e_lo=e_lo,
                         e_hi=e_hi, wseed=wseed)


@functools.lru_cache(maxsize=None)
def i8_quant8f_case(M, N, K):
    """Rows of class 14 only (SCA < 1 / 64 in every row), no outlier columns."""
    return i8_exact_case(M, N, K, [], (14,) * M, 3)


# the prefill GEMM: (outlier columns, gather capacity kpad or None); the last outlier column of a case is set by
# one row alone (i8_gemm_case)
I8_GEMM_SIDES = [(0, None), (3, None), (32, None), (33, None), (70, None), (70, 128), (64, 64), (70, 64), (3, 64)]


@functools.lru_cache(maxsize=None)
def i8_gemm_case(M, N, K, ncols, wseed=0, e_lo=3, e_hi=9):
    rng = np.random.default_rng([78, M, K, ncols])
    ocols = np.sort(rng.choice(K, ncols, replace=False))
    rows = np.array(i8_rows(M))
    setters = np.nonzero(rows != 14)[0]
    hot = [rng.choice(setters, int(rng.integers(1, 3)), replace=False) for _ in range(ncols)]
    if ncols:
        hot[-1] = setters[-1:]  # an outlier column that a single row sets
    return i8_exact_case(M, N, K, ocols, rows, 0, hot=hot, rowmax_in_outlier=ncols > 0, wseed=wseed, e_lo=e_lo, e_hi=e_hi)


I8_GENERIC_SHAPES = [(1, 20, 6, 2), (7, 780, 36, 30), (40, 132, 10, 5)]  # (M, K, N, outlier columns)


@functools.lru_cache(maxsize=None)
def i8_generic_case(M, K, N, ncols):
    rng = np.random.default_rng([79, M, K, N])
    return i8_exact_case(M, N, K, rng.choice(K, ncols, replace=False), i8_rows(M), 0, rowmax_in_outlier=M > 1)


def i8_zero_row_case(M, N, K):
    """A case whose last row is all zero (SCA 0: codes 0, output 0) -- alone at M = 1 -- next to rows with outliers."""
    c = i8_exact_case(max(M, 2), N, K, [7, 90], i8_rows(max(M, 2), False), 9, hot=[[0], [0]], mutants=False)
    a = c["a"][:M].copy()
    a[M - 1] = 0.0
    c = dict(c, a=a, M=M, rowmax_row=None)
    c.update(i8_reference(a, c["cb"], c["e"]))
    assert c["sca"][M - 1] == 0 and not c["y16"][M - 1].any()
    return c


def i8_has_rowmax(cases):
    """At least one of a test's cases has a row whose SCA is decided inside an outlier column another row sets."""
    return any(c["rowmax_row"] is not None for c in cases)
