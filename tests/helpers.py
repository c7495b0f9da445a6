"""Shared test helpers: host-side statements of the device layouts and tolerance rules."""
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
