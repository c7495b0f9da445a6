"""llj_nll (bf16 logits) and llj_g_nll (fp32 logits) through the C ABI against a float64 numpy
`logsumexp - gather` of the same stored logits (GPU only).

Tolerance: the bound the kernel was specified with, |row_nll - ref| <= (V / 256 + 32) * 2^-23 + 2^-22 * |ref|, which the kernel's
summation structure (csrc/nll.hip) fits, so it is not restated or tuned. The structure: 256 threads, each
summing its V / 256 exp terms chunk by chunk (16-byte chunks: 8 bf16 or 4 fp32 columns; per chunk its terms,
one add into the running sum and at most one rescale of it), then 6 butterfly merges inside a wave and 3
merges across the 4 waves. Relative to the sum S (all terms positive, every partial sum <= S), for the
4-column chunks, the worse case: each exp term is within 2^-23 (1 ulp of expf; the rounding of x - max
changes a term by d * 2^-24 * exp(-d) of S at most); the V / 256 + V / 1024 adds give (V / 512) * 1.25 *
2^-23; each of the at most V / 1024 rescales is one expf and one rounding, 1.5 * 2^-23; each of the 9 merges
two factors, two products and an add, 2 * 2^-23. Together
    |dS / S| <= (1 + V * 1.25 / 512 + V * 1.5 / 1024 + 18) * 2^-23 = (V / 256 + 19) * 2^-23,
which carries over to log S as an absolute error. logf and the rounding of the final subtraction are within
2^-22 * |ref|; the rounding of lse = max + log S, 2^-24 * |lse| <= 2^-24 * (|ref| + |x_t|), takes the
remaining 13 * 2^-23 as long as the target's own logit is below 26 in magnitude, which holds for the N(0, 4^2)
logits here (the row with the +-80 entries keeps its target off those two columns).

total[0] is a double sum of floats in a fixed order: against numpy's float64 sum of the kernel's own
row_nll it must agree within M * 2^-50 relative.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"

# (M, V, ldl, element offset of the base pointer)
SHAPES = [
    (1, 2048, 2048, 0),
    (3, 2048, 2048, 0),
    (130, 2048, 2048, 0),   # `total` over more rows than one 64-row chunk
    (2, 32000, 32000, 0),
    (2, 32000, 32064, 0),
    (5, 2047, 2051, 1),     # no row 16-byte aligned: the element path
    (2, 7, 7, 0),           # fewer columns than threads
    (12, 1003, 1008, 0),    # aligned rows whose V is no multiple of the 16-byte chunk: the tail columns
    (12, 1003, 1003, 1),    # the element path with every special row
    (300, 40, 40, 0),       # `total`: more rows than its 256 threads, so a thread adds two rows in order
]
# special rows, given to rows 1, 2, ... as far as M allows (row 0 stays a plain normal row)
SPECIALS = ["neginf_block", "nan_logit", "ignored", "target_is_V", "all_equal", "pm80", "target_0", "target_last",
            "target_argmax", "ignored"]


def st():
    return torch.cuda.current_stream().cuda_stream


def make_case(M, V, seed):
    """(fp32 logits (M, V), int32 targets (M,), names of the special rows)."""
    rng = np.random.default_rng(seed)
    x = (4.0 * rng.standard_normal((M, V))).astype(np.float32)
    t = rng.integers(0, V, M).astype(np.int32)
    names = {}
    for m, what in zip(range(1, M), SPECIALS):
        names[m] = what
        if what == "neginf_block":
            nb = min(256, V // 2)
            x[m, :nb] = -np.inf
            t[m] = nb + (t[m] % (V - nb))
        elif what == "nan_logit":
            x[m, (7 * m) % V] = np.nan
        elif what == "ignored":
            t[m] = -1
        elif what == "target_is_V":
            t[m] = V
        elif what == "all_equal":
            x[m] = 1.25
        elif what == "pm80":
            x[m, 1 % V], x[m, V - 2] = 80.0, -80.0
            if t[m] in (1 % V, V - 2):
                t[m] = 0
        elif what == "target_0":
            t[m] = 0
        elif what == "target_last":
            t[m] = V - 1
        elif what == "target_argmax":
            t[m] = int(x[m].argmax())
    return x, t, names


def reference(stored: np.ndarray, t: np.ndarray):
    """float64 row NLL of the stored logits (0 for an ignored row, NaN for a target outside the row)."""
    M, V = stored.shape
    ref = np.zeros(M)
    with np.errstate(invalid="ignore", divide="ignore"):
        for m in range(M):
            if t[m] < 0:
                continue
            if t[m] >= V:
                ref[m] = np.nan
                continue
            row = stored[m].astype(np.float64)
            mx = np.max(row[np.isfinite(row)]) if np.isfinite(row).any() else 0.0
            lse = mx + np.log(np.exp(row - mx).sum())
            ref[m] = lse - row[t[m]]
    return ref


def device_logits(x, ldl, off, dtype):
    """The logits in a NaN-filled buffer of row stride ldl starting `off` elements in: (buffer, data_ptr,
    float64 copy of what is stored)."""
    M, V = x.shape
    buf = torch.full((off + M * ldl + 8,), float("nan"), dtype=dtype, device=dev)
    view = buf[off:off + M * ldl].view(M, ldl)
    view[:, :V] = torch.from_numpy(x).to(dev).to(dtype)
    stored = view[:, :V].float().cpu().numpy().astype(np.float64)
    return buf, view.data_ptr(), stored


def run(hip, name, ptr, ldl, M, V, t_dev, total):
    out = torch.full((M,), 123.0, dtype=torch.float32, device=dev)
    rc = getattr(hip, name)(ptr, ldl, M, V, t_dev.data_ptr(), out.data_ptr(), None if total is None else total.data_ptr(),
                            st())
    assert rc == 0, f"{name} returned {rc}"
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("M,V,ldl,off", SHAPES)
def test_row_nll_and_total(hip, dtype, M, V, ldl, off):
    name = "llj_nll" if dtype == torch.bfloat16 else "llj_g_nll"
    x, t, names = make_case(M, V, seed=M * 100003 + V + ldl)
    buf, ptr, stored = device_logits(x, ldl, off, dtype)
    assert (ptr % 16 == 0) == (off == 0)
    ref = reference(stored, t)
    t_dev = torch.from_numpy(t).to(dev)

    # ---- every row, total = NULL; columns V..ldl (and the buffer around the rows) are NaN: never read
    got = run(hip, name, ptr, ldl, M, V, t_dev, None)
    again = run(hip, name, ptr, ldl, M, V, t_dev, None)
    assert np.array_equal(got.view(np.int32), again.view(np.int32)), "row_nll differs between two runs"
    nan_rows = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan_rows), (names, np.flatnonzero(np.isnan(got)), np.flatnonzero(nan_rows))
    for m, what in names.items():
        assert nan_rows[m] == (what in ("nan_logit", "target_is_V")), (m, what)
        if what == "ignored":
            assert got[m] == 0.0
        if what == "all_equal":
            assert abs(ref[m] - np.log(V)) < 1e-12
    ok = ~nan_rows
    err = np.abs(got[ok].astype(np.float64) - ref[ok])
    bound = (V / 256 + 32) * 2.0 ** -23 + 2.0 ** -22 * np.abs(ref[ok])
    worst = int(np.argmax(err / bound))
    print(f"[nll] {name} M={M} V={V} ldl={ldl} off={off}: max |err| {err.max():.3e} "
          f"(largest err / bound {err[worst] / bound[worst]:.3f})")
    assert (err <= bound).all(), (np.flatnonzero(ok)[worst], err[worst], bound[worst])

    # ---- totals: the rows that are NaN by construction ignored, so the sum is finite; two calls accumulate
    t2 = t.copy()
    t2[nan_rows] = -1
    t2_dev = torch.from_numpy(t2).to(dev)
    counted = int((t2 >= 0).sum())
    total = torch.zeros(2, dtype=torch.float64, device=dev)
    rows = run(hip, name, ptr, ldl, M, V, t2_dev, total)
    first = total.cpu().numpy().copy()
    assert np.array_equal(rows[t2 >= 0].view(np.int32), got[t2 >= 0].view(np.int32))
    assert (rows[t2 < 0] == 0).all()
    want = rows.astype(np.float64)[t2 >= 0].sum()
    assert first[1] == counted
    assert abs(first[0] - want) <= M * 2.0 ** -50 * abs(want), (first[0], want)
    run(hip, name, ptr, ldl, M, V, t2_dev, total)
    second = total.cpu().numpy()
    assert second[1] == 2 * counted and second[0] == first[0] + first[0]
    fresh = torch.zeros(2, dtype=torch.float64, device=dev)
    run(hip, name, ptr, ldl, M, V, t2_dev, fresh)
    assert np.array_equal(fresh.cpu().numpy().view(np.int64), first.view(np.int64)), "total differs between two runs"
    # a NaN row makes the total NaN (it is counted): nothing is dropped silently
    if nan_rows.any():
        tn = torch.zeros(2, dtype=torch.float64, device=dev)
        run(hip, name, ptr, ldl, M, V, t_dev, tn)
        tn = tn.cpu().numpy()
        assert np.isnan(tn[0]) and tn[1] == int((t >= 0).sum())


def test_argument_checks(hip):
    """NULL pointers, M <= 0, V <= 0 and ldl < V return LLJ_EINVAL (1000) before any launch."""
    x = torch.zeros(2, 8, dtype=torch.float32, device=dev)
    t = torch.zeros(2, dtype=torch.int32, device=dev)
    o = torch.zeros(2, dtype=torch.float32, device=dev)
    for name in ("llj_nll", "llj_g_nll"):
        f = getattr(hip, name)
        good = [x.data_ptr(), 8, 2, 8, t.data_ptr(), o.data_ptr(), None, st()]
        for i, bad in ((0, None), (4, None), (5, None), (2, 0), (2, -1), (3, 0), (1, 7)):
            a = list(good)
            a[i] = bad
            assert f(*a) == 1000, (name, i, bad)
    torch.cuda.synchronize()
    assert (o == 0).all()
