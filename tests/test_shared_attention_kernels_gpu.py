"""llj_attention_shared (decode attention of B rows that share a prompt prefix of P keys, csrc/attention_shared.hip)
against a numpy float64 attention written here: row b at position p attends keys 0 .. p, the keys below P taken
from row 0's cache and the rest from row b's. Tolerance: helpers.assert_bf16_close at its defaults, the project's
bound for bf16 attention outputs (test_attention, test_attention_split_keys); inputs as in those tests.

Every shape runs at nsplit 1 and at nsplit 32, where prefix ranges are at least 64 keys, so at most 24 of the 32
ranges hold a key (P <= 1500) and the others are empty.
"""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import assert_bf16_close, bf16

pytestmark = pytest.mark.gpu
dev = "cuda"

# hs, nh, B, S, P, p
SHAPES = [
    (128, 2, 8, 64, 17, 16),        # suffix empty: p = P - 1, the first decode step
    (128, 2, 8, 64, 17, 17),
    (128, 3, 5, 144, 80, 143),      # odd B, last slot
    (64, 4, 2, 48, 1, 20),
    (64, 4, 12, 96, 33, 40),        # two row groups
    (128, 2, 1, 64, 10, 30),
    (128, 2, 8, 2048, 1500, 1999),
]
NSPLITS = [1, 32]


def T(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to(dev)  # (a copy: the shared cases are read-only)
    return t if dtype is None else t.to(dtype)


def st():
    return torch.cuda.current_stream().cuda_stream


def oracle(q, kc, vc, P, p, nh, hs):
    """float64: row b over keys 0 .. p, keys < P from row 0, the rest from row b."""
    B = q.shape[0]
    q, kc, vc = q.astype(np.float64), kc.astype(np.float64), vc.astype(np.float64)
    y = np.zeros((B, nh * hs))
    for b in range(B):
        for h in range(nh):
            K = np.concatenate([kc[0, h, :P], kc[b, h, P:p + 1]])
            V = np.concatenate([vc[0, h, :P], vc[b, h, P:p + 1]])
            s = K @ q[b, h * hs:(h + 1) * hs] / np.sqrt(hs)
            e = np.exp(s - s.max())
            y[b, h * hs:(h + 1) * hs] = (e / e.sum()) @ V
    return y


@functools.lru_cache(maxsize=None)
def case(shape):
    """(q, kc, vc, reference) of a shape, computed once and shared (read-only) by the tests below; the rows'
    prefix slots hold different values, so reading the prefix from another row than 0 fails the oracle."""
    hs, nh, B, S, P, p = shape
    rng = np.random.default_rng(hs + S + P + p)
    kc = bf16(rng.standard_normal((B, nh, S, hs)))
    vc = bf16(rng.standard_normal((B, nh, S, hs)))
    q = bf16(rng.standard_normal((B, nh * hs)) * 2)
    ref = oracle(q, kc, vc, P, p, nh, hs)
    for a in (q, kc, vc, ref):
        a.setflags(write=False)
    return q, kc, vc, ref


def run_shared(hip, shape, nsplit, qd, kd, vd, extra=0):
    """y (rows + extra, C) and ws (bytes + extra) pre-filled with 0xFF, after one launch."""
    hs, nh, B, S, P, p = shape
    nb = hip.llj_attention_shared_ws_bytes(B, nh, hs, nsplit)
    assert nb == B * nh * (nsplit + 1) * (hs + 4) * 4
    ws = torch.full((nb + extra,), 0xFF, dtype=torch.uint8, device=dev)
    y = torch.full(((B + extra) * nh * hs,), -1, dtype=torch.int16, device=dev).view(torch.bfloat16).view(B + extra, -1)
    pd = T(np.array([p], np.int32))
    rc = hip.llj_attention_shared(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), y.data_ptr(), pd.data_ptr(), B, P, nh,
                                  hs, S, nsplit, ws.data_ptr(), st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return y, ws


def run_plain(hip, shape, qd, kd, vd):
    hs, nh, B, S, P, p = shape
    y = torch.empty(B, nh * hs, dtype=torch.bfloat16, device=dev)
    pd = T(np.array([p], np.int32))
    rc = hip.llj_attention(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), y.data_ptr(), pd.data_ptr(), B, 1, nh, hs, S,
                           st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("nsplit", NSPLITS)
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes(hip, shape, nsplit):
    q, kc, vc, ref = case(shape)
    y, _ = run_shared(hip, shape, nsplit, T(q, torch.bfloat16), T(kc, torch.bfloat16), T(vc, torch.bfloat16))
    assert_bf16_close(y.float().cpu().numpy(), ref, f"shared attention {shape} nsplit {nsplit}")


@pytest.mark.parametrize("nsplit", NSPLITS)
@pytest.mark.parametrize("shape", SHAPES)
def test_prefix_is_read_from_row_0_only(hip, shape, nsplit):
    """Slots [0, P) of rows 1 .. B - 1 hold NaN: the shared kernel never touches them (finite output, the oracle
    check passes), llj_attention on the same buffers reads them (NaN in those rows)."""
    hs, nh, B, S, P, p = shape
    q, kc, vc, ref = case(shape)
    qd, kd, vd = T(q, torch.bfloat16), T(kc, torch.bfloat16), T(vc, torch.bfloat16)
    kd[1:, :, :P] = float("nan")
    vd[1:, :, :P] = float("nan")
    y, _ = run_shared(hip, shape, nsplit, qd, kd, vd)
    got = y.float().cpu().numpy()
    assert np.isfinite(got).all()
    assert_bf16_close(got, ref, f"shared attention, NaN prefixes {shape} nsplit {nsplit}")
    plain = run_plain(hip, shape, qd, kd, vd).float().cpu().numpy()
    assert np.isfinite(plain[0]).all()
    assert np.isnan(plain[1:]).any(axis=1).all()  # every other row (vacuous at B = 1)


@pytest.mark.parametrize("shape", SHAPES)
def test_agrees_with_per_row_attention_on_copied_prefixes(hip, shape):
    """Rows 1 .. B - 1 hold copies of row 0's prefix (what prefill_shared leaves): llj_attention and the shared
    kernel pass the same oracle check."""
    hs, nh, B, S, P, p = shape
    q, kc, vc, ref = case(shape)
    qd, kd, vd = T(q, torch.bfloat16), T(kc, torch.bfloat16), T(vc, torch.bfloat16)
    kd[1:, :, :P] = kd[:1, :, :P]
    vd[1:, :, :P] = vd[:1, :, :P]
    assert_bf16_close(run_plain(hip, shape, qd, kd, vd).float().cpu().numpy(), ref, f"llj_attention {shape}")
    for nsplit in NSPLITS:
        y, _ = run_shared(hip, shape, nsplit, qd, kd, vd)
        assert_bf16_close(y.float().cpu().numpy(), ref, f"shared attention {shape} nsplit {nsplit}")


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[4], SHAPES[6]])
def test_deterministic(hip, shape):
    q, kc, vc, _ = case(shape)
    qd, kd, vd = T(q, torch.bfloat16), T(kc, torch.bfloat16), T(vc, torch.bfloat16)
    (y1, w1), (y2, w2) = (run_shared(hip, shape, 32, qd, kd, vd) for _ in range(2))
    assert torch.equal(y1.view(torch.int16), y2.view(torch.int16))
    assert torch.equal(w1, w2)  # the partials too (the pad floats keep their fill)


@pytest.mark.parametrize("nsplit", NSPLITS)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[4]])
def test_no_stray_writes(hip, shape, nsplit):
    """y and ws larger than needed and pre-filled with 0xFF bytes: the tails are unchanged."""
    hs, nh, B, S, P, p = shape
    q, kc, vc, ref = case(shape)
    extra = 3
    y, ws = run_shared(hip, shape, nsplit, T(q, torch.bfloat16), T(kc, torch.bfloat16), T(vc, torch.bfloat16), extra)
    assert (y[B:].view(torch.int16) == -1).all()
    assert (ws[-extra:] == 0xFF).all()
    assert_bf16_close(y[:B].float().cpu().numpy(), ref, f"shared attention {shape}")
