"""Model-level parity of LLaMA-Adapter inference on the GPU: lit_llama.adapter.LLaMA through the
drop-in API (forward, generate, DecodeSession graph replay) against the traces the reference's own
lit_llama/adapter.py produced (tests/golden/adapter.npz, made by tests/golden/make_golden_adapter.py).

The fixture's gates are non-zero (+-0.5 .. 1.5 per head): zeroing them moves the reference's fp32
logits by 0.37 relative, so a model that drops or mis-scales the prefix term fails every bound
below. The greedy prompts were chosen by looking at the reference alone (its bf16 and fp32 ids agree
on all 24 steps and the first 20 margins exceed the guards), so a margin-guarded comparison cannot
legitimately stop before step 20.
"""
import numpy as np
import pytest
import torch

from oracle.weights import Cfg, make_params
from tests.test_model_gpu import build, gen, gptq_packed, guarded, teacher_forced

pytestmark = pytest.mark.gpu

CFG = Cfg(block_size=128, n_layer=4, n_head=4, n_embd=256, vocab_size=2048)
CFG128 = Cfg(block_size=128, n_layer=4, n_head=2, n_embd=256, vocab_size=2048)
CFG_INT4 = Cfg(block_size=128, n_layer=2, n_head=4, n_embd=256, vocab_size=2048)
REL_I8 = 3e-2  # tests/test_model_7b_gpu.py: llm.int8 against its own statistics-launch form
N_NEW = 24


def adp_of(g, prefix="adp/"):
    return {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}


def build_adapter(cfg: Cfg, params: dict, adp: dict, start=2, aT=10, mode=None, packed=None, dtype=torch.bfloat16,
                  zero_gates=False):
    from lit_llama.adapter import LLaMA, LLaMAConfig
    from lit_llama.utils import EmptyInitOnDevice

    with EmptyInitOnDevice(device=torch.device("cuda"), dtype=dtype, quantization_mode=mode):
        m = LLaMA(LLaMAConfig(block_size=cfg.block_size, vocab_size=cfg.vocab_size, n_layer=cfg.n_layer,
                              n_head=cfg.n_head, n_embd=cfg.n_embd, adapter_prompt_length=aT,
                              adapter_start_layer=start))
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in {**params, **adp}.items()}
    if zero_gates:
        sd = {k: (torch.zeros_like(v) if k.endswith("gating_factor") else v) for k, v in sd.items()}
    if packed is not None:
        for k in list(sd):
            if k.endswith(".weight") and k[:-7] + ".quant_weight" in packed:
                del sd[k]
        sd.update({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in packed.items()})
    m.load_state_dict(sd)
    assert m.transformer.wte.weight.dtype == dtype
    return m.eval()


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


class Calls:
    """Names of the library entry points a block of code goes through (wraps lit_llama._hip.call)."""

    def __init__(self, monkeypatch):
        from lit_llama import _hip

        self.names = []
        orig = _hip.call

        def spy(name, *a):
            self.names.append(name)
            return orig(name, *a)

        monkeypatch.setattr(_hip, "call", spy)

    def count(self, name):
        return self.names.count(name)


@pytest.fixture(scope="module")
def g(golden):
    return golden("adapter")


@pytest.fixture(scope="module")
def params(g):
    return make_params(CFG, int(g["seed"]))


@pytest.fixture(scope="module")
def bf16_model(g, params):
    return build_adapter(CFG, params, adp_of(g))


@pytest.fixture(scope="module")
def fp32_model(g, params):
    return build_adapter(CFG, params, adp_of(g), dtype=torch.float32)


def test_bf16_prefill_matches_reference(g, bf16_model):
    m = bf16_model
    idx = torch.from_numpy(g["prompt"][None].astype(np.int64)).cuda()
    m.reset_cache()
    out = m(idx).float().cpu().numpy()[0]
    r = rel(out, g["fp32_prefill_nocache"])
    print(f"[adapter] bf16 prefill rel vs the fp32 reference {r:.3e} (the reference's own bf16: {float(g['rel_ref_bf16']):.3e})")
    assert r < 2e-2, r
    m.reset_cache()
    out2 = m(idx, CFG.block_size, torch.arange(idx.shape[1]).cuda()).float().cpu().numpy()[0]
    m.reset_cache()
    np.testing.assert_allclose(out2, out, rtol=0, atol=1e-6)


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("roll", [False, True])
def test_bf16_greedy_matches_reference(g, bf16_model, monkeypatch, fused, roll):
    """generate() (captured-graph decode) with the prefix term inside the decode attention launch
    (fused) and as llj_attention + llj_adapter_prefix_add; the cache as long as the run, and rolling
    (max_seq_length 16) while the prefix stays."""
    import lit_llama.adapter as A

    monkeypatch.setattr(A, "ADAPTER_FUSED", fused)
    tag = "roll_" if roll else ""
    prompt = g[tag + "prompt"]
    calls = Calls(monkeypatch)
    ids = gen(bf16_model, prompt, N_NEW, **({"max_seq_length": 16} if roll else {}))
    assert (calls.count("llj_attention_adapter") > 0) == bool(fused)
    assert (calls.count("llj_adapter_prefix_add") > 0) == (not fused)
    n = guarded(ids, g[tag + "bf16_ids"], g[tag + "bf16_top_v"], len(prompt), tol=0.15)
    n32 = guarded(ids, g[tag + "fp32_ids"], g[tag + "fp32_top_v"], len(prompt), tol=0.25)
    print(f"[adapter] greedy fused={fused} roll={roll}: {n} / {n32} of {N_NEW} steps equal the reference's bf16 / fp32 ids")
    assert n >= 20, n
    assert n32 >= 20, n32


def test_batch_rows_equal_single_run(g, bf16_model):
    import generate as G

    prompt = g["prompt"]
    single = gen(bf16_model, prompt, N_NEW)
    prompts = torch.from_numpy(np.stack([prompt] * 3)).cuda()
    out = G.generate_batch(bf16_model, prompts, N_NEW).cpu().numpy()
    for b in range(3):
        np.testing.assert_array_equal(out[b], single)


def test_fp32_model_matches_reference(g, fp32_model, params):
    """The fp32 model (any-shape kernels + llj_adapter_prefix_add in fp32): fp32 against fp32."""
    m = fp32_model
    idx = torch.from_numpy(g["prompt"][None].astype(np.int64)).cuda()
    out = m(idx)
    assert out.dtype == torch.float32
    r = rel(out[0].cpu().numpy(), g["fp32_prefill_nocache"])
    print(f"[adapter] fp32 prefill rel {r:.2e}")
    assert r < 1e-4, r
    for tag in ("", "roll_"):
        prompt = g[tag + "prompt"]
        ids = gen(m, prompt, N_NEW, **({"max_seq_length": 16} if tag else {}))
        n = guarded(ids, g[tag + "fp32_ids"], g[tag + "fp32_top_v"], len(prompt), tol=1e-3)
        assert n == N_NEW, (tag, n)
    # head size 128
    m2 = build_adapter(CFG128, make_params(CFG128, int(g["hs128/seed"])), adp_of(g, "hs128/adp/"), dtype=torch.float32)
    idx2 = torch.from_numpy(g["hs128/prompt"][None].astype(np.int64)).cuda()
    r2 = rel(m2(idx2)[0].cpu().numpy(), g["hs128/fp32_prefill_nocache"])
    print(f"[adapter] fp32 hs 128 prefill rel {r2:.2e}")
    assert r2 < 1e-4, r2


def test_bf16_hs128_prefill(g):
    """head size 128 on the streaming path (llj_attention_adapter<128>) against the fp32 reference."""
    m = build_adapter(CFG128, make_params(CFG128, int(g["hs128/seed"])), adp_of(g, "hs128/adp/"))
    idx = torch.from_numpy(g["hs128/prompt"][None].astype(np.int64)).cuda()
    r = rel(m(idx).float().cpu().numpy()[0], g["hs128/fp32_prefill_nocache"])
    print(f"[adapter] bf16 hs 128 prefill rel {r:.3e}")
    assert r < 2e-2, r


def int4_models(g, golden, dtype):
    g4 = golden("int4_gptq")
    p4 = make_params(CFG_INT4, int(g4["seed"]))
    return build_adapter(CFG_INT4, p4, adp_of(g, "int4/adp/"), start=int(g["int4/start"]), mode="gptq.int4",
                         packed=gptq_packed(g4), dtype=dtype)


def test_int4_fp32_matches_reference(g, golden):
    m = int4_models(g, golden, torch.float32)
    prompt = g["int4/prompt"]
    T = len(prompt)
    ids = gen(m, prompt, N_NEW)
    assert guarded(ids, g["int4/fp32_ids"], g["int4/fp32_top_v"], T, tol=1e-3) == N_NEW
    L = teacher_forced(m, g["int4/fp32_ids"][:T + 6], T, 64)[0]
    for s in (0, 5):
        r = rel(L[s], g[f"int4/fp32_logits_step{s}"])
        print(f"[adapter] int4 fp32 step {s} rel {r:.2e}")
        assert r < 1e-4, (s, r)


def test_int4_bf16_greedy_matches_reference(g, golden):
    from lit_llama.quantization import ColBlockQuantizedLinear

    m = int4_models(g, golden, torch.bfloat16)
    assert isinstance(m.transformer.h[1].attn.c_attn, ColBlockQuantizedLinear)
    prompt = g["int4/prompt"]
    T = len(prompt)
    ids = gen(m, prompt, N_NEW)
    assert guarded(ids, g["int4/bf16_ids"], g["int4/bf16_top_v"], T, tol=0.15) == N_NEW
    assert guarded(ids, g["int4/fp32_ids"], g["int4/fp32_top_v"], T, tol=0.25) == N_NEW


def test_flash_and_split_routes_agree_with_one_block(g, bf16_model, monkeypatch):
    """A 40-token prompt (the flash kernel) and a decode step over a split cache take their own
    attention kernel plus llj_adapter_prefix_add; the last-row logits agree with the same model
    forced down the one-block route (llj_attention_adapter)."""
    from lit_llama import model as M

    m = bf16_model
    rng = np.random.default_rng(40)
    idx = torch.from_numpy(rng.integers(3, CFG.vocab_size, (1, 41))).cuda()
    S = CFG.block_size

    def run():
        m.reset_cache()
        a = m(idx[:, :40], S, torch.arange(40).cuda())[0, -1].float().cpu().numpy()
        b = m(idx[:, 40:], S, torch.tensor([40]).cuda())[0, -1].float().cpu().numpy()
        m.reset_cache()
        return a, b

    calls = Calls(monkeypatch)
    monkeypatch.setattr(M, "ATTN_SPLIT_MIN_S", 64)
    monkeypatch.setattr(M, "ATTN_SPLIT_KEYS", 32)
    assert 40 >= M.FLASH_MIN_T and S > M.ATTN_SPLIT_KEYS
    pre_a, dec_a = run()
    n_ad = CFG.n_layer - 2
    assert calls.count("llj_attention_prefill") == CFG.n_layer and calls.count("llj_attention_split") == CFG.n_layer
    assert calls.count("llj_adapter_prefix_add") == 2 * n_ad and calls.count("llj_attention_adapter") == 0
    calls.names.clear()
    monkeypatch.setattr(M, "FLASH_MIN_T", 10 ** 9)
    monkeypatch.setattr(M, "ATTN_SPLIT_MIN_S", 10 ** 9)
    pre_b, dec_b = run()
    assert calls.count("llj_attention_adapter") == 2 * n_ad and calls.count("llj_adapter_prefix_add") == 0
    assert calls.count("llj_attention_prefill") == 0 and calls.count("llj_attention_split") == 0
    r1, r2 = rel(pre_a, pre_b), rel(dec_a, dec_b)
    print(f"[adapter] flash vs one-block {r1:.3e}; split vs one-block {r2:.3e}")
    assert r1 < 2e-2, r1
    assert r2 < 2e-2, r2


@pytest.mark.parametrize("fused", [1, 0])
def test_zero_gates_is_the_base_model(g, params, monkeypatch, fused):
    """Zero-init attention: with all gates zero the adapter model is lit_llama.LLaMA bit for bit."""
    import lit_llama.adapter as A

    monkeypatch.setattr(A, "ADAPTER_FUSED", fused)
    base = build(CFG, params)
    m = build_adapter(CFG, params, adp_of(g), zero_gates=True)
    idx = torch.from_numpy(g["prompt"][None].astype(np.int64)).cuda()
    assert torch.equal(m(idx), base(idx))
    ids, ids0 = gen(m, g["prompt"], N_NEW), gen(base, g["prompt"], N_NEW)
    np.testing.assert_array_equal(ids, ids0)


def test_legacy_gating_checkpoint(g, params):
    """A checkpoint with one gating value for a whole layer (fewer than four dimensions)."""
    adp = adp_of(g, "legacy/adp/")
    assert adp["transformer.h.2.attn.gating_factor"].ndim < 4
    m = build_adapter(CFG, params, adp, dtype=torch.float32)
    idx = torch.from_numpy(g["prompt"][None].astype(np.int64)).cuda()
    r = rel(m(idx)[0].cpu().numpy(), g["legacy/fp32_prefill_nocache"])
    print(f"[adapter] legacy gating fp32 prefill rel {r:.2e}")
    assert r < 1e-4, r
    assert rel(g["legacy/fp32_prefill_nocache"], g["fp32_prefill_nocache"]) > 1e-2  # a different model


def test_llm_int8_zero_gates_close_to_base(g, params):
    """llm.int8: the adapter model never takes the statistics hand-off (llj_attention_i8 emits y's
    statistics before the prefix term), so with zero gates it differs from the base llm.int8 model
    only by y's statistics coming from llj_i8_stats. Non-zero gates under llm.int8 are unpinned: the
    reference's Linear8bitLt needs bitsandbytes, which the fixture generator's host lacks."""
    base = build(CFG, params, mode="llm.int8")
    m = build_adapter(CFG, params, adp_of(g), mode="llm.int8", zero_gates=True)
    T = len(g["prompt"])
    seq = g["bf16_ids"][:T + 4]
    La = teacher_forced(m, seq[4:], T - 4, 64)[0]  # 8 prompt rows: decode-size launches from the start
    Lb = teacher_forced(base, seq[4:], T - 4, 64)[0]
    for s in range(La.shape[0]):
        r = rel(La[s], Lb[s])
        assert r < REL_I8, (s, r)


def test_base_model_issues_no_adapter_launch(g, params, monkeypatch):
    """A plain lit_llama.LLaMA never reaches either new export; the adapter model does."""
    calls = Calls(monkeypatch)
    base = build(CFG, params)
    idx = torch.from_numpy(g["prompt"][None].astype(np.int64)).cuda()
    base(idx)
    gen(base, g["prompt"], 4)
    assert calls.count("llj_attention") > 0
    assert calls.count("llj_attention_adapter") == 0 and calls.count("llj_adapter_prefix_add") == 0
    n_base = len(calls.names)
    calls.names.clear()
    m = build_adapter(CFG, params, adp_of(g))
    m(idx)
    gen(m, g["prompt"], 4)
    assert calls.count("llj_attention_adapter") > 0
    assert len(calls.names) == n_base  # the prefix term costs no launch on the fused route
