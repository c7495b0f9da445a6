"""Model-level parity of LLaMA-Adapter v2 inference on the GPU: lit_llama.adapter.LLaMA +
lit_llama.adapter_v2.add_adapter_v2_parameters_to_linear_layers through the drop-in API (forward, generate
= DecodeSession graph replay) against the traces of the reference's own model
(tests/golden/adapter_v2.npz, made by tests/golden/make_golden_adapter_v2.py).

The fixture's scales (+-U(0.5, 1.5)) and biases (half the rms of each Linear's output) differ per
column and per layer: an identity affine moves the reference's fp32 logits by 1.29 relative, dropping
the biases alone by 1.01, the scales alone by 1.39, so a model that drops or misplaces either fails
every bound below. Tolerances are those of tests/test_adapter_gpu.py for the same comparisons.
"""
import numpy as np
import pytest
import torch

from oracle.weights import Cfg, make_params
from tests.test_adapter_gpu import CFG, CFG128, CFG_INT4, Calls, adp_of, build_adapter, rel
from tests.test_model_gpu import build, gen, gptq_packed, guarded, teacher_forced

pytestmark = pytest.mark.gpu
N_NEW = 24
V2_CALLS = ("llj_linear_v2", "llj_norm_qkv_rope_v2", "llj_linear_resid_v2", "llj_linear_resid_attn_v2",
            "llj_norm_swiglu_v2", "llj_norm_linear_v2", "llj_gemm_linear_v2", "llj_gemm_resid_v2",
            "llj_gemm_silu_mul_v2", "llj_gemm_qkv_rope_v2", "llj_g_linear_v2")


def build_v2(cfg: Cfg, params: dict, adp: dict, start=2, aT=10, mode=None, packed=None, dtype=torch.bfloat16):
    """The reference's recipe (generate/adapter_v2.py:64-71): build, add the parameters, load."""
    from lit_llama.adapter import LLaMA, LLaMAConfig
    from lit_llama.adapter_v2 import add_adapter_v2_parameters_to_linear_layers
    from lit_llama.utils import EmptyInitOnDevice

    with EmptyInitOnDevice(device=torch.device("cuda"), dtype=dtype, quantization_mode=mode):
        m = LLaMA(LLaMAConfig(block_size=cfg.block_size, vocab_size=cfg.vocab_size, n_layer=cfg.n_layer,
                              n_head=cfg.n_head, n_embd=cfg.n_embd, adapter_prompt_length=aT,
                              adapter_start_layer=start))
        add_adapter_v2_parameters_to_linear_layers(m)
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in {**params, **adp}.items()}
    if packed is not None:
        for k in list(sd):
            if k.endswith(".weight") and k[:-7] + ".quant_weight" in packed:
                del sd[k]
        sd.update({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in packed.items()})
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all("adapter_scale" in k or "adapter_bias" in k for k in missing), (missing, unexpected)
    assert m.lm_head.adapter_scale.dtype == dtype and m.lm_head.adapter_scale.is_cuda
    return m.eval()


@pytest.fixture(scope="module")
def g(golden):
    return golden("adapter_v2")


@pytest.fixture(scope="module")
def params(g):
    return make_params(CFG, int(g["seed"]))


@pytest.fixture(scope="module")
def bf16_model(g, params):
    return build_v2(CFG, params, adp_of(g))


def test_bf16_prefill_matches_reference(g, bf16_model, monkeypatch):
    """12 prompt rows (the decode GEMVs in row slices) and the same rows through the prefill GEMMs."""
    from lit_llama import model as M

    m = bf16_model
    idx = torch.from_numpy(g["prompt"][None].astype(np.int64)).cuda()
    calls = Calls(monkeypatch)
    m.reset_cache()
    out = m(idx).float().cpu().numpy()[0]
    r = rel(out, g["fp32_prefill_nocache"])
    print(f"[adapter v2] bf16 prefill rel vs the fp32 reference {r:.3e} (the reference's own bf16: "
          f"{float(g['rel_ref_bf16']):.3e})")
    assert r < 2e-2, r
    assert calls.count("llj_norm_qkv_rope_v2") > 0 and calls.count("llj_gemm_qkv_rope_v2") == 0
    m.reset_cache()
    out2 = m(idx, CFG.block_size, torch.arange(idx.shape[1]).cuda()).float().cpu().numpy()[0]
    np.testing.assert_allclose(out2, out, rtol=0, atol=1e-6)
    monkeypatch.setattr(M, "GEMM_MIN_ROWS", 8)
    calls.names.clear()
    m.reset_cache()
    out3 = m(idx).float().cpu().numpy()[0]
    m.reset_cache()
    assert calls.count("llj_gemm_qkv_rope_v2") == CFG.n_layer and calls.count("llj_gemm_resid_v2") == 2 * CFG.n_layer
    assert calls.count("llj_gemm_silu_mul_v2") == CFG.n_layer and calls.count("llj_gemm_linear_v2") == CFG.n_layer + 1
    r3 = rel(out3, g["fp32_prefill_nocache"])
    print(f"[adapter v2] bf16 prefill through the GEMMs rel {r3:.3e}")
    assert r3 < 2e-2, r3


@pytest.mark.parametrize("roll", [False, True])
def test_bf16_greedy_matches_reference(g, bf16_model, monkeypatch, roll):
    """generate() = DecodeSession: the captured graph of the fused v2 decode step is what runs; the
    cache as long as the run, and rolling (max_seq_length 16)."""
    tag = "roll_" if roll else ""
    prompt = g[tag + "prompt"]
    calls = Calls(monkeypatch)
    ids = gen(bf16_model, prompt, N_NEW, **({"max_seq_length": 16} if roll else {}))
    assert calls.count("llj_norm_swiglu_v2") > 0 and calls.count("llj_attention_adapter") > 0
    n = guarded(ids, g[tag + "bf16_ids"], g[tag + "bf16_top_v"], len(prompt), tol=0.15)
    n32 = guarded(ids, g[tag + "fp32_ids"], g[tag + "fp32_top_v"], len(prompt), tol=0.25)
    print(f"[adapter v2] greedy roll={roll}: {n} / {n32} of {N_NEW} steps equal the reference's bf16 / fp32 ids")
    assert n >= 20, n
    assert n32 >= 20, n32


def test_batch_rows_equal_single_run(g, bf16_model):
    """3 decode rows (the streamed-A GEMVs with the norm hand-off) equal three single-row runs."""
    import generate as G

    prompt = g["prompt"]
    single = gen(bf16_model, prompt, N_NEW)
    prompts = torch.from_numpy(np.stack([prompt] * 3)).cuda()
    out = G.generate_batch(bf16_model, prompts, N_NEW).cpu().numpy()
    for b in range(3):
        np.testing.assert_array_equal(out[b], single)


def test_fp32_model_matches_reference(g, params):
    """The fp32 model (any-shape kernels, llj_g_linear_v2 in fp32): fp32 against fp32; head size 128."""
    m = build_v2(CFG, params, adp_of(g), dtype=torch.float32)
    idx = torch.from_numpy(g["prompt"][None].astype(np.int64)).cuda()
    out = m(idx)
    assert out.dtype == torch.float32
    r = rel(out[0].cpu().numpy(), g["fp32_prefill_nocache"])
    print(f"[adapter v2] fp32 prefill rel {r:.2e}")
    assert r < 1e-4, r
    for tag in ("", "roll_"):
        prompt = g[tag + "prompt"]
        ids = gen(m, prompt, N_NEW, **({"max_seq_length": 16} if tag else {}))
        n = guarded(ids, g[tag + "fp32_ids"], g[tag + "fp32_top_v"], len(prompt), tol=1e-3)
        assert n == N_NEW, (tag, n)
    m2 = build_v2(CFG128, make_params(CFG128, int(g["hs128/seed"])), adp_of(g, "hs128/adp/"), dtype=torch.float32)
    idx2 = torch.from_numpy(g["hs128/prompt"][None].astype(np.int64)).cuda()
    r2 = rel(m2(idx2)[0].cpu().numpy(), g["hs128/fp32_prefill_nocache"])
    print(f"[adapter v2] fp32 hs 128 prefill rel {r2:.2e}")
    assert r2 < 1e-4, r2


def test_bf16_hs128_prefill(g):
    m = build_v2(CFG128, make_params(CFG128, int(g["hs128/seed"])), adp_of(g, "hs128/adp/"))
    idx = torch.from_numpy(g["hs128/prompt"][None].astype(np.int64)).cuda()
    r = rel(m(idx).float().cpu().numpy()[0], g["hs128/fp32_prefill_nocache"])
    print(f"[adapter v2] bf16 hs 128 prefill rel {r:.3e}")
    assert r < 2e-2, r


REL_INT4 = 3e-2  # __graft_entry__.smoke(): the int4 bf16 model's prefill logits against an fp32 restatement


def _trace(model, prompt):
    """(greedy ids, top-2 logit values per step) of a model of this package: its own reference trace."""
    ids = gen(model, prompt, N_NEW)
    L = teacher_forced(model, ids, len(prompt), 64)[0]
    return ids, -np.sort(-L, axis=-1)[:, :2], L


def test_int4_bf16_matches_own_dense_models(g, golden):
    """gptq.int4 v2, which the reference cannot run (its v2 forward calls F.linear on `weight`): the
    packed weights of int4_gptq.npz dequantized into this package's dense v2 models -- fp32 (validated
    against the reference by test_fp32_model_matches_reference) and bf16 (test_bf16_*) -- and the int4 bf16
    streaming model compared with their traces under the guards of
    tests/test_adapter_gpu.py::test_int4_bf16_greedy_matches_reference (0.15 against the bf16 trace, 0.25
    against the fp32 one, all N_NEW steps), plus its teacher-forced logits on the fp32 model's tokens
    against the fp32 model's within REL_INT4."""
    from lit_llama.quantization import ColBlockQuantizedLinear

    g4 = golden("int4_gptq")
    p4 = make_params(CFG_INT4, int(g4["seed"]))
    adp, start = adp_of(g, "int4/adp/"), int(g["int4/start"])
    m4 = build_v2(CFG_INT4, p4, adp, start=start, mode="gptq.int4", packed=gptq_packed(g4))
    assert isinstance(m4.lm_head, ColBlockQuantizedLinear) and hasattr(m4.lm_head, "adapter_scale")
    deq = dict(p4)
    for name, mod in m4.named_modules():
        if isinstance(mod, ColBlockQuantizedLinear):
            deq[name + ".weight"] = mod.get_weight(torch.float32).cpu().numpy()
    prompt = g["int4/prompt"]
    T = len(prompt)
    ids32, top32, L32 = _trace(build_v2(CFG_INT4, deq, adp, start=start, dtype=torch.float32), prompt)
    ids16, top16, _ = _trace(build_v2(CFG_INT4, deq, adp, start=start), prompt)
    ids = gen(m4, prompt, N_NEW)
    n16 = guarded(ids, ids16, top16, T, tol=0.15)
    n32 = guarded(ids, ids32, top32, T, tol=0.25)
    L4 = teacher_forced(m4, ids32, T, 64)[0]
    rels = [rel(L4[s], L32[s]) for s in range(L32.shape[0])]
    print(f"[adapter v2] int4 bf16: {n16} / {n32} of {N_NEW} greedy steps equal the dense bf16 / fp32 models'; "
          f"teacher-forced logits rel max {max(rels):.3e}")
    assert n16 == N_NEW, n16
    assert n32 == N_NEW, n32
    assert max(rels) < REL_INT4, rels
    # a dropped affine on the int4 path cannot pass: identity vectors move these logits far beyond the bound
    v1 = {k: v for k, v in adp.items() if "adapter_scale" not in k and "adapter_bias" not in k}
    mi = build_v2(CFG_INT4, p4, v1, start=start, mode="gptq.int4", packed=gptq_packed(g4))
    r_id = rel(teacher_forced(mi, ids32[:T + 1], T, 64)[0][0], L32[0])
    print(f"[adapter v2] int4 with an identity affine: logits rel {r_id:.3f}")
    assert r_id > 10 * REL_INT4, r_id


def test_identity_affine_is_the_v1_model(g, params):
    """Scale 1, bias 0 (the initialisation) and the same norms: bitwise the v1 model's logits and ids,
    prompt rows on the GEMVs and the decode graph."""
    v1 = {k: v for k, v in adp_of(g).items() if "adapter_scale" not in k and "adapter_bias" not in k}
    a = build_adapter(CFG, params, v1)
    b = build_v2(CFG, params, v1)
    assert torch.equal(b.lm_head.adapter_scale, torch.ones_like(b.lm_head.adapter_scale))
    idx = torch.from_numpy(g["prompt"][None].astype(np.int64)).cuda()
    assert torch.equal(a(idx), b(idx))
    np.testing.assert_array_equal(gen(a, g["prompt"], N_NEW), gen(b, g["prompt"], N_NEW))


def test_base_and_v1_models_call_no_v2_entry_point(g, params, monkeypatch):
    """The base and the v1 model never reach a `_v2` export and issue the launches they issued before;
    the v2 model issues the same number of launches as v1: prompt and decode steps alike."""
    v1 = {k: v for k, v in adp_of(g).items() if "adapter_scale" not in k and "adapter_bias" not in k}
    idx = torch.from_numpy(g["prompt"][None].astype(np.int64)).cuda()
    calls = Calls(monkeypatch)
    counts = {}
    for tag, m in (("base", build(CFG, params)), ("v1", build_adapter(CFG, params, v1)),
                   ("v2", build_v2(CFG, params, adp_of(g)))):
        calls.names.clear()
        m(idx)
        gen(m, g["prompt"], 4)
        n2 = sum(calls.count(c) for c in V2_CALLS)
        assert (n2 > 0) == (tag == "v2"), (tag, n2)
        counts[tag] = len(calls.names)
        if tag == "v2":
            assert calls.count("llj_norm_qkv_rope") == 0 and calls.count("llj_linear_resid") == 0
            assert calls.count("llj_norm_swiglu") == 0 and calls.count("llj_norm_linear") == 0
            # the prefix keys / values come from c_attn's own forward, once per reset_cache(): a dense v1
            # c_attn is torch's F.linear, the v2 one llj_linear_v2 -- one per adapted layer and forward
            assert calls.count("llj_linear_v2") == 2 * (CFG.n_layer - 2)
    assert counts["v1"] == counts["base"], counts
    assert counts["v2"] == counts["v1"] + 2 * (CFG.n_layer - 2), counts  # nothing per layer and step


def test_llm_int8_raises(g, params):
    m = build_v2(CFG, params, adp_of(g), mode="llm.int8")
    idx = torch.from_numpy(g["prompt"][None].astype(np.int64)).cuda()
    with pytest.raises(NotImplementedError, match="LLM.int8"):
        m(idx)


def test_dense_linear_keeps_its_own_bias():
    """reference adapter_v2.py:28-31 passes the Linear's own bias to F.linear: a biased dense Linear
    keeps it on the streaming path (against torch's bf16 F.linear within the bf16 bound of
    tests/helpers.assert_bf16_close) and is refused, not silently unbiased, on the any-shape path."""
    from lit_llama.adapter_v2 import adapter_v2_linear_with_bias_and_scale
    from tests.helpers import assert_bf16_close

    torch.manual_seed(5)
    lin = torch.nn.Linear(256, 80, bias=True, device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        lin.bias.copy_(torch.randn(80))
    x = torch.randn(3, 256, device="cuda", dtype=torch.bfloat16)
    plain = torch.nn.functional.linear(x, lin.weight, lin.bias)
    adapter_v2_linear_with_bias_and_scale(lin)
    with torch.no_grad():
        lin.adapter_scale.copy_(torch.rand(80) + 0.5)
        lin.adapter_bias.copy_(0.3 * torch.randn(80))
        want = lin.adapter_scale * (plain + lin.adapter_bias)
        got = lin(x)
        nobias = lin.adapter_scale * (torch.nn.functional.linear(x, lin.weight) + lin.adapter_bias)
    assert_bf16_close(got.float().cpu().numpy(), want.float().cpu().numpy(), "biased dense v2 Linear")
    assert rel(got.float().cpu().numpy(), nobias.float().cpu().numpy()) > 0.1  # the bias matters here
    lin32 = adapter_v2_linear_with_bias_and_scale(torch.nn.Linear(256, 80, bias=True, device="cuda"))
    with pytest.raises(NotImplementedError), torch.no_grad():
        lin32(torch.randn(3, 256, device="cuda"))
