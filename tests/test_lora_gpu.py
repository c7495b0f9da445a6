"""Model-level parity of LoRA inference on the GPU: lit_llama.LLaMA built under lit_llama.lora.lora through
the drop-in API (forward, generate = DecodeSession graph replay) against the traces of the reference's own
model (tests/golden/lora.npz, made by tests/golden/make_golden_lora.py).

Merged = eval() (llj_lora_merge folds the update into c_attn's weight: the base model's launches),
unmerged = train mode with dropout 0 (the reference's unmerged forward: one down-projection launch per
layer and the `_lora` QKV op). The fixture's LoRA term moves the reference's fp32 logits by 0.68 relative, so
a model that drops or misplaces it fails every bound below; the reference's own bf16 models are within
1.5e-2 of its fp32 logits on every stored prompt (the generator asserts it), this package's bound is 2e-2
as in the other model tests. gptq.int4 + LoRA, which the reference refuses, is compared with this
package's own dense unmerged models on the dequantized weights.
"""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle.weights import Cfg, make_params
from tests.test_adapter_gpu import CFG, CFG128, CFG_INT4, Calls, rel
from tests.test_model_gpu import build, gen, gptq_packed, guarded, teacher_forced

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
N_NEW = 24
LORA_CALLS = ("llj_norm_qkv_rope_lora", "llj_gemm_qkv_rope_lora", "llj_g_linear_lora", "llj_lora_merge")
REL_INT4 = 3e-2  # __graft_entry__.smoke(): the int4 bf16 model's prefill logits against an fp32 restatement


def lora_of(g, prefix="lora/"):
    return {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}


def build_lora(cfg: Cfg, params: dict, lo: dict, merged=True, mode=None, packed=None, dtype=torch.bfloat16, r=8,
               alpha=16, dropout=0.0):
    """The reference's recipe (generate/lora.py:68-81): build under lora(), load both state dicts, then
    eval() (merged) -- or train() for the unmerged forward of a dense model."""
    from lit_llama import LLaMA, LLaMAConfig
    from lit_llama.lora import lora
    from lit_llama.utils import EmptyInitOnDevice

    with EmptyInitOnDevice(device=torch.device("cuda"), dtype=dtype, quantization_mode=mode), \
            lora(r=r, alpha=alpha, dropout=dropout, enabled=True):
        m = LLaMA(LLaMAConfig(block_size=cfg.block_size, vocab_size=cfg.vocab_size, n_layer=cfg.n_layer,
                              n_head=cfg.n_head, n_embd=cfg.n_embd))
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in {**params, **lo}.items()}
    if packed is not None:
        for k in list(sd):
            if k.endswith(".weight") and k[:-7] + ".quant_weight" in packed:
                del sd[k]
        sd.update({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in packed.items()})
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all("lora_" in k for k in missing), (missing, unexpected)
    c = m.transformer.h[0].attn.c_attn
    assert c.lora_A.is_cuda and c.lora_A.dtype == dtype
    m = m.eval() if merged else m.train()
    assert c.merged == (merged and mode is None)
    return m


@pytest.fixture(scope="module")
def g(golden):
    return golden("lora")


@pytest.fixture(scope="module")
def params(g):
    return make_params(CFG, int(g["seed"]))


@pytest.fixture(scope="module")
def models(g, params):
    return {True: build_lora(CFG, params, lora_of(g), merged=True),
            False: build_lora(CFG, params, lora_of(g), merged=False)}


def cuda_idx(prompt):
    return torch.from_numpy(prompt[None].astype(np.int64)).cuda()


@pytest.mark.parametrize("merged", [True, False])
def test_bf16_prefill_matches_reference(g, models, monkeypatch, merged):
    """12 prompt rows (the decode GEMVs in row slices), the same rows through the prefill GEMMs, and a
    40-token prompt (GEMM rows by itself), each against the reference's fp32 logits."""
    from lit_llama import model as M

    m, tag = models[merged], "merged" if merged else "unmerged"
    idx = cuda_idx(g["prefill_prompt"])
    calls = Calls(monkeypatch)
    m.reset_cache()
    out = m(idx).float().cpu().numpy()[0]
    r = rel(out, g["fp32_prefill_merged"])
    print(f"[lora] bf16 {tag} prefill rel vs the fp32 reference {r:.3e} (the reference's own bf16: "
          f"{float(g['rel_ref_bf16_' + tag]):.3e})")
    assert r < 2e-2, r
    assert calls.count("llj_gemm_qkv_rope") + calls.count("llj_gemm_qkv_rope_lora") == 0
    assert (calls.count("llj_norm_qkv_rope_lora") > 0) == (not merged)
    assert (calls.count("llj_norm_qkv_rope") > 0) == merged
    m.reset_cache()
    out2 = m(idx, CFG.block_size, torch.arange(idx.shape[1]).cuda()).float().cpu().numpy()[0]
    np.testing.assert_allclose(out2, out, rtol=0, atol=1e-6)
    monkeypatch.setattr(M, "GEMM_MIN_ROWS", 8)
    calls.names.clear()
    m.reset_cache()
    out3 = m(idx).float().cpu().numpy()[0]
    assert calls.count("llj_gemm_qkv_rope" if merged else "llj_gemm_qkv_rope_lora") == CFG.n_layer
    r3 = rel(out3, g["fp32_prefill_merged"])
    print(f"[lora] bf16 {tag} prefill through the GEMMs rel {r3:.3e}")
    assert r3 < 2e-2, r3
    monkeypatch.undo()
    calls = Calls(monkeypatch)
    m.reset_cache()
    tail = m(cuda_idx(g["long_prompt"])).float().cpu().numpy()[0, -g["long_fp32_prefill_tail"].shape[0]:]
    m.reset_cache()
    assert calls.count("llj_gemm_qkv_rope" if merged else "llj_gemm_qkv_rope_lora") == CFG.n_layer
    r4 = rel(tail, g["long_fp32_prefill_tail"])
    print(f"[lora] bf16 {tag} 40-token prompt (GEMM rows) rel {r4:.3e} (the reference's own bf16: "
          f"{float(g['long_rel_ref_bf16']):.3e})")
    assert r4 < 2e-2, r4


@pytest.mark.parametrize("merged", [True, False])
@pytest.mark.parametrize("roll", [False, True])
def test_bf16_greedy_matches_reference(g, models, monkeypatch, roll, merged):
    """generate() = DecodeSession: the captured graph of the decode step is what runs; the cache as long
    as the run, and rolling (max_seq_length 16). All 24 steps equal the reference's ids."""
    tag = "roll_" if roll else ""
    prompt = g[tag + "prompt"]
    calls = Calls(monkeypatch)
    ids = gen(models[merged], prompt, N_NEW, **({"max_seq_length": 16} if roll else {}))
    assert (calls.count("llj_norm_qkv_rope_lora") > 0) == (not merged)
    assert np.array_equal(g[tag + "bf16_ids"], g[tag + "fp32_ids"])
    n = int((ids[len(prompt):] == g[tag + "bf16_ids"][len(prompt):]).sum())
    print(f"[lora] greedy merged={merged} roll={roll}: {n} of {N_NEW} steps equal the reference's ids")
    np.testing.assert_array_equal(ids, g[tag + "bf16_ids"])


def test_batch_rows_equal_single_run(g, models):
    """3 decode rows (the streamed-A GEMVs with the norm hand-off, t of three rows) equal single-row runs."""
    import generate as G

    prompt = g["prompt"]
    for merged in (False, True):
        single = gen(models[merged], prompt, N_NEW)
        out = G.generate_batch(models[merged], torch.from_numpy(np.stack([prompt] * 3)).cuda(), N_NEW).cpu().numpy()
        for b in range(3):
            np.testing.assert_array_equal(out[b], single)


@pytest.mark.parametrize("merged", [True, False])
def test_fp32_model_matches_reference(g, params, merged):
    """The fp32 model (any-shape kernels; unmerged: llj_g_linear_lora in fp32): fp32 against fp32."""
    m = build_lora(CFG, params, lora_of(g), merged=merged, dtype=torch.float32)
    out = m(cuda_idx(g["prefill_prompt"]))
    assert out.dtype == torch.float32
    got = out[0].cpu().numpy()
    r = rel(got, g["fp32_prefill_merged"])
    ru = rel(got[-g["fp32_prefill_unmerged_tail"].shape[0]:], g["fp32_prefill_unmerged_tail"])
    print(f"[lora] fp32 merged={merged} prefill rel {r:.2e} (against the reference's unmerged rows {ru:.2e})")
    assert r < 1e-4 and ru < 1e-4, (r, ru)
    for tag in ("", "roll_"):
        prompt = g[tag + "prompt"]
        ids = gen(m, prompt, N_NEW, **({"max_seq_length": 16} if tag else {}))
        n = guarded(ids, g[tag + "fp32_ids"], g[tag + "fp32_top_v"], len(prompt), tol=1e-3)
        assert n == N_NEW, (tag, n)


@pytest.mark.parametrize("merged", [True, False])
def test_bf16_hs128_prefill(g, merged):
    m = build_lora(CFG128, make_params(CFG128, int(g["hs128/seed"])), lora_of(g, "hs128/lora/"), merged=merged)
    r = rel(m(cuda_idx(g["hs128/prompt"])).float().cpu().numpy()[0], g["hs128/fp32_prefill_merged"])
    print(f"[lora] bf16 hs 128 merged={merged} prefill rel {r:.3e} (the reference's own bf16: "
          f"{float(g['hs128/rel_ref_bf16']):.3e})")
    assert r < 2e-2, r


def _trace(model, prompt):
    """(greedy ids, teacher-forced logits per step) of a model of this package: its own reference trace."""
    ids = gen(model, prompt, N_NEW)
    return ids, teacher_forced(model, ids, len(prompt), 64)[0]


def test_int4_lora_matches_own_dense_unmerged_models(g, golden, monkeypatch):
    """gptq.int4 + LoRA (unmerged on the quantized base; the reference raises NotImplementedError for any
    --quantize): the packed weights of int4_gptq.npz dequantized into this package's dense unmerged models
    -- bf16 (greedy ids equal) and fp32 (teacher-forced logits within smoke()'s int4 bound)."""
    from lit_llama.quantization import ColBlockQuantizedLinear

    g4 = golden("int4_gptq")
    p4 = make_params(CFG_INT4, int(g4["seed"]))
    lo = lora_of(g, "int4/lora/")
    calls = Calls(monkeypatch)
    m4 = build_lora(CFG_INT4, p4, lo, mode="gptq.int4", packed=gptq_packed(g4))
    c = m4.transformer.h[0].attn.c_attn
    assert isinstance(c, ColBlockQuantizedLinear) and c.merged is False and calls.count("llj_lora_merge") == 0
    deq = dict(p4)
    for name, mod in m4.named_modules():
        if isinstance(mod, ColBlockQuantizedLinear):
            deq[name + ".weight"] = mod.get_weight(torch.float32).cpu().numpy()
    prompt = g["int4/prompt"]
    T = len(prompt)
    ids32, L32 = _trace(build_lora(CFG_INT4, deq, lo, merged=False, dtype=torch.float32), prompt)
    ids16, _ = _trace(build_lora(CFG_INT4, deq, lo, merged=False), prompt)
    calls.names.clear()
    ids = gen(m4, prompt, N_NEW)
    assert calls.count("llj_norm_qkv_rope_lora") > 0 and calls.count("llj_norm_qkv_rope") == 0
    L4 = teacher_forced(m4, ids32, T, 64)[0]
    rels = [rel(L4[s], L32[s]) for s in range(L32.shape[0])]
    n16, n32 = int((ids == ids16).sum()) - T, int((ids == ids32).sum()) - T
    print(f"[lora] int4 bf16: {n16} / {n32} of {N_NEW} greedy steps equal the dense bf16 / fp32 unmerged models'; "
          f"teacher-forced logits rel max {max(rels):.3e}")
    np.testing.assert_array_equal(ids, ids16)
    assert max(rels) < REL_INT4, rels
    # a dropped term on the int4 path cannot pass: lora_B = 0 moves these logits far beyond the bound
    mz = build_lora(CFG_INT4, p4, {}, mode="gptq.int4", packed=gptq_packed(g4))
    r0 = rel(teacher_forced(mz, ids32[:T + 1], T, 64)[0][0], L32[0])
    print(f"[lora] int4 with lora_B = 0: logits rel {r0:.3f}")
    assert r0 > 10 * REL_INT4, r0
    # ... and the quantized Linear's own forward runs the unmerged form (llj_g_linear + llj_g_linear_lora)
    x = torch.randn(5, CFG_INT4.n_embd, device="cuda", dtype=torch.bfloat16)
    calls.names.clear()
    y = c(x)  # (the any-shape kernel reads the reference layout: the packed codes are unpacked first)
    assert [n for n in calls.names if n.startswith("llj_g_")] == ["llj_g_linear", "llj_g_linear_lora"], calls.names
    dense = build_lora(CFG_INT4, deq, lo, merged=False).transformer.h[0].attn.c_attn
    assert rel(y.float().cpu().numpy(), dense(x).float().cpu().numpy()) < 2e-2


def test_zero_lora_b_is_the_base_model(g, params):
    """lora_B = 0 (the initialisation): bitwise the base model's logits and ids, merged and unmerged,
    prompt rows on the GEMVs, on the GEMMs and the decode graph."""
    base = build(CFG, params)
    only_a = {k: v for k, v in lora_of(g).items() if k.endswith("lora_A")}
    idx, lidx = cuda_idx(g["prefill_prompt"]), cuda_idx(g["long_prompt"])
    want, lwant, ids = base(idx), base(lidx), gen(base, g["prompt"], N_NEW)
    for merged in (True, False):
        m = build_lora(CFG, params, only_a, merged=merged)
        assert torch.count_nonzero(m.transformer.h[0].attn.c_attn.lora_B) == 0
        assert torch.equal(m(idx), want) and torch.equal(m(lidx), lwant), merged
        np.testing.assert_array_equal(gen(m, g["prompt"], N_NEW), ids)


def test_base_and_merged_models_call_no_lora_entry_point(g, params, monkeypatch):
    """A base model never reaches a LoRA export and issues the launches it issued before; a merged dense
    model issues the base model's call list; an unmerged one adds the down-projection per layer and row
    slice and swaps the QKV op for its `_lora` form."""
    idx = cuda_idx(g["prefill_prompt"])
    calls = Calls(monkeypatch)
    lists = {}
    for tag in ("base", "merged", "unmerged"):
        m = build(CFG, params) if tag == "base" else build_lora(CFG, params, lora_of(g), merged=tag == "merged")
        calls.names.clear()
        m(idx)
        m(cuda_idx(g["long_prompt"]))
        gen(m, g["prompt"], 4)
        lists[tag] = list(calls.names)
        n = sum(calls.count(c) for c in LORA_CALLS)
        assert (n > 0) == (tag == "unmerged"), (tag, n)
    assert lists["merged"] == lists["base"]
    un = lists["unmerged"]
    assert un.count("llj_norm_qkv_rope") == 0 and un.count("llj_gemm_qkv_rope") == 0
    n_qkv = lists["base"].count("llj_norm_qkv_rope") + lists["base"].count("llj_gemm_qkv_rope")
    assert un.count("llj_norm_qkv_rope_lora") + un.count("llj_gemm_qkv_rope_lora") == n_qkv
    assert len(un) == len(lists["base"]) + n_qkv  # one down-projection launch per QKV launch, nothing else
    # each `_lora` QKV op directly follows its down-projection
    for i, name in enumerate(un):
        if name == "llj_norm_qkv_rope_lora":
            assert un[i - 1] == "llj_norm_linear", un[i - 2:i + 1]
        if name == "llj_gemm_qkv_rope_lora":
            assert un[i - 1] == "llj_gemm_linear", un[i - 2:i + 1]


def test_train_and_eval_toggle_the_merge(g, params, monkeypatch):
    """eval() merges once, train() unmerges once, repeated calls change nothing; the forward follows."""
    m = build_lora(CFG, params, lora_of(g), merged=False, dtype=torch.float32)
    c = m.transformer.h[0].attn.c_attn
    w0 = c.weight.detach().clone()
    idx = cuda_idx(g["prefill_prompt"])
    un = m(idx)
    calls = Calls(monkeypatch)
    m.eval()
    m.eval()
    assert c.merged and calls.count("llj_lora_merge") == CFG.n_layer and not torch.equal(c.weight, w0)
    me = m(idx)
    assert rel(me.cpu().numpy(), un.cpu().numpy()) < 1e-5
    m.train()
    m.train()
    assert not c.merged and calls.count("llj_lora_merge") == 2 * CFG.n_layer
    assert rel(c.weight.cpu().numpy(), w0.cpu().numpy()) < 1e-6
    # MergedLinear's own forward: F.linear when merged, the unmerged form otherwise
    x = torch.randn(5, CFG.n_embd, device="cuda")
    calls.names.clear()
    y = c(x)
    assert calls.names == ["llj_g_linear", "llj_g_linear_lora"], calls.names
    m.eval()
    calls.names.clear()
    assert rel(c(x).cpu().numpy(), y.cpu().numpy()) < 1e-5 and calls.names == []


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_generate_and_convert_end_to_end(tmp_path, capsys):
    """generate/lora.py and scripts/convert_lora_weights.py on a random 19M checkpoint and LoRA checkpoint
    written to tmp_path; the converted checkpoint in a plain LLaMA reproduces the merged model's logits
    bitwise."""
    from tokenizers import Tokenizer as HFTok
    from tokenizers.models import WordLevel
    from tokenizers.pre_tokenizers import WhitespaceSplit

    cfg = Cfg(n_layer=6, n_head=8, n_embd=512, vocab_size=35000)  # llama_configs["19M"]
    p = make_params(cfg, 3)
    ck, lk = tmp_path / "lit-llama.pth", tmp_path / "lit-llama-lora-finetuned.pth"
    torch.save({k: torch.from_numpy(v) for k, v in p.items()}, ck)
    rng = np.random.default_rng(5)
    lo = {}
    for i in range(cfg.n_layer):
        lo[f"transformer.h.{i}.attn.c_attn.lora_A"] = (rng.standard_normal((16, 512)) / np.sqrt(512)).astype(np.float32)
        lo[f"transformer.h.{i}.attn.c_attn.lora_B"] = (0.12 * rng.standard_normal((1024, 8))).astype(np.float32)
    torch.save({k: torch.from_numpy(v) for k, v in lo.items()}, lk)
    words = ["###", "Response:"] + [f"w{i}" for i in range(5, 35000)]  # every id decodes to a word
    tok = HFTok(WordLevel({"<pad>": 0, "<s>": 1, "</s>": 2, **{w: i + 3 for i, w in enumerate(words)}},
                          unk_token="<pad>"))
    tok.pre_tokenizer = WhitespaceSplit()
    tok.save(str(tmp_path / "tokenizer.json"))
    cli = _load(REPO / "lit-llama-ja_amd" / "generate" / "lora.py", "llj_generate_lora")
    cli.main("w7 w8 w9", lora_path=lk, pretrained_path=ck, tokenizer_path=tmp_path / "tokenizer.json",
             max_new_tokens=10)
    out, err = capsys.readouterr()
    assert len(out.split()) >= 8, out  # the text after the response mark: the new tokens
    assert "tokens/sec" in err and "Time to load model" in err and "Memory used" in err
    with pytest.raises(NotImplementedError, match="LLM.int8"):
        cli.main("w7", lora_path=lk, pretrained_path=ck, tokenizer_path=tmp_path / "tokenizer.json", quantize="llm.int8")
    # ---- convert, then a plain LLaMA on the merged checkpoint against the merged LoRA model
    conv = _load(REPO / "lit-llama-ja_amd" / "scripts" / "convert_lora_weights.py", "llj_convert_lora_weights")
    saved = conv.main(lora_path=lk, checkpoint_path=ck)
    assert saved == tmp_path / "lit-llama-lora-finetuned-lora-merged-weights.pth" and saved.is_file()
    sd = torch.load(saved)
    assert sorted(sd) == sorted(p) and all(v.dtype == torch.bfloat16 for v in sd.values())
    plain = build(cfg, {k: v.float().numpy() for k, v in sd.items()})
    merged = cli.load_model({k: torch.from_numpy(v) for k, v in p.items()}, {k: torch.from_numpy(v) for k, v in lo.items()})
    assert merged.transformer.h[0].attn.c_attn.merged
    idx = torch.arange(3, 15, device="cuda")[None]
    assert torch.equal(plain(idx), merged(idx))
    base = build(cfg, p)
    assert rel(base(idx).float().cpu().numpy(), merged(idx).float().cpu().numpy()) > 0.1  # the update matters here
