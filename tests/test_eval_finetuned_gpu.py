"""Perplexity of fine-tuned models on the GPU: evaluate/full.py's `perplexity` (LLaMA.window_nll: the no-cache
forward of every window and the device NLL kernel over its logits) on this package's adapter v1, adapter v2
and LoRA models against the reference's fp32 run of its own loop on its own models
(tests/golden/eval_finetuned.npz, made by tests/golden/make_golden_eval_finetuned.py).

The fixture's streams (300 tokens: windows of 128, 128 and 44) are text the fine-tuned model finds likely:
leaving the fine-tune tensors out moves every window's summed NLL of the reference by at least 9e-2 (v1),
0.55 (v2), 0.21 (LoRA) relative, so a model that drops the prefix, the affine or the LoRA term fails every
bound below. Bounds: a bf16 model's per-window NLL within 1e-2 relative and its perplexity within 5e-2
(tests/test_model_gpu.py::test_perplexity_matches_reference; the reference's own bf16 run is within 5e-3
of its fp32 NLL, the generator asserts it), an fp32 model's per-window NLL within 1e-4
(tests/test_fp32_gpu.py) and its perplexity within what that implies, the token counts equal. gptq.int4 + v2 / LoRA, which the reference cannot run,
is compared with this package's own dense fp32 model on the dequantized weights within 3e-2.
"""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle.weights import Cfg, make_params, make_prompt
from tests.test_adapter_gpu import CFG, CFG_INT4, Calls, adp_of, build_adapter
from tests.test_adapter_v2_gpu import build_v2
from tests.test_lora_gpu import build_lora, lora_of
from tests.test_model_gpu import build, gen, gptq_packed

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
REL_BF16, REL_PPL_BF16, REL_FP32 = 1e-2, 5e-2, 1e-4
REL_INT4 = 3e-2  # __graft_entry__.smoke(), tests/test_lora_gpu.py: an int4 bf16 model against an fp32 restatement
VARIANTS = ("v1", "v2", "lora")
QKV_GEMM = {"v1": "llj_gemm_qkv_rope", "v2": "llj_gemm_qkv_rope_v2", "lora": "llj_gemm_qkv_rope",
            "lora_unmerged": "llj_gemm_qkv_rope_lora"}
QKV_GEMV = {"v1": "llj_norm_qkv_rope", "v2": "llj_norm_qkv_rope_v2", "lora": "llj_norm_qkv_rope",
            "lora_unmerged": "llj_norm_qkv_rope_lora"}


def perplexity(*a, **kw):
    from evaluate.full import perplexity as f

    return f(*a, **kw)


@pytest.fixture(scope="module")
def g(golden):
    return golden("eval_finetuned")


@pytest.fixture(scope="module")
def make(golden):
    """make(variant, dtype) -> the model of that variant (the tensors of the variant's own fixture), cached."""
    cache = {}

    def f(variant, dtype=torch.bfloat16):
        if (variant, dtype) not in cache:
            if variant == "v1":
                ga = golden("adapter")
                m = build_adapter(CFG, make_params(CFG, int(ga["seed"])), adp_of(ga), dtype=dtype)
            elif variant == "v2":
                ga = golden("adapter_v2")
                m = build_v2(CFG, make_params(CFG, int(ga["seed"])), adp_of(ga), dtype=dtype)
            else:
                ga = golden("lora")
                m = build_lora(CFG, make_params(CFG, int(ga["seed"])), lora_of(ga), merged=variant == "lora",
                               dtype=dtype)
            cache[(variant, dtype)] = m
        return cache[(variant, dtype)]

    return f


def tokens_of(g, variant):
    return torch.from_numpy(g[variant.split("_")[0] + "/tokens"]).cuda()


def window_sums(model, tokens, block=128):
    return np.array([perplexity(model, tokens[:, i:i + block])[1] for i in range(0, tokens.shape[1], block)])


def check(g, variant, model, rel_nll, rel_ppl, what):
    """rel_ppl None: what rel_nll on every window implies for ppl = exp(sum / tokens), rel_nll * sum / tokens."""
    key = variant.split("_")[0]
    tokens = tokens_of(g, variant)
    ppl, nll, toks = perplexity(model, tokens)
    per = window_sums(model, tokens)
    ref = g[key + "/nll_per_window"]
    rels = np.abs(per - ref) / ref
    rp = abs(ppl - float(g[key + "/ppl"])) / float(g[key + "/ppl"])
    if rel_ppl is None:
        rel_ppl = rel_nll * ref.sum() / int(g[key + "/toks"])
    print(f"[eval {variant}] {what}: per-window NLL rel {rels.max():.3e} (bound {rel_nll:g}), ppl {ppl:.4f} vs "
          f"{float(g[key + '/ppl']):.4f} rel {rp:.3e}; the reference's own bf16 {float(g[key + '/rel_ref_bf16_max']):.2e}, "
          f"without the fine-tune {float(g[key + '/rel_finetune_min']):.2f}")
    assert toks == int(g[key + "/toks"]) == tokens.shape[1] - len(ref)
    assert abs(nll - per.sum()) <= 1e-9 * per.sum()  # one accumulator over the windows = the windows one by one
    assert (rels < rel_nll).all(), rels
    assert rp < rel_ppl, rp


@pytest.mark.parametrize("variant", VARIANTS)
def test_bf16_perplexity_matches_reference(g, make, monkeypatch, variant):
    """Windows of 128, 128 and 44 rows: all three through the prefill GEMMs (GEMM_MIN_ROWS = 32), one NLL
    launch pair per window."""
    m = make(variant)
    calls = Calls(monkeypatch)
    perplexity(m, tokens_of(g, variant))
    assert calls.count(QKV_GEMM[variant]) == 3 * CFG.n_layer and calls.count(QKV_GEMV[variant]) == 0
    assert calls.count("llj_nll") == 3 and calls.count("llj_g_nll") == 0
    check(g, variant, m, REL_BF16, REL_PPL_BF16, "bf16, prefill GEMMs")


@pytest.mark.parametrize("variant", VARIANTS)
def test_bf16_perplexity_on_the_row_sliced_gemv_route(g, make, monkeypatch, variant):
    """The same windows with the prefill GEMMs switched off (model.GEMM_MIN_ROWS, as
    tests/test_model_gpu.py::test_prefill_gemm_path_equals_gemv_path): the prompt rows in GEMV row slices."""
    from lit_llama import model as M

    m = make(variant)
    monkeypatch.setattr(M, "GEMM_MIN_ROWS", 10 ** 9)
    calls = Calls(monkeypatch)
    perplexity(m, tokens_of(g, variant))
    assert calls.count(QKV_GEMM[variant]) == 0 and calls.count(QKV_GEMV[variant]) > 0
    check(g, variant, m, REL_BF16, REL_PPL_BF16, "bf16, GEMV row slices")


@pytest.mark.parametrize("variant", VARIANTS)
def test_fp32_perplexity_matches_reference(g, make, monkeypatch, variant):
    m = make(variant, torch.float32)
    calls = Calls(monkeypatch)
    perplexity(m, tokens_of(g, variant))
    assert calls.count("llj_g_nll") == 3 and calls.count("llj_nll") == 0
    check(g, variant, m, REL_FP32, None, "fp32")


@pytest.mark.parametrize("dtype,rel_nll,rel_ppl", [(torch.bfloat16, REL_BF16, REL_PPL_BF16),
                                                   (torch.float32, REL_FP32, None)], ids=["bf16", "fp32"])
def test_lora_unmerged_equals_the_merged_fixture(g, make, monkeypatch, dtype, rel_nll, rel_ppl):
    """Train mode with dropout 0 (the unmerged forward: the `_lora` QKV op) against the merged model's values."""
    m = make("lora_unmerged", dtype)
    assert m.transformer.h[0].attn.c_attn.merged is False
    calls = Calls(monkeypatch)
    perplexity(m, tokens_of(g, "lora"))
    if dtype == torch.bfloat16:
        assert calls.count(QKV_GEMM["lora_unmerged"]) == 3 * CFG.n_layer and calls.count(QKV_GEMM["lora"]) == 0
    else:
        assert calls.count("llj_g_linear_lora") > 0
    check(g, "lora_unmerged", m, rel_nll, rel_ppl, f"unmerged {dtype}")


def _int4_case(variant, golden):
    """(int4 model, dense fp32 model on the dequantized weights, the same without the fine-tune tensors)."""
    from lit_llama.quantization import ColBlockQuantizedLinear

    g4 = golden("int4_gptq")
    p4 = make_params(CFG_INT4, int(g4["seed"]))
    if variant == "v2":
        ga = golden("adapter_v2")
        adp, start = adp_of(ga, "int4/adp/"), int(ga["int4/start"])
        v1 = {k: v for k, v in adp.items() if "adapter_scale" not in k and "adapter_bias" not in k}
        mk = lambda p, t, **kw: build_v2(CFG_INT4, p, t, start=start, **kw)  # noqa: E731
        tensors, without = adp, v1
    else:
        tensors, without = lora_of(golden("lora"), "int4/lora/"), {}
        mk = lambda p, t, **kw: build_lora(CFG_INT4, p, t, merged=False, **kw)  # noqa: E731
    m4 = mk(p4, tensors, mode="gptq.int4", packed=gptq_packed(g4))
    deq = dict(p4)
    for name, mod in m4.named_modules():
        if isinstance(mod, ColBlockQuantizedLinear):
            deq[name + ".weight"] = mod.get_weight(torch.float32).cpu().numpy()
    return m4, mk(deq, tensors, dtype=torch.float32), mk(deq, without, dtype=torch.float32)


@pytest.mark.parametrize("variant", ["v2", "lora"])
def test_int4_perplexity_matches_own_dense_model(golden, monkeypatch, variant):
    """gptq.int4 + adapter v2 / LoRA (unmerged beside the quantized weight): the int4 bf16 model's per-window
    NLL against this package's dense fp32 model on the dequantized weights, within REL_INT4. The stream is the
    dense fp32 model's own greedy text (12 random tokens, then its continuation, per window; windows of 128
    and 44), the first head seed at which leaving the fine-tune tensors out moves that model's window NLL by
    more than 3 * REL_INT4 -- a choice made on the dense models alone."""
    m4, dense, bare = _int4_case(variant, golden)
    for seed in range(40, 48):
        parts = [gen(dense, make_prompt(12, CFG_INT4.vocab_size, seed + 100 * w), n - 12) for w, n in enumerate((128, 44))]
        tokens = torch.from_numpy(np.concatenate(parts)[None].astype(np.int64)).cuda()
        ref, without = window_sums(dense, tokens), window_sums(bare, tokens)
        move = float((np.abs(without - ref) / ref).min())
        if move > 3 * REL_INT4:
            break
    else:
        raise AssertionError(f"no stream on which the fine-tune matters (last move {move:.3f})")
    calls = Calls(monkeypatch)
    got = window_sums(m4, tokens)
    assert calls.count("llj_nll") == 2
    assert calls.count("llj_gemm_qkv_rope_v2" if variant == "v2" else "llj_gemm_qkv_rope_lora") == 2 * CFG_INT4.n_layer
    rels = np.abs(got - ref) / ref
    print(f"[eval int4 {variant}] per-window NLL rel {rels.max():.3e} (bound {REL_INT4:g}); without the fine-tune "
          f"the dense model moves by {move:.3f} (head seed {seed})")
    assert (rels < REL_INT4).all(), rels
    assert perplexity(m4, tokens)[2] == tokens.shape[1] - 2


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_window_nll_values_total_and_call_list(g, make, monkeypatch, variant, dtype):
    """window_nll returns the (T - 1,) per-token values of the logits the forward returns (float64
    log-softmax of the same stored logits, the kernel test's bound), their sum and count arrive in `total`
    over two calls, and a plain forward issues the same calls without the NLL one."""
    m = make(variant, dtype)
    idx = tokens_of(g, variant)[:, 128:225]  # 97 tokens: an odd row count
    T, V = idx.shape[1], m.config.padded_vocab_size
    nll_call = "llj_g_nll" if dtype == torch.float32 else "llj_nll"
    m(idx)  # (an adapter model's first forward after reset_cache() also builds its prefix keys / values)
    calls = Calls(monkeypatch)
    logits = m(idx)[0]
    forward_calls = list(calls.names)
    assert "llj_nll" not in forward_calls and "llj_g_nll" not in forward_calls
    calls.names.clear()
    total = torch.zeros(2, dtype=torch.float64, device="cuda")
    out = m.window_nll(idx, total)
    assert calls.names == forward_calls + [nll_call]
    assert out.shape == (T - 1,) and out.dtype == torch.float32 and out.is_cuda
    lp = torch.log_softmax(logits[:-1].double(), -1)
    ref = -lp.gather(1, idx[0, 1:, None].long())[:, 0].cpu().numpy()
    got = out.double().cpu().numpy()
    bound = (V / 256 + 32) * 2.0 ** -23 + 2.0 ** -22 * np.abs(ref)
    assert (np.abs(got - ref) <= bound).all(), float(np.abs(got - ref).max())
    t = total.cpu().numpy()
    assert t[1] == T - 1 and abs(t[0] - got.sum()) <= T * 2.0 ** -50 * got.sum()
    out2 = m.window_nll(idx, total)
    assert torch.equal(out, out2)
    assert total.cpu().numpy().tolist() == [t[0] + t[0], 2.0 * (T - 1)]
    assert torch.equal(m.window_nll(idx), out)  # total is optional
    with pytest.raises(AssertionError):
        m.window_nll(idx[:, :1])


def test_base_model_forward_issues_no_nll_call(golden, monkeypatch):
    ga = golden("lora")
    m = build(CFG, make_params(CFG, int(ga["seed"])))
    calls = Calls(monkeypatch)
    idx = torch.from_numpy(ga["long_prompt"][None].astype(np.int64)).cuda()
    m(idx)
    gen(m, ga["prompt"], 4)
    assert calls.count("llj_nll") + calls.count("llj_g_nll") == 0
    n = len(calls.names)
    m.window_nll(idx)
    assert calls.names[n:].count("llj_nll") == 1 and calls.names[-1] == "llj_nll"


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_mains_end_to_end(tmp_path, capsys, monkeypatch):
    """evaluate/adapter.py, adapter_v2.py and lora.py on a random 19M checkpoint, fine-tune checkpoints and a
    word-level tokenizer written to tmp_path: each scores the tokens of the wrapped text (the row count of its
    NLL launch) and prints their perplexity, which is `perplexity` of the model built by hand on those tokens
    (within 2e-3: two builds of a bf16 model, far below the distance between two texts); with
    instruction_tuning = False the raw text is scored."""
    from lit_llama import _hip

    rows, orig = [], _hip.call

    def spy(name, *a):
        if name in ("llj_nll", "llj_g_nll"):
            rows.append((name, a[2]))
        return orig(name, *a)

    monkeypatch.setattr(_hip, "call", spy)
    from tokenizers import Tokenizer as HFTok
    from tokenizers.models import WordLevel
    from tokenizers.pre_tokenizers import WhitespaceSplit

    from lit_llama import HFTokenizer

    cfg = Cfg(n_layer=6, n_head=8, n_embd=512, vocab_size=35000)  # llama_configs["19M"]
    p = make_params(cfg, 3)
    ck = tmp_path / "lit-llama.pth"
    torch.save({k: torch.from_numpy(v) for k, v in p.items()}, ck)
    rng = np.random.default_rng(5)
    lo, adp = {}, {}
    for i in range(cfg.n_layer):
        lo[f"transformer.h.{i}.attn.c_attn.lora_A"] = (rng.standard_normal((16, 512)) / np.sqrt(512)).astype(np.float32)
        lo[f"transformer.h.{i}.attn.c_attn.lora_B"] = (0.12 * rng.standard_normal((1024, 8))).astype(np.float32)
        if i >= 2:  # adapter_start_layer = 2, adapter_prompt_length = 10 (the adapter config's defaults)
            adp[f"transformer.h.{i}.attn.adapter_wte.weight"] = rng.standard_normal((10, 512)).astype(np.float32)
            adp[f"transformer.h.{i}.attn.gating_factor"] = rng.uniform(0.5, 1.5, (1, 8, 1, 1)).astype(np.float32)
    v2 = dict(adp)
    v2["lm_head.adapter_scale"] = rng.uniform(0.5, 1.5, 35008).astype(np.float32)  # (the padded vocabulary)
    v2["lm_head.adapter_bias"] = (0.1 * rng.standard_normal(35008)).astype(np.float32)
    paths = {}
    for name, sd in (("lora", lo), ("adapter", adp), ("adapter_v2", v2)):
        paths[name] = tmp_path / f"{name}-finetuned.pth"
        torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, paths[name])
    words = [f"w{i}" for i in range(3, 35000)]
    tok = HFTok(WordLevel({"<pad>": 0, "<s>": 1, "</s>": 2, **{w: i + 3 for i, w in enumerate(words)}},
                          unk_token="<pad>"))
    tok.pre_tokenizer = WhitespaceSplit()
    tok.save(str(tmp_path / "tokenizer.json"))
    text = " ".join(f"w{int(i)}" for i in rng.integers(3, 30000, 150))
    tp = tmp_path / "text.txt"
    tp.write_text(text, encoding="utf-8")
    tokenizer = HFTokenizer(tmp_path / "tokenizer.json")
    for name, flag, dtype in (("lora", "lora_path", "float32"), ("adapter", "adapter_path", "bfloat16"),
                              ("adapter_v2", "adapter_path", "bfloat16")):
        cli = _load(REPO / "lit-llama-ja_amd" / "evaluate" / f"{name}.py", f"llj_evaluate_{name}")
        wrapped = (cli if name == "adapter" else cli._v1).instruction_text(text, True)
        enc = tokenizer.encode(wrapped, bos=True, eos=False, device=torch.device("cuda"))[None]
        raw = tokenizer.encode(text, bos=True, eos=False, device=torch.device("cuda"))[None]
        assert enc.shape[1] > raw.shape[1] == 151
        rows.clear()
        res = cli.main(str(tp), **{flag: paths[name]}, checkpoint_path=ck, tokenizer_path=tmp_path / "tokenizer.json",
                       dtype=dtype)
        assert rows == [("llj_g_nll" if dtype == "float32" else "llj_nll", enc.shape[1] - 1)]
        out, err = capsys.readouterr()
        assert out.strip() == f"Perplexity on {tp}: {res[str(tp)]:.2f}", out
        assert "tokens/sec" in err and "Time to load model" in err and "Memory used" in err
        # by hand: the same model, the wrapped text's tokens
        v1 = cli if name == "adapter" else cli._v1
        sds = ({k: torch.from_numpy(v) for k, v in p.items()},
               {k: torch.from_numpy(v) for k, v in {"lora": lo, "adapter": adp, "adapter_v2": v2}[name].items()})
        dt = getattr(torch, dtype)
        if name == "lora":
            model = v1.generate_cli("lora").load_model(*sds, None, dtype=dt)
            assert model.transformer.h[0].attn.c_attn.merged
        else:
            model = cli.load_model(*sds, None, dt)
            assert hasattr(model.lm_head, "adapter_scale") == (name == "adapter_v2")
        assert abs(perplexity(model, enc)[0] - res[str(tp)]) < 2e-3 * res[str(tp)]
        del model
    # instruction_tuning = False scores the raw text
    cli.instruction_tuning = False
    rows.clear()
    res = cli.main(str(tp), adapter_path=paths["adapter_v2"], checkpoint_path=ck,
                   tokenizer_path=tmp_path / "tokenizer.json", dtype="bfloat16")
    assert rows == [("llj_nll", raw.shape[1] - 1)]
    model = cli.load_model(*sds, None, torch.bfloat16)
    assert abs(perplexity(model, raw)[0] - res[str(tp)]) < 2e-3 * res[str(tp)]
