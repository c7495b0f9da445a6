"""Prompts of different lengths prefilled as one packed batch (GPU): DecodeSession.prefill_ragged(packed=True),
LLaMA._run_packed / packed_prefill_support, generate.generate_prompts(packed_prefill=True) and the CLIs' flag.

The models, prompts, forced-token driver, B = 1 reference and bound are those of tests/test_ragged_gpu.py: the packed
rows run other GEMM kernels than a T_b-row prefill, so the packed route is held to max |dlogits| <= 3e-2 max |ref| per
row after the prefill and after each of 12 forced steps (the project's bound for swapping routes), not to bit
equality; the default route must stay what it was, launch for launch.
"""
import numpy as np
import pytest
import torch

import tests.helpers as H
from oracle.weights import Cfg, make_params
from tests.test_adapter_gpu import Calls
from tests.test_model_gpu import teacher_forced
from tests.test_ragged_gpu import (BOUND, GREEDY_SEED, LENGTHS, LENGTHS12, S, STEPS, check, drive, forced_of, model,
                                   prompts_of, reference)

pytestmark = pytest.mark.gpu

assert BOUND == 3e-2 and sum(LENGTHS) == 62  # M = 62 >= GEMM_MIN_ROWS = 32: the packed route runs
KINDS = ["bf16-64", "bf16-128", "int4", "adapter", "v2"]


def session(kind, lengths, golden=None, packed=True, **kw):
    from lit_llama.engine import DecodeSession

    sess = DecodeSession(model(kind, golden), len(lengths), S, max(lengths) + 1 + STEPS, **{"use_graph": False, **kw})
    if packed is None:
        sess.prefill_ragged(prompts_of(lengths))
    else:
        sess.prefill_ragged(prompts_of(lengths), packed=packed)
    return sess


def packed_layer(v2="", prefix=False):
    return ["llj_rmsnorm_rows", "llj_gemm_linear" + v2, "llj_rope_kv_packed", "llj_attention_prefill_packed",
            *(["llj_adapter_prefix_add"] if prefix else []), "llj_gemm_resid" + v2, "llj_rmsnorm_rows",
            "llj_gemm_linear" + v2, "llj_gemm_silu_mul" + v2, "llj_gemm_resid" + v2]


# ------------------------------------------------------------------ route and launches
@pytest.mark.parametrize("kind,lengths", [("bf16-64", LENGTHS), ("bf16-64", LENGTHS12), ("adapter", LENGTHS),
                                          ("v2", LENGTHS)], ids=["bf16-B8", "bf16-B12", "adapter", "adapter-v2"])
def test_packed_prefill_streams_every_weight_once(kind, lengths, golden, monkeypatch):
    """One pass over all rows: per layer each Linear's GEMM once whatever B is (c_attn and c_fc1 are both
    llj_gemm_linear), one llj_rope_kv_packed, one llj_attention_prefill_packed (+ llj_adapter_prefix_add on a prefix
    layer), then the head over the B last rows; packed=False runs B per-prompt passes."""
    m = model(kind, golden)
    n_layer = len(m.transformer.h)
    start = n_layer if kind == "bf16-64" else m.config.adapter_start_layer
    assert m.packed_prefill_support(sum(lengths)) is None
    calls = Calls(monkeypatch)
    if hasattr(m, "_build_adapter_kv"):  # the prefix keys / values are made inside the first prefix layer after a
        build = m._build_adapter_kv      # reset_cache(): c_attn on the prefix embedding, not a launch of the prefill

        def unrecorded():
            n = len(calls.names)
            build()
            del calls.names[n:]

        monkeypatch.setattr(m, "_build_adapter_kv", unrecorded)
    sess = session(kind, lengths, golden, packed=True)
    names = list(calls.names)
    assert sess.packed_prefill is True
    v2 = "_v2" if kind == "v2" else ""
    want = ["llj_embedding"]
    for i in range(n_layer):
        want += packed_layer(v2, i >= start)
    assert names[:len(want)] == want, names
    tail = names[len(want):]
    assert tail[-1] == "llj_argmax" and not [n for n in tail if "gemm" in n or "packed" in n or "attention" in n], tail
    assert sum(n.startswith("llj_gemm_") for n in names) == 5 * n_layer
    assert names.count("llj_rope_kv_packed") == names.count("llj_attention_prefill_packed") == n_layer
    assert names.count("llj_embedding") == 1
    calls.names.clear()
    sess = session(kind, lengths, golden, packed=False)
    assert sess.packed_prefill is False
    assert calls.count("llj_embedding") == len(lengths) and not [n for n in calls.names if "packed" in n]


def test_default_prefill_issues_todays_launches(monkeypatch):
    """prefill_ragged(prompts) and prefill_ragged(prompts, packed=False): the launches of a B = 1 session's prefill,
    prompt after prompt, then one choice of the first tokens."""
    from lit_llama.engine import DecodeSession

    m = model("bf16-64")
    calls = Calls(monkeypatch)
    want = []
    for p in prompts_of(LENGTHS):
        calls.names.clear()
        DecodeSession(m, 1, S, p.numel() + 1 + STEPS, use_graph=False).prefill(p.view(1, -1))
        assert calls.names[-1] == "llj_argmax"
        want += calls.names[:-1]
    want.append("llj_argmax")
    for packed in (None, False):
        calls.names.clear()
        sess = session("bf16-64", LENGTHS, packed=packed)
        assert calls.names == want, (packed, calls.names)
        assert sess.packed_prefill is False


# ------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("kind,lengths", [(k, LENGTHS) for k in KINDS] + [("bf16-64", LENGTHS12)],
                         ids=["bf16-hs64", "bf16-hs128", "gptq.int4", "adapter", "adapter-v2", "B12"])
def test_packed_rows_match_batch_1_sessions(kind, lengths, golden):
    ref = reference(kind, lengths, golden)  # (first: a model holds one session's caches at a time)
    m = model(kind, golden)
    loop = session(kind, lengths, golden, packed=False)
    kv0 = [c.clone() for c in m.kv_caches[0]]  # layer 0 after the per-prompt prefill
    sess = session(kind, lengths, golden, packed=True)
    assert sess.packed_prefill is True
    tmax = max(lengths)
    assert (sess.t_prompt, sess.steps_done, int(sess.pos.item())) == (tmax, 1, tmax - 1)
    assert sess.off.cpu().tolist() == [tmax - t for t in lengths] == sess.offsets and sess.work.ragged
    for got, want, what in zip(m.kv_caches[0], kv0, "KV"):
        for b, t in enumerate(lengths):
            H.assert_bf16_close(got[b, :, :t].float().cpu().numpy(), want[b, :, :t].float().cpu().numpy(),
                                f"layer 0 {what} of row {b}")
            assert not got[b, :, t:].view(torch.int16).any(), (what, b)
    got = drive(sess, forced_of(len(lengths)))
    check(got, ref, f"packed {kind} B={len(lengths)}")
    for i, (kc, vc) in enumerate(m.kv_caches):
        for c in (kc, vc):
            for b, t in enumerate(lengths):
                assert c[b, :, :t + STEPS].view(torch.int16).ne(0).any(dim=-1).all(), (i, b)
                assert not c[b, :, t + STEPS:].view(torch.int16).any(), (i, b)
    rows = sess.output_rows()
    for r, p, t in zip(rows, prompts_of(lengths), lengths):
        assert r.shape == (t + 1 + STEPS,) and torch.equal(r[:t], p.to(torch.int32))


# ------------------------------------------------------------------ unchanged behaviour
def test_too_few_rows_take_the_loop():
    """M = 5 < 32 rows: packed=True is the per-prompt prefill, bit for bit."""
    m = model("bf16-64")
    assert isinstance(m.packed_prefill_support(5), str) and m.packed_prefill_support(32) is None
    outs = []
    for packed in (False, True):
        sess = session("bf16-64", [5], packed=packed)
        assert sess.packed_prefill is False
        outs.append((drive(sess, forced_of(1), 3), [c.clone() for kv in m.kv_caches for c in kv]))
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    for a, b in zip(outs[0][1], outs[1][1]):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("kind", ["int8", "fp32"])
def test_unsupported_models_are_unchanged(kind):
    """LLM.int8 and fp32 models: packed_prefill_support gives ragged_support's reason, prefill_ragged raises it
    with either flag, and generate_prompts runs the prompts one after the other as before."""
    import generate as G
    from lit_llama.engine import DecodeSession

    m = model(kind)
    lengths = [20, 30, 25]
    why = m.ragged_support()
    assert why and m.packed_prefill_support(sum(lengths)) == why
    prompts = prompts_of(lengths)
    for packed in (False, True):
        sess = DecodeSession(m, 3, 64, 30 + 6, use_graph=False)
        with pytest.raises(NotImplementedError) as e:
            sess.prefill_ragged(prompts, packed=packed)
        assert str(e.value) == why and sess.packed_prefill is False
    a = G.generate_prompts(m, prompts, 6, top_k=1)
    b = G.generate_prompts(m, prompts, 6, top_k=1, packed_prefill=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ------------------------------------------------------------------ end to end
def test_greedy_rows_equal_single_runs():
    """generate_prompts(top_k=1, packed_prefill=True) against generate() per prompt under the guard of
    tests/test_ragged_gpu.py's test of the same name: a row may differ only from a step whose top-2 margin in the
    B = 1 teacher-forced logits is below 0.05, and at most 2 of the 8 rows may; the precondition (at most 2 rows hold
    such a step at all) is asserted from the B = 1 runs first."""
    import generate as G

    m, n = model("bf16-64"), 10
    prompts = prompts_of(LENGTHS, seed=100 + GREEDY_SEED)
    singles, margins = [], []
    for p in prompts:
        one = G.generate(m, p, n, max_seq_length=S, top_k=1)
        m.reset_cache()
        lg = teacher_forced(m, one.cpu().numpy()[None], p.numel(), S)[0]
        top = np.sort(lg, -1)[:, ::-1]
        singles.append(one)
        margins.append(top[:, 0] - top[:, 1])
    tight = [b for b, mg in enumerate(margins) if (mg < 0.05).any()]
    print(f"rows with a step of margin < 0.05: {tight}; smallest margins " + " ".join(f"{mg.min():.3f}" for mg in margins))
    assert len(tight) <= 2, "precondition: choose another GREEDY_SEED"
    rows = G.generate_prompts(m, prompts, n, max_seq_length=S, top_k=1, packed_prefill=True)
    assert len(rows) == len(prompts)
    exits = 0
    for b, (r, one, p) in enumerate(zip(rows, singles, prompts)):
        assert r.dtype == p.dtype and r.shape == one.shape and torch.equal(r[:p.numel()], p)
        if not torch.equal(r, one):
            s = int((r != one).nonzero()[0, 0]) - p.numel()
            assert margins[b][s] < 0.05, (b, s, float(margins[b][s]))
            exits += 1
    print(f"rows that left through the margin guard: {exits}")
    assert exits <= 2


def test_generate_prompts_passes_the_flag(monkeypatch):
    import generate as G

    m = model("bf16-64")
    calls = Calls(monkeypatch)
    G.generate_prompts(m, prompts_of(LENGTHS), 3, max_seq_length=S, top_k=1)
    assert not [n for n in calls.names if "packed" in n]
    calls.names.clear()
    G.generate_prompts(m, prompts_of(LENGTHS), 3, max_seq_length=S, top_k=1, packed_prefill=True)
    assert calls.count("llj_attention_prefill_packed") == len(m.transformer.h)


def test_graph_replay_equals_eager():
    outs = []
    for graph in (False, True):
        sess = session("bf16-128", LENGTHS, use_graph=graph)
        assert sess.packed_prefill is True
        sess.decode(STEPS)
        torch.cuda.synchronize()
        assert (sess.graph is not None) == graph
        outs.append((sess.output().cpu().numpy(), sess.logits.float().cpu().numpy()))
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])


def test_main_prompts_file_packed(tmp_path, capsys, monkeypatch):
    """generate.py main(prompts_file=..., packed_prefill=True) on the word-level tokenizer set-up of
    tests/test_ragged_gpu.py's test_main_prompts_file, with 38 prompt tokens in all so that the packed route runs:
    one continuation per line of the file, in file order."""
    import generate as G
    from tokenizers import Tokenizer as HFTok
    from tokenizers.models import WordLevel
    from tokenizers.pre_tokenizers import Whitespace

    cfg = Cfg(n_layer=6, n_head=8, n_embd=512, vocab_size=35000)  # llama_configs["19M"]
    ck = tmp_path / "lit-llama.pth"
    torch.save({k: torch.from_numpy(v) for k, v in make_params(cfg, 3).items()}, ck)
    words = [f"w{i}" for i in range(3, 35000)]  # every id decodes to a word
    tok = HFTok(WordLevel({"<pad>": 0, "<s>": 1, "</s>": 2, **{w: i + 3 for i, w in enumerate(words)}},
                          unk_token="<pad>"))
    tok.pre_tokenizer = Whitespace()
    tok.save(str(tmp_path / "tokenizer.json"))
    texts = [" ".join(f"w{i}" for i in range(3, 18)), "w9", " ".join(f"w{i}" for i in range(20, 39))]  # 15 + 1 + 19 words
    pf = tmp_path / "prompts.txt"
    pf.write_text("\n" + texts[0] + "\n\n" + texts[1] + "\n" + texts[2] + "\n\n")
    calls = Calls(monkeypatch)
    G.main("unused", max_new_tokens=10, checkpoint_path=ck, tokenizer_path=tmp_path / "tokenizer.json",
           prompts_file=pf, packed_prefill=True)
    assert calls.count("llj_attention_prefill_packed") == calls.count("llj_rope_kv_packed") == cfg.n_layer
    out, err = capsys.readouterr()
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 3, out
    for l, t in zip(lines, texts):
        assert l.startswith(f"<s> {t} ") and len(l.split()) >= 1 + len(t.split()) + 10 - 2, l
    assert err.count("tokens/sec") == 1 and "3 prompts" in err


@pytest.mark.parametrize("script", ["generate/adapter_v2.py", "generate/lora.py"])
def test_instruction_clis_take_prompts_file(script):
    """Both scripts have main_prompts_file (main keeps the reference's signature, which tests/test_adapter_v2_host.py
    and tests/test_lora_host.py pin), and the parser accepts the flags (a missing checkpoint stops the run at the
    loader's first assertion, after the arguments were parsed)."""
    import importlib.util
    import inspect
    import subprocess
    import sys
    from pathlib import Path

    path = Path(__file__).resolve().parent.parent / "lit-llama-ja_amd" / script
    spec = importlib.util.spec_from_file_location("llj_cli_" + path.stem, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    prm = inspect.signature(mod.main_prompts_file).parameters
    assert list(prm)[0] == "prompts_file" and prm["packed_prefill"].default is False
    assert "prompts_file" not in inspect.signature(mod.main).parameters
    r = subprocess.run([sys.executable, str(path), "--prompts_file", "nowhere.txt", "--packed_prefill",
                        "--pretrained_path", "nowhere.pth"], capture_output=True, text=True)
    assert r.returncode != 0 and "AssertionError" in r.stderr and "unrecognized arguments" not in r.stderr
