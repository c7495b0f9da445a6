"""Prompts of different lengths decoded as one batch (GPU): DecodeSession.prefill_ragged / output_rows, the decode
route of c_attn's plain store + llj_attention_ragged, generate.generate_prompts and generate.main(prompts_file=...).

Sessions are driven with forced tokens, as in tests/test_samples_gpu.py, so that a last-bit difference between two
routes cannot change the sequence: use_graph=False, and before every decode(1) row-distinct tokens from a fixed
random (B, n) table are copied into sess.cur; sess.logits is read after the step. The comparison is the existing
code: for each row a B = 1 DecodeSession that prefills that row's prompt and takes the same forced tokens. Bound:
max |dlogits| <= 3e-2 max |ref| at every step and row, the project's bound for swapping attention routes
(test_long_cache_split_attention_decode, tests/test_samples_gpu.py).
"""
import numpy as np
import pytest
import torch

from oracle.weights import Cfg, make_params
from tests.test_adapter_gpu import CFG as ADP_CFG
from tests.test_adapter_gpu import Calls, adp_of, build_adapter
from tests.test_model_gpu import _random_int4_model, build, teacher_forced

pytestmark = pytest.mark.gpu

CFGS = {
    64: Cfg(block_size=128, n_layer=2, n_head=4, n_embd=256, vocab_size=2048),
    128: Cfg(block_size=128, n_layer=2, n_head=2, n_embd=256, vocab_size=2048),
}
LENGTHS = [1, 2, 5, 9, 9, 13, 16, 7]
LENGTHS12 = LENGTHS + [3, 11, 1, 6]
S, STEPS = 32, 12
BOUND = 3e-2
# the prompts of test_greedy_rows_equal_single_runs: of the seeds 0 .. 7 the one whose B = 1 runs (the existing code
# alone) have at most 2 rows with a step of margin < 0.05 (2; the others 4 to 6: this model's bf16 logits sit 0.031
# apart). The test asserts that precondition itself.
GREEDY_SEED = 5

_models, _refs = {}, {}


def model(kind, golden=None):
    if kind not in _models:
        if kind in ("bf16-64", "bf16-128", "int8", "fp32"):
            cfg = CFGS[128 if kind == "bf16-128" else 64]
            params = make_params(cfg, 7)
            if kind == "fp32":
                from tests.test_fp32_gpu import build32

                _models[kind] = build32(cfg, params)
            else:
                _models[kind] = build(cfg, params, mode="llm.int8" if kind == "int8" else None)
        elif kind == "int4":
            _models[kind] = _random_int4_model(256, 4, seed=31)
        elif kind == "adapter":
            g = golden("adapter")
            _models[kind] = build_adapter(ADP_CFG, make_params(ADP_CFG, int(g["seed"])), adp_of(g))
        elif kind == "v2":
            from tests.test_adapter_v2_gpu import build_v2

            g = golden("adapter_v2")
            _models[kind] = build_v2(ADP_CFG, make_params(ADP_CFG, int(g["seed"])), adp_of(g))
        else:
            raise KeyError(kind)
    return _models[kind]


def prompts_of(lengths, seed=21):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(3, 2048, (t,), generator=g).cuda() for t in lengths]


def forced_of(rows):
    return torch.randint(3, 2048, (rows, STEPS), generator=torch.Generator().manual_seed(22)).to(torch.int32).cuda()


def drive(sess, forced, steps=STEPS):
    """logits after the prefill and after each forced step: (steps + 1, rows, V) float32"""
    torch.cuda.synchronize()
    out = [sess.logits.float().cpu().numpy()]
    for s in range(steps):
        sess.cur.copy_(forced[:, s])
        sess.decode(1)
        torch.cuda.synchronize()
        out.append(sess.logits.float().cpu().numpy())
    return np.stack(out)


def reference(kind, lengths, golden=None):
    """The existing code, row by row: a B = 1 session per prompt with that row's forced tokens. (steps + 1, B, V),
    computed once per case and left unchanged."""
    from lit_llama.engine import DecodeSession

    key = (kind, tuple(lengths))
    if key not in _refs:
        m, forced, rows = model(kind, golden), forced_of(len(lengths)), []
        for b, p in enumerate(prompts_of(lengths)):
            sess = DecodeSession(m, 1, S, p.numel() + 1 + STEPS, use_graph=False)
            sess.prefill(p.view(1, -1))
            rows.append(drive(sess, forced[b:b + 1])[:, 0])
        ref = np.stack(rows, 1)
        ref.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def ragged_session(kind, lengths, golden=None, **kw):
    from lit_llama.engine import DecodeSession

    sess = DecodeSession(model(kind, golden), len(lengths), S, max(lengths) + 1 + STEPS, **{"use_graph": False, **kw})
    sess.prefill_ragged(prompts_of(lengths))
    return sess


def check(got, ref, what):
    worst = 0.0
    for s in range(ref.shape[0]):
        ratios = [float(np.abs(got[s, b] - ref[s, b]).max() / np.abs(ref[s, b]).max()) for b in range(ref.shape[1])]
        worst = max(worst, max(ratios))
        print(f"[{what}] step {s}: max |dlogits| / max |ref| per row " + " ".join(f"{r:.2e}" for r in ratios))
    print(f"[{what}] worst ratio {worst:.3e} (bound {BOUND})")
    for s in range(ref.shape[0]):
        for b in range(ref.shape[1]):
            assert np.abs(got[s, b] - ref[s, b]).max() <= BOUND * np.abs(ref[s, b]).max(), (what, s, b)


@pytest.mark.parametrize("kind,lengths", [("bf16-64", LENGTHS), ("bf16-128", LENGTHS), ("int4", LENGTHS),
                                          ("adapter", LENGTHS), ("v2", LENGTHS), ("bf16-64", LENGTHS12),
                                          ("bf16-64", [5])],
                         ids=["bf16-hs64", "bf16-hs128", "gptq.int4", "adapter", "adapter-v2", "B12", "B1"])
def test_ragged_rows_match_batch_1_sessions(kind, lengths, golden):
    ref = reference(kind, lengths, golden)  # (first: a model holds one session's caches at a time)
    sess = ragged_session(kind, lengths, golden)
    tmax = max(lengths)
    assert sess.work.ragged and sess.work.qkv.shape == (len(lengths), 3 * 256)
    assert (sess.t_prompt, sess.steps_done, int(sess.pos.item())) == (tmax, 1, tmax - 1)
    assert sess.off.cpu().tolist() == [tmax - t for t in lengths] == sess.offsets
    got = drive(sess, forced_of(len(lengths)))
    np.testing.assert_array_equal(got[0], ref[0])  # the prefill logits: bitwise a B = 1 session's
    check(got, ref, f"{kind} B={len(lengths)}")
    # the token buffer: left-padded prompts, then the first chosen token and the forced ones' successors
    rows = sess.output_rows()
    for r, p, t in zip(rows, prompts_of(lengths), lengths):
        assert r.shape == (t + 1 + STEPS,) and torch.equal(r[:t], p.to(torch.int32))
    assert sess.output().shape == (len(lengths), tmax + 1 + STEPS)


def test_caches_hold_each_row_at_its_own_positions():
    """After the prefill and 3 steps row b's slots 0 .. T_b + 2 are written (bitwise the B = 1 prefill's in the
    prompt's slots) and every slot above is still zero."""
    from lit_llama.engine import DecodeSession

    m, prompts, forced = model("bf16-64"), prompts_of(LENGTHS), forced_of(len(LENGTHS))
    single = []
    for p in prompts[:3]:
        s1 = DecodeSession(m, 1, S, p.numel() + 4, use_graph=False)
        s1.prefill(p.view(1, -1))
        single.append([(kc[0, :, :p.numel()].clone(), vc[0, :, :p.numel()].clone()) for kc, vc in m.kv_caches])
    sess = ragged_session("bf16-64", LENGTHS)
    drive(sess, forced, 3)
    for i, (kc, vc) in enumerate(m.kv_caches):
        for c in (kc, vc):
            bits = c.view(torch.int16)
            for b, t in enumerate(LENGTHS):
                assert bits[b, :, :t + 3].ne(0).any(dim=-1).all(), (i, b)
                assert not bits[b, :, t + 3:].any(), (i, b)
        for b in range(3):
            assert torch.equal(kc[b, :, :LENGTHS[b]], single[b][i][0]) and torch.equal(vc[b, :, :LENGTHS[b]], single[b][i][1])


def test_graph_replay_equals_eager():
    outs = []
    for graph in (False, True):
        sess = ragged_session("bf16-128", LENGTHS, use_graph=graph)
        sess.decode(STEPS)
        torch.cuda.synchronize()
        assert (sess.graph is not None) == graph
        outs.append((sess.output().cpu().numpy(), sess.logits.float().cpu().numpy()))
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])


def test_greedy_rows_equal_single_runs():
    """generate_prompts(top_k=1) against generate() per prompt, with the guard of test_batch12_rows_equal_single_runs:
    a row may differ only from a step whose top-2 margin in the B = 1 teacher-forced logits is below 0.05. At most 2
    of the 8 rows may take that exit; the prompts (GREEDY_SEED) are such that at most 2 rows contain any step with a
    margin below 0.05, which is asserted from the B = 1 runs before anything is compared."""
    import generate as G

    m, n = model("bf16-64"), 10
    prompts = prompts_of(LENGTHS, seed=100 + GREEDY_SEED)
    singles, margins = [], []
    for p in prompts:
        one = G.generate(m, p, n, max_seq_length=S, top_k=1)
        m.reset_cache()
        lg = teacher_forced(m, one.cpu().numpy()[None], p.numel(), S)[0]  # (n, V): the logits behind each new token
        top = np.sort(lg, -1)[:, ::-1]
        singles.append(one)
        margins.append(top[:, 0] - top[:, 1])
    tight = [b for b, mg in enumerate(margins) if (mg < 0.05).any()]
    print(f"rows with a step of margin < 0.05: {tight}; smallest margins " + " ".join(f"{mg.min():.3f}" for mg in margins))
    assert len(tight) <= 2, "precondition: choose another GREEDY_SEED"
    rows = G.generate_prompts(m, prompts, n, max_seq_length=S, top_k=1)
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


def test_eos_cuts_each_row_at_its_own_first_eos():
    import generate as G

    m, n = model("bf16-64"), 20
    prompts = prompts_of(LENGTHS, seed=41)
    full = G.generate_prompts(m, prompts, n, max_seq_length=S + 8, top_k=1)
    assert [r.numel() for r in full] == [t + n for t in LENGTHS]
    # the EOS id: the new token that occurs in the most rows (each row is then cut at its own first occurrence)
    news = [r[t:].tolist() for r, t in zip(full, LENGTHS)]
    eos = max(sorted({x for row in news for x in row}), key=lambda x: sum(x in row for row in news))
    cut = G.generate_prompts(m, prompts, n, max_seq_length=S + 8, top_k=1, eos_id=eos)
    lens = []
    for r, c, t, new in zip(full, cut, LENGTHS, news):
        want = r[:t + new.index(eos)] if eos in new else r
        assert torch.equal(c, want)
        assert eos not in c[t:].tolist()
        lens.append(c.numel() - t)
    print(f"eos {eos}: new tokens per row {lens}")
    assert min(lens) < n and len(set(lens)) > 1  # rows finish at different steps


def _layer(qkv, att, extra=()):
    return [qkv, att, *extra, "llj_linear_resid", "llj_norm_swiglu", "llj_linear_resid"]


def test_plain_sessions_issue_todays_launches(monkeypatch):
    """prefill / generate / generate_batch never reach llj_attention_ragged, and a plain decode step is the sequence
    of model.py's header: per layer c_attn + RoPE + KV write, attention, c_proj, SwiGLU, mlp.c_proj (batched rows:
    one llj_rmsnorm_rows ahead of layer 0, the norm statistics handed on from there)."""
    import generate as G
    from lit_llama.engine import DecodeSession

    m = model("bf16-64")
    calls = Calls(monkeypatch)
    prompts = prompts_of([6] * 8)
    G.generate(m, prompts[0], 4, top_k=1)
    G.generate(m, prompts[0], 4, top_k=5)
    G.generate_batch(m, torch.stack(prompts), 4)
    G.generate_samples(m, prompts[0], 3, 4, top_k=1)
    assert calls.count("llj_attention") > 0 and calls.count("llj_norm_qkv_rope") > 0
    assert calls.count("llj_attention_ragged") == 0
    for rows in (1, 8):
        sess = DecodeSession(m, rows, S, 12, use_graph=False)
        sess.prefill(torch.stack(prompts[:rows]))
        assert not sess.work.ragged and sess.work.off is None and not hasattr(sess.work, "qkv")
        calls.names.clear()
        sess.decode(1)
        want = ["llj_embedding"] + (["llj_rmsnorm_rows"] if rows > 1 else [])
        want += 2 * _layer("llj_norm_qkv_rope", "llj_attention") + ["llj_norm_linear", "llj_argmax"]
        assert calls.names == want, (rows, calls.names)


@pytest.mark.parametrize("kind", ["bf16-64", "adapter", "v2"])
def test_ragged_step_launches(kind, golden, monkeypatch):
    """A ragged step: today's sequence with c_attn as llj_norm_linear and llj_attention_ragged as the attention,
    n_layer times, plus llj_adapter_prefix_add on an adapter prefix layer; never llj_norm_qkv_rope."""
    m = model(kind, golden)
    sess = ragged_session(kind, LENGTHS, golden)
    calls = Calls(monkeypatch)
    sess.decode(1)
    v2 = "_v2" if kind == "v2" else ""
    n_layer = len(m.transformer.h)
    start = n_layer if kind == "bf16-64" else m.config.adapter_start_layer
    want = ["llj_embedding", "llj_rmsnorm_rows"]
    for i in range(n_layer):
        layer = _layer("llj_norm_linear", "llj_attention_ragged", ["llj_adapter_prefix_add"] if i >= start else [])
        want += [n + v2 if n in ("llj_norm_linear", "llj_linear_resid", "llj_norm_swiglu") else n for n in layer]
    want += ["llj_norm_linear" + v2, "llj_argmax"]
    assert calls.names == want, calls.names
    assert calls.count("llj_attention_ragged") == n_layer


@pytest.mark.parametrize("kind", ["int8", "fp32"])
def test_unsupported_models_raise_and_fall_back(kind):
    import generate as G
    from lit_llama.engine import DecodeSession

    m = model(kind)
    why = m.ragged_support()
    assert isinstance(why, str) and why
    prompts = prompts_of([3, 7, 5])
    sess = DecodeSession(m, 3, S, 7 + 6, use_graph=False)
    with pytest.raises(NotImplementedError) as e:
        sess.prefill_ragged(prompts)
    assert str(e.value) == why
    rows = G.generate_prompts(m, prompts, 6, top_k=1)
    for r, p in zip(rows, prompts):
        assert torch.equal(r, G.generate(m, p, 6, top_k=1))


def test_supported_models_give_no_reason(golden):
    for kind in ("bf16-64", "bf16-128", "int4", "adapter", "v2"):
        assert model(kind, golden).ragged_support() is None, kind


def test_session_argument_checks():
    from lit_llama.engine import DecodeSession

    m = model("bf16-64")
    prompts = prompts_of([3, 7, 5])
    with pytest.raises(ValueError):
        DecodeSession(m, 2, S, 13).prefill_ragged(prompts)  # 3 prompts, batch 2
    with pytest.raises(ValueError):
        DecodeSession(m, 3, S, 7).prefill_ragged(prompts)  # no room for one new token
    with pytest.raises(ValueError):
        DecodeSession(m, 3, 12, 13).prefill_ragged(prompts)  # the ring would wrap: total_len > S
    with pytest.raises(ValueError):
        DecodeSession(m, 3, S, 13).prefill_ragged(prompts[:2] + [prompts[2][:0]])  # an empty prompt


def test_main_prompts_file(tmp_path, capsys):
    """generate.py main with a prompts file on the word-level tokenizer set-up of test_generate_main_end_to_end:
    the texts on stdout in file order, one timing line on stderr."""
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
    texts = ["w3 w4 w5", "w9", "w10 w11 w12 w13 w14 w15 w16"]
    pf = tmp_path / "prompts.txt"
    pf.write_text("\n" + texts[0] + "\n\n" + texts[1] + "\n" + texts[2] + "\n\n")
    G.main("unused", max_new_tokens=10, checkpoint_path=ck, tokenizer_path=tmp_path / "tokenizer.json",
           prompts_file=pf)
    out, err = capsys.readouterr()
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 3, out
    for l, t in zip(lines, texts):
        assert l.startswith(f"<s> {t} ") and len(l.split()) >= 1 + len(t.split()) + 10 - 2, l
    assert err.count("tokens/sec") == 1 and "3 prompts" in err and "Time to load model" in err and "Memory used" in err
