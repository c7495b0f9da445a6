"""One prompt sampled B times as one batch (GPU): DecodeSession.prefill_shared, the shared-prefix decode attention
route behind model.SHARED_PREFIX_MIN, generate.generate_samples and generate.main(batch_samples=True).

Sessions are driven with forced tokens, so that a last-bit difference between two routes cannot change the
sequence: use_graph=False, and before every decode(1) row-distinct tokens from a fixed random (B, n) table are
copied into sess.cur; sess.logits is read after the step. The comparison is the existing code: a DecodeSession
that prefills the prompt repeated B times. Bound: max |dlogits| <= 3e-2 max |ref| at every step, the bound
test_long_cache_split_attention_decode uses for swapping attention routes.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import llama_np as O
from oracle.weights import Cfg, make_params
from tests.test_model_gpu import build

pytestmark = pytest.mark.gpu

CFGS = {
    64: Cfg(block_size=128, n_layer=2, n_head=4, n_embd=256, vocab_size=2048),
    128: Cfg(block_size=128, n_layer=2, n_head=2, n_embd=256, vocab_size=2048),
}
B, T, STEPS = 8, 9, 12
S, TOTAL = 32, T + 1 + STEPS
BOUND = 3e-2


def _prompt():
    return torch.randint(3, 2048, (T,), generator=torch.Generator().manual_seed(11)).cuda()


def _forced():
    return torch.randint(3, 2048, (B, STEPS), generator=torch.Generator().manual_seed(12)).to(torch.int32).cuda()


@functools.lru_cache(maxsize=None)
def model(hs, kind="bf16"):
    cfg = CFGS[hs]
    params = make_params(cfg, 7)
    if kind == "fp32":
        from tests.test_fp32_gpu import build32

        return build32(cfg, params)
    return build(cfg, params, mode="llm.int8" if kind == "int8" else None)


def drive(sess, steps, rows=B):
    """logits after the prefill and after each forced step: (steps + 1, rows, V) float32"""
    forced = _forced()
    torch.cuda.synchronize()
    out = [sess.logits.float().cpu().numpy()]
    for s in range(steps):
        sess.cur.copy_(forced[:rows, s])
        sess.decode(1)
        torch.cuda.synchronize()
        out.append(sess.logits.float().cpu().numpy())
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def reference(hs, kind="bf16", s=S, total=TOTAL, steps=STEPS, rows=B):
    """The existing code: prefill of the prompt repeated `rows` times, then the forced steps. Computed once per
    case and left unchanged."""
    from lit_llama.engine import DecodeSession

    sess = DecodeSession(model(hs, kind), rows, s, total, use_graph=False)
    sess.prefill(_prompt().repeat(rows, 1))
    assert sess.work.shared_prefix == 0
    ref = drive(sess, steps, rows)
    ref.setflags(write=False)
    return ref


def shared_session(hs, kind="bf16", s=S, total=TOTAL, **kw):
    from lit_llama.engine import DecodeSession

    sess = DecodeSession(model(hs, kind), B, s, total, **{"use_graph": False, **kw})
    sess.prefill_shared(_prompt())
    return sess


def check(got, ref, what):
    for s in range(len(ref)):
        d, scale = np.abs(got[s] - ref[s]).max(), np.abs(ref[s]).max()
        print(f"[{what}] step {s}: max |dlogits| {d:.4g} = {d / scale:.3e} of max |ref| {scale:.4g}")
    for s in range(len(ref)):
        assert np.abs(got[s] - ref[s]).max() <= BOUND * np.abs(ref[s]).max(), (what, s)


@pytest.mark.parametrize("hs", [64, 128])
def test_repeated_prompt_row_0_agrees_with_batch_1(hs):
    """The comparison session prefills 8 x 9 rows and the shared one 9 (other prefill kernels): row 0 of the
    repeated-prompt session agrees with a B = 1 session within the bound for these seeds."""
    ref = reference(hs)
    one = reference(hs, rows=1)
    check(one[:, :1], ref[:, :1], f"B=1 vs row 0 of B=8, hs {hs}")


@pytest.mark.parametrize("hs", [64, 128])
def test_shared_route_matches_repeated_prompt_session(hs, monkeypatch):
    from lit_llama import model as MD

    monkeypatch.setattr(MD, "SHARED_PREFIX_MIN", 1)
    ref = reference(hs)  # (first: a model holds one session's caches at a time)
    sess = shared_session(hs)
    assert sess.work.shared_prefix == T and sess.work.shared_ws is not None
    assert (sess.t_prompt, sess.steps_done, int(sess.pos.item())) == (T, 1, T - 1)
    check(drive(sess, STEPS), ref, f"shared route, hs {hs}")


@pytest.mark.parametrize("hs", [64, 128])
def test_copy_route_matches_repeated_prompt_session(hs, monkeypatch):
    from lit_llama import model as MD

    monkeypatch.setattr(MD, "SHARED_PREFIX_MIN", S + 1)
    ref = reference(hs)
    sess = shared_session(hs)
    assert sess.work.shared_prefix == 0
    check(drive(sess, STEPS), ref, f"copy route, hs {hs}")


@pytest.mark.parametrize("hs", [64, 128])
def test_caches_after_prefill_shared(hs, monkeypatch):
    """Every row holds row 0's T prompt slots bitwise; the slots from T on are zero."""
    from lit_llama import model as MD

    monkeypatch.setattr(MD, "SHARED_PREFIX_MIN", 1)
    sess = shared_session(hs)
    caches = sess.model.kv_caches
    assert len(caches) == CFGS[hs].n_layer
    for kc, vc in caches:
        for c in (kc, vc):
            assert c.shape == (B, CFGS[hs].n_head, S, hs)
            bits = c.view(torch.int16)
            assert bits[0, :, :T].ne(0).any()
            for b in range(B):
                assert torch.equal(bits[b, :, :T], bits[0, :, :T])
            assert not bits[:, :, T:].any()


def test_first_step_draws_are_per_row(monkeypatch):
    """The B first tokens come from one row of logits and the rows' own uniforms (uniforms[T, b]: the token at
    position T): each equals the host restatement of the sampler rule on that row of logits at its uniform, and
    the uniforms are spread so that these differ."""
    from lit_llama import model as MD

    monkeypatch.setattr(MD, "SHARED_PREFIX_MIN", 1)
    table = torch.zeros(TOTAL, B, dtype=torch.float32, device="cuda")
    u = (np.arange(B, dtype=np.float32) + 0.5) / B
    table[T] = torch.from_numpy(u).cuda()
    sess = shared_session(64, temperature=1.0, top_k=None, uniforms=table)
    torch.cuda.synchronize()
    logits = sess.logits.float().cpu().numpy()
    assert (logits == logits[0]).all()
    want = [O.sample_inverse_cdf(logits[0], 1.0, None, float(u[b]))[0] for b in range(B)]
    assert len(set(want)) > 1, want
    got = sess.output()[:, T].cpu().numpy()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(sess.cur.cpu().numpy(), want)
    np.testing.assert_array_equal(sess.output()[:, :T].cpu().numpy(), _prompt().cpu().numpy()[None].repeat(B, 0))


@pytest.mark.parametrize("kind", ["int8", "fp32", "wrap"])
def test_models_that_take_the_copy_route(kind, monkeypatch):
    """An LLM.int8 model (its attention hands statistics to c_proj), an fp32 model (any-shape kernels) and a
    session whose ring wraps (total_len > S) decode from the copied caches with the existing attention."""
    from lit_llama import model as MD

    monkeypatch.setattr(MD, "SHARED_PREFIX_MIN", 1)
    s, k = (12, "bf16") if kind == "wrap" else (S, kind)  # 12 slots: the 4 steps reach position 12 = slot 0
    ref = reference(64, k, s=s, steps=4)
    sess = shared_session(64, k, s=s)
    assert sess.work.shared_prefix == 0
    check(drive(sess, 4), ref, f"copy route, {kind}")


def test_graph_and_eager_sessions_give_the_same_ids(monkeypatch):
    from lit_llama import model as MD

    monkeypatch.setattr(MD, "SHARED_PREFIX_MIN", 1)
    table = torch.rand(TOTAL, B, generator=torch.Generator().manual_seed(5)).cuda()
    outs = []
    for graph in (False, True):
        sess = shared_session(128, use_graph=graph, temperature=0.8, top_k=50, uniforms=table)
        assert sess.work.shared_prefix == T
        sess.decode(STEPS)
        torch.cuda.synchronize()
        outs.append(sess.output().cpu().numpy())
    assert outs[0].shape == (B, TOTAL)
    np.testing.assert_array_equal(outs[0], outs[1])
    assert len({tuple(r) for r in outs[0]}) > 1  # the rows are different samples


@pytest.mark.parametrize("shared", [True, False])
def test_generate_samples(shared, monkeypatch):
    import generate as G
    from lit_llama import model as MD

    monkeypatch.setattr(MD, "SHARED_PREFIX_MIN", 1 if shared else 10 ** 9)
    m, prompt, n = model(64), _prompt(), 20
    runs = []
    for seed in (1234, 1234, 99):
        torch.manual_seed(seed)
        runs.append(G.generate_samples(m, prompt, 5, n, temperature=0.8, top_k=200))
    for rows in runs:
        assert isinstance(rows, list) and len(rows) == 5
        for r in rows:
            assert r.dtype == prompt.dtype and r.shape == (T + n,) and torch.equal(r[:T], prompt)
            assert bool(((r >= 0) & (r < 2048)).all())
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    assert any(not torch.equal(a, b) for a, b in zip(runs[0], runs[2]))
    assert len({tuple(r.tolist()) for r in runs[0]}) > 1
    # EOS: a token of row 0's continuation; every row is cut before its first occurrence
    eos = int(runs[0][0][T + 4])
    torch.manual_seed(1234)
    cut = G.generate_samples(m, prompt, 5, n, temperature=0.8, top_k=200, eos_id=eos)
    assert len(cut) == 5 and cut[0].shape[0] <= T + 4
    for full, c in zip(runs[0], cut):
        hit = (full[T:] == eos).nonzero()
        want = full[:T + int(hit[0, 0])] if hit.numel() else full
        assert torch.equal(c, want)
    # one sample; greedy rows are all equal
    torch.manual_seed(1234)
    one = G.generate_samples(m, prompt, 1, n, temperature=0.8, top_k=200)
    assert len(one) == 1 and one[0].shape == (T + n,)
    greedy = G.generate_samples(m, prompt, 3, n, top_k=1)
    assert all(torch.equal(g, greedy[0]) for g in greedy)


def test_main_batch_samples(tmp_path, capsys):
    """generate.py main with batch_samples on the word-level tokenizer set-up of test_generate_main_end_to_end:
    the 3 samples on stdout, one timing line on stderr."""
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
    G.main("w3 w4 w5", num_samples=3, max_new_tokens=10, checkpoint_path=ck, tokenizer_path=tmp_path / "tokenizer.json",
           batch_samples=True)
    out, err = capsys.readouterr()
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 3, out
    for l in lines:
        assert l.startswith("<s> w3 w4 w5 ") and len(l.split()) >= 4 + 10 - 2, l
    assert err.count("tokens/sec") == 1 and "Time to load model" in err and "Memory used" in err
