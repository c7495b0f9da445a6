"""CPU tests of the host side of decoding prompts of different lengths as one batch (no GPU, no library): the
offsets and the left-padded token buffer of DecodeSession.prefill_ragged, output_rows' slicing, the decisions of
generate.generate_prompts to fall back to the per-prompt generate() loop, and --prompts_file parsing.
"""
import types

import pytest
import torch

from lit_llama import engine as E


def _prompts(lengths):
    return [torch.arange(10 * (b + 1), 10 * (b + 1) + t) for b, t in enumerate(lengths)]


def test_offsets_and_left_padded_layout():
    lengths = [1, 9, 4]
    tmax, off = E.ragged_layout(lengths)
    assert (tmax, off) == (9, [8, 0, 5])
    prompts = _prompts(lengths)
    total = tmax + 3
    tok = E.left_padded(prompts, total)
    assert tok.shape == (3, total) and tok.dtype == torch.int32
    for b, p in enumerate(prompts):
        assert torch.equal(tok[b, off[b]:tmax], p.to(torch.int32))
        assert not tok[b, :off[b]].any() and not tok[b, tmax:].any()
    # into a buffer of the session's: the same layout
    buf = torch.full((3, total), -1, dtype=torch.int32)
    assert E.left_padded(prompts, total, buf) is buf
    assert torch.equal(buf[:, tmax - 1], torch.tensor([10, 28, 33], dtype=torch.int32))
    assert torch.equal(buf[0, :8], torch.full((8,), -1, dtype=torch.int32))  # the padding is not written


def test_equal_lengths_have_no_padding():
    assert E.ragged_layout([5, 5]) == (5, [0, 0])
    assert E.ragged_layout([7]) == (7, [0])


@pytest.mark.parametrize("lengths", [[], [3, 0, 2]])
def test_empty_prompts_are_refused(lengths):
    with pytest.raises(ValueError):
        E.ragged_layout(lengths)


def test_output_rows_slicing():
    lengths = [1, 9, 4]
    tmax, off = E.ragged_layout(lengths)
    total = tmax + 5
    tok = E.left_padded(_prompts(lengths), total)
    tok[:, tmax:] = torch.arange(100, 100 + 3 * 5, dtype=torch.int32).view(3, 5)
    sess = E.DecodeSession.__new__(E.DecodeSession)  # the slicing alone: no device behind it
    sess.tokens, sess.offsets, sess.B, sess.t_prompt, sess.steps_done = tok, off, 3, tmax, 2
    rows = sess.output_rows()
    assert [r.numel() for r in rows] == [t + 2 for t in lengths]
    for b, (r, p) in enumerate(zip(rows, _prompts(lengths))):
        assert torch.equal(r[:lengths[b]], p.to(torch.int32))
        assert r[lengths[b]:].tolist() == [100 + 5 * b, 101 + 5 * b]
    assert torch.equal(sess.tokens[:, :tmax + 2], torch.stack([tok[b, :tmax + 2] for b in range(3)]))
    sess.offsets = None  # a session of equal-length prompts: the rows of output()
    assert [r.tolist() for r in sess.output_rows()] == tok[:, :tmax + 2].tolist()


class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, model, idx, max_new_tokens, **kw):
        self.calls.append((idx, max_new_tokens, kw))
        return torch.cat([idx, idx.new_full((max_new_tokens,), 7)])


def _fake_model(reason=None, block_size=64):
    return types.SimpleNamespace(config=types.SimpleNamespace(block_size=block_size), ragged_support=lambda: reason)


def _no_session(*a, **k):
    raise AssertionError("the batched route was taken")


@pytest.mark.parametrize("case", ["one prompt", "unsupported", "wrap", "wrap by block_size"])
def test_generate_prompts_falls_back_to_the_loop(case, monkeypatch):
    import generate as G

    rec = _Recorder()
    monkeypatch.setattr(G, "generate", rec)
    monkeypatch.setattr(G, "DecodeSession", _no_session)
    prompts, kw, model = _prompts([3, 9, 4]), {}, _fake_model()
    if case == "one prompt":
        prompts = prompts[:1]
    elif case == "unsupported":
        model = _fake_model("LLM.int8 Linears")
    elif case == "wrap":
        kw = {"max_seq_length": 12}  # 9 + 5 > 12
    else:
        model = _fake_model(block_size=13)  # the default max_seq_length = min(9 + 5, 13)
    out = G.generate_prompts(model, prompts, 5, temperature=0.7, top_k=3, eos_id=2, **kw)
    assert len(out) == len(prompts) == len(rec.calls)
    for (idx, n, passed), p, o in zip(rec.calls, prompts, out):
        assert idx is p and n == 5 and o.numel() == p.numel() + 5
        assert passed == {"max_seq_length": kw.get("max_seq_length"), "temperature": 0.7, "top_k": 3, "eos_id": 2}


def test_generate_prompts_takes_the_batch_when_it_can(monkeypatch):
    import generate as G

    rec = _Recorder()
    monkeypatch.setattr(G, "generate", rec)

    class Stop(Exception):
        pass

    def session(model, batch, max_seq_length, total_len, **kw):
        assert (batch, max_seq_length, total_len) == (3, 14, 14) and kw["top_k"] == 1 and kw["seed"] == 0
        raise Stop

    monkeypatch.setattr(G, "DecodeSession", session)
    with pytest.raises(Stop):
        G.generate_prompts(_fake_model(), _prompts([3, 9, 4]), 5, top_k=1)
    assert not rec.calls
    assert G.generate_prompts(_fake_model(), [], 5) == []


def test_prompts_file_parsing(tmp_path):
    import generate as G

    f = tmp_path / "prompts.txt"
    f.write_text("\nfirst prompt \n\n   \nsecond\n\tthird one\n\n", encoding="utf-8")
    assert G.read_prompts_file(f) == ["first prompt", "second", "third one"]
