"""bench.py's timed decode and its --dump-outputs files on a 2-layer model: the dumped arrays are
what a caller of the timed path holds after the last timed step (ids so far, last logits), float32,
identical from run to run; --steps really is the number of timed steps, also when they do not fit
one session (block_size positions) and run as several sessions of the same prompts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BLOCK, S, T_PROMPT, WARMUP = 128, 64, 16, 2


def _model():
    from lit_llama import LLaMA, LLaMAConfig
    from lit_llama.utils import EmptyInitOnDevice

    dev = torch.device("cuda")
    with EmptyInitOnDevice(device=dev, dtype=torch.bfloat16):
        m = LLaMA(LLaMAConfig(block_size=BLOCK, vocab_size=2048, n_layer=2, n_head=4, n_embd=256))
    g = torch.Generator(device=dev).manual_seed(5)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.Linear):
                mod.weight.normal_(0.0, 1.0 / mod.in_features ** 0.5, generator=g)
            elif isinstance(mod, torch.nn.Embedding):
                mod.weight.normal_(0.0, 1.0, generator=g)
        for blk in m.transformer.h:
            blk.rms_1.scale.fill_(1.0)
            blk.rms_2.scale.fill_(1.0)
        m.transformer.ln_f.scale.fill_(1.0)
    return m.eval()


def _timed_and_dumped(bench, model, steps, out_dir):
    r = bench.time_decode(model, 1, T_PROMPT, S, WARMUP, steps, 1)
    bench.dump_outputs(r["session"], out_dir)
    return r, np.load(out_dir / "tokens.npy"), np.load(out_dir / "logits.npy")


@pytest.mark.parametrize("steps", [5, 150])  # one session; two sessions (109 + 41 timed steps)
def test_dump_outputs_are_the_timed_decodes_last_step(tmp_path, steps):
    import bench
    from lit_llama.engine import DecodeSession

    model = _model()
    skip = bench.untimed_steps(T_PROMPT, S, WARMUP, steps)
    seg_cap = BLOCK - (T_PROMPT + 1 + skip)
    last = steps % seg_cap or seg_cap  # timed steps of the last session
    r, tok, log = _timed_and_dumped(bench, model, steps, tmp_path / "a")
    assert r["tokens"] == steps and r["seconds"] > 0.0
    assert r["session"].steps_done == 1 + skip + last
    assert tok.dtype == np.float32 and log.dtype == np.float32
    assert tok.shape == (1, T_PROMPT + 1 + skip + last) and log.shape == (1, model.config.padded_vocab_size)
    assert np.isfinite(log).all()

    # the same prompts through a session of the caller's own: same ids, same last logits
    prompts = torch.randint(3, model.config.vocab_size, (1, T_PROMPT), generator=torch.Generator().manual_seed(1234))
    assert np.array_equal(tok[0, :T_PROMPT], prompts[0].numpy().astype(np.float32))
    sess = DecodeSession(model, 1, S, tok.shape[1])
    sess.prefill(prompts.cuda())
    sess.decode(skip + last)
    torch.cuda.synchronize()
    assert np.array_equal(tok, sess.output().cpu().numpy().astype(np.float32))
    assert np.array_equal(log, sess.logits.float().cpu().numpy())
    assert log[0, int(tok[0, -1])] == log[0].max()  # the last id is the greedy choice from those logits

    # identical inputs from run to run: a second timed run dumps the same arrays
    _, tok2, log2 = _timed_and_dumped(bench, model, steps, tmp_path / "b")
    assert np.array_equal(tok, tok2) and np.array_equal(log, log2)
