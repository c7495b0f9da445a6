"""Text generation with the MI355X decode path — drop-in for reference generate.py.

`generate()` keeps the reference signature and semantics (generate.py:18-89): 1-D prompt,
`max_seq_length = min(T + max_new_tokens, block_size)` by default, temperature + top-k
sampling, EOS returns idx[:input_pos] (the EOS token itself is NOT included). Every decode
step runs as one captured HIP graph replay: greedy (top_k=1) ends in the argmax kernel, other
top_k / temperatures in the device top-k sampler.

`generate_samples()` (CLI: --batch_samples) produces the num_samples continuations of one prompt as one batch:
one prefill, every row its own draws, one decode step for all rows (DecodeSession.prefill_shared).

`generate_prompts()` (CLI: --prompts_file) continues several prompts of different lengths as one batch: each
prompt prefilled as generate() does it, then one decode step for all rows, every row at its own position
(DecodeSession.prefill_ragged). With packed_prefill=True (CLI: --packed_prefill) the prompts are also prefilled
as one batch of packed rows, every Linear's weights streamed once instead of once per prompt.

CLI flags follow reference generate.py:92-102 (argparse; jsonargparse is not installed).
The default CLI decode (top_k=200, temperature=0.8) runs the same captured graph as greedy, with
the device sampler (llj_sample) in place of the argmax.
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path
from typing import Optional

import torch

wd = Path(__file__).resolve().parent
sys.path.insert(0, str(wd))

from lit_llama import LLaMA, HFTokenizer  # noqa: E402
from lit_llama.checkpoint import read_checkpoint  # noqa: E402
from lit_llama.engine import DecodeSession  # noqa: E402
from lit_llama.utils import EmptyInitOnDevice, llama_model_lookup  # noqa: E402

EOS_CHECK_EVERY = 16  # greedy graph path: host looks at the ids once per 16 tokens


@torch.no_grad()
def generate(model: LLaMA, idx: torch.Tensor, max_new_tokens: int, *, max_seq_length: Optional[int] = None,
             temperature: float = 1.0, top_k: Optional[int] = None, eos_id: Optional[int] = None) -> torch.Tensor:
    """Takes a conditioning sequence (prompt) as input and continues to generate as many tokens as requested.

    Reference generate.py:18-89. Every decode step, greedy (top_k=1) or sampled, is one replay of
    the captured HIP graph; sampling draws its uniforms from a counter hash seeded from torch's
    default generator, so torch.manual_seed makes a run reproducible as in the reference."""
    T = idx.size(0)
    T_new = T + max_new_tokens
    if max_seq_length is None:
        max_seq_length = min(T_new, model.config.block_size)
    if max_new_tokens <= 0:
        return idx.clone()
    seed = 0 if top_k == 1 else int(torch.randint(0, 2 ** 62, (1,)))
    sess = DecodeSession(model, 1, max_seq_length, T_new, temperature=temperature, top_k=top_k, seed=seed)
    return _run_session(sess, idx, max_new_tokens, eos_id)


def _run_session(sess, idx, max_new_tokens, eos_id):
    T = idx.size(0)
    sess.prefill(idx.view(1, -1))
    left = max_new_tokens - 1
    while True:
        if eos_id is not None:
            gen = sess.output()[0, T:]
            hit = (gen == eos_id).nonzero()
            if hit.numel():  # the reference returns idx[:input_pos]: the EOS token is excluded
                return sess.output()[0, :T + int(hit[0, 0])].to(idx.dtype)
        if left == 0:
            break
        n = min(left, EOS_CHECK_EVERY) if eos_id is not None else left
        sess.decode(n)
        left -= n
    return sess.output()[0].to(idx.dtype)


@torch.no_grad()
def generate_batch(model: LLaMA, idx: torch.Tensor, max_new_tokens: int, *, max_seq_length: Optional[int] = None,
                   eos_id: Optional[int] = None):
    """Greedy decoding of B equal-length prompts (B, T) together (bs=8 throughput mode).
    Each row equals generate(model, idx[b], ..., top_k=1). Returns (B, T + max_new_tokens),
    or with eos_id a list of per-row tensors cut like the reference's EOS rule."""
    B, T = idx.shape
    T_new = T + max_new_tokens
    if max_seq_length is None:
        max_seq_length = min(T_new, model.config.block_size)
    sess = DecodeSession(model, B, max_seq_length, T_new)
    sess.prefill(idx)
    if max_new_tokens > 1:
        sess.decode(max_new_tokens - 1)
    out = sess.output().to(idx.dtype)
    if eos_id is None:
        return out
    rows = []
    for b in range(B):
        hit = (out[b, T:] == eos_id).nonzero()
        rows.append(out[b, :T + int(hit[0, 0])] if hit.numel() else out[b])
    return rows


@torch.no_grad()
def generate_samples(model: LLaMA, idx: torch.Tensor, num_samples: int, max_new_tokens: int, *,
                     max_seq_length: Optional[int] = None, temperature: float = 1.0, top_k: Optional[int] = None,
                     eos_id: Optional[int] = None) -> list:
    """num_samples continuations of one 1-D prompt as one batch: the prompt is prefilled once
    (DecodeSession.prefill_shared), every row draws its own tokens (the uniform of row b at position p is
    hash(seed, p, b), the seed drawn from torch's default generator as in generate()), and a decode step
    serves all rows. Returns a list of num_samples 1-D tensors, each cut by the reference's EOS rule (the EOS
    token itself excluded); with eos_id the host looks at the ids every EOS_CHECK_EVERY steps and stops once
    every row has one. top_k == 1 is greedy: all rows equal."""
    if num_samples < 1:
        raise ValueError(f"num_samples {num_samples} < 1")
    T = idx.size(0)
    T_new = T + max_new_tokens
    if max_seq_length is None:
        max_seq_length = min(T_new, model.config.block_size)
    if max_new_tokens <= 0:
        return [idx.clone() for _ in range(num_samples)]
    seed = 0 if top_k == 1 else int(torch.randint(0, 2 ** 62, (1,)))
    sess = DecodeSession(model, num_samples, max_seq_length, T_new, temperature=temperature, top_k=top_k, seed=seed)
    sess.prefill_shared(idx)
    left = max_new_tokens - 1
    while left:
        if eos_id is not None and bool((sess.output()[:, T:] == eos_id).any(dim=1).all()):
            break
        n = min(left, EOS_CHECK_EVERY) if eos_id is not None else left
        sess.decode(n)
        left -= n
    out = sess.output().to(idx.dtype)
    if eos_id is None:
        return list(out.unbind(0))
    rows = []
    for b in range(num_samples):
        hit = (out[b, T:] == eos_id).nonzero()
        rows.append(out[b, :T + int(hit[0, 0])] if hit.numel() else out[b])
    return rows


@torch.no_grad()
def generate_prompts(model: LLaMA, prompts, max_new_tokens: int, *, max_seq_length: Optional[int] = None,
                     temperature: float = 1.0, top_k: Optional[int] = None, eos_id: Optional[int] = None,
                     packed_prefill: bool = False) -> list:
    """Continuations of several 1-D prompts of any lengths as one batch (DecodeSession.prefill_ragged): every
    prompt is prefilled as generate() prefills it, then one decode step serves all rows, each at its own
    position. Returns one 1-D tensor per prompt, in order, each cut by the reference's EOS rule (the EOS token
    itself excluded); with eos_id the host looks at the ids every EOS_CHECK_EVERY steps and stops once every row
    has one. Sampling draws row b's uniform at step position p from hash(seed, p, b), p the position shared by
    the batch (the longest prompt's), the seed from torch's default generator as in generate().
    max_seq_length defaults to min(Tmax + max_new_tokens, block_size), Tmax the longest prompt. The prompts run
    one after the other through generate(), as before this function existed, when there is only one, when
    model.ragged_support() names a reason (LLM.int8, unmerged LoRA, fp32 / any-shape models), or when
    Tmax + max_new_tokens exceeds max_seq_length (the batch's caches do not wrap).
    packed_prefill: the batch's prompts are prefilled as one run over their sum T_b packed rows instead of one
    after the other (DecodeSession.prefill_ragged(packed=True); the per-prompt loop where
    model.packed_prefill_support() names a reason, fewer than 32 tokens in all among them). The two prefills agree
    to rounding, not bitwise."""
    prompts = list(prompts)
    if not prompts:
        return []
    lens = [int(p.size(0)) for p in prompts]
    tmax = max(lens)
    msl = min(tmax + max_new_tokens, model.config.block_size) if max_seq_length is None else max_seq_length
    if len(prompts) == 1 or tmax + max_new_tokens > msl or model.ragged_support() is not None:
        return [generate(model, p, max_new_tokens, max_seq_length=max_seq_length, temperature=temperature,
                         top_k=top_k, eos_id=eos_id) for p in prompts]
    if max_new_tokens <= 0:
        return [p.clone() for p in prompts]
    seed = 0 if top_k == 1 else int(torch.randint(0, 2 ** 62, (1,)))
    sess = DecodeSession(model, len(prompts), msl, tmax + max_new_tokens, temperature=temperature, top_k=top_k,
                         seed=seed)
    sess.prefill_ragged(prompts, packed=packed_prefill)
    left = max_new_tokens - 1
    while left:
        if eos_id is not None and bool((sess.output()[:, tmax:] == eos_id).any(dim=1).all()):
            break
        n = min(left, EOS_CHECK_EVERY) if eos_id is not None else left
        sess.decode(n)
        left -= n
    rows = []
    for row, p in zip(sess.output_rows(), prompts):
        row = row.to(p.dtype)
        if eos_id is not None:
            hit = (row[p.size(0):] == eos_id).nonzero()
            if hit.numel():
                row = row[:p.size(0) + int(hit[0, 0])]
        rows.append(row)
    return rows


def read_prompts_file(path) -> list:
    """The prompts of --prompts_file: one per non-empty line, in file order."""
    with open(path, encoding="utf-8") as f:
        return [line.strip() for line in f if line.strip()]


def main(prompt: str = "Hello, my name is", *, num_samples: int = 1, max_new_tokens: int = 50, top_k: int = 200,
         temperature: float = 0.8, checkpoint_path: Path = Path("checkpoints/lit-llama/7B/lit-llama.pth"),
         tokenizer_path: Path = Path("checkpoints/lit-llama/tokenizer.model"), quantize: Optional[str] = None,
         batch_samples: bool = False, prompts_file: Optional[Path] = None, packed_prefill: bool = False) -> None:
    """Generates text samples based on a pre-trained LLaMA model and tokenizer (reference generate.py:92-155).
    batch_samples: the num_samples samples as one batch (generate_samples) instead of one after the other.
    prompts_file: one prompt per non-empty line instead of `prompt`, all generated as one batch
    (generate_prompts), the texts printed in file order; packed_prefill: their prompts prefilled as one packed
    batch as well (it means nothing without prompts_file)."""
    assert checkpoint_path.is_file(), checkpoint_path
    assert tokenizer_path.is_file(), tokenizer_path
    if not torch.cuda.is_available():
        raise SystemExit("this generate.py runs on a ROCm GPU (MI355X) only")
    print("Loading model ...", file=sys.stderr)
    t0 = time.time()
    checkpoint = read_checkpoint(checkpoint_path)  # weights only, memory-mapped (incremental_save files too)
    name = llama_model_lookup(checkpoint)
    with EmptyInitOnDevice(device=torch.device("cuda"), dtype=torch.bfloat16, quantization_mode=quantize):
        model = LLaMA.from_name(name)
    model.load_state_dict(checkpoint)
    del checkpoint
    print(f"Time to load model: {time.time() - t0:.02f} seconds.", file=sys.stderr)
    model.eval()
    tokenizer = HFTokenizer(tokenizer_path)
    encoded = tokenizer.encode(prompt, bos=True, eos=False, device=torch.device("cuda"))
    prompt_length = encoded.size(0)
    torch.manual_seed(1234)
    if prompts_file is not None:
        dev = torch.device("cuda")
        enc = [tokenizer.encode(text, bos=True, eos=False, device=dev) for text in read_prompts_file(prompts_file)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ys = generate_prompts(model, enc, max_new_tokens, temperature=temperature, top_k=top_k,
                              packed_prefill=packed_prefill)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        model.reset_cache()
        for y in ys:
            print(tokenizer.decode(y))
        tokens_generated = sum(y.size(0) - e.size(0) for y, e in zip(ys, enc))
        print(f"Time for inference of {len(enc)} prompts: {t:.02f} sec total, {tokens_generated / t:.02f} tokens/sec",
              file=sys.stderr)
        print(f"Memory used: {torch.cuda.max_memory_reserved() / 1e9:.02f} GB", file=sys.stderr)
        return
    if batch_samples:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ys = generate_samples(model, encoded, num_samples, max_new_tokens, temperature=temperature, top_k=top_k)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        model.reset_cache()
        for y in ys:
            print(tokenizer.decode(y))
        tokens_generated = sum(y.size(0) - prompt_length for y in ys)
        print(f"Time for inference of {num_samples} samples: {t:.02f} sec total, {tokens_generated / t:.02f} tokens/sec",
              file=sys.stderr)
        print(f"Memory used: {torch.cuda.max_memory_reserved() / 1e9:.02f} GB", file=sys.stderr)
        return
    for i in range(num_samples):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y = generate(model, encoded, max_new_tokens, temperature=temperature, top_k=top_k)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        model.reset_cache()
        print(tokenizer.decode(y))
        tokens_generated = y.size(0) - prompt_length
        print(f"Time for inference {i + 1}: {t:.02f} sec total, {tokens_generated / t:.02f} tokens/sec", file=sys.stderr)
    print(f"Memory used: {torch.cuda.max_memory_reserved() / 1e9:.02f} GB", file=sys.stderr)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="Generates text samples based on a pre-trained LLaMA model and tokenizer.")
    ap.add_argument("--prompt", default="Hello, my name is")
    ap.add_argument("--num_samples", type=int, default=1)
    ap.add_argument("--max_new_tokens", type=int, default=50)
    ap.add_argument("--top_k", type=int, default=200)
    ap.add_argument("--temperature", type=float, default=0.8)
    ap.add_argument("--checkpoint_path", type=Path, default=Path("checkpoints/lit-llama/7B/lit-llama.pth"))
    ap.add_argument("--tokenizer_path", type=Path, default=Path("checkpoints/lit-llama/tokenizer.model"))
    ap.add_argument("--quantize", default=None, choices=[None, "llm.int8", "gptq.int4", "gptq.int8"])
    ap.add_argument("--batch_samples", action="store_true",
                    help="generate the num_samples samples as one batch: the prompt is prefilled once")
    ap.add_argument("--prompts_file", type=Path, default=None,
                    help="a file with one prompt per non-empty line, replacing --prompt: all lines are generated as "
                         "one batch, whatever their lengths, and printed in file order")
    ap.add_argument("--packed_prefill", action="store_true",
                    help="with --prompts_file: prefill all prompts as one packed batch, every weight streamed once, "
                         "instead of one prompt after the other")
    a = ap.parse_args()
    main(a.prompt, num_samples=a.num_samples, max_new_tokens=a.max_new_tokens, top_k=a.top_k,
         temperature=a.temperature, checkpoint_path=a.checkpoint_path, tokenizer_path=a.tokenizer_path,
         quantize=a.quantize, batch_samples=a.batch_samples, prompts_file=a.prompts_file,
         packed_prefill=a.packed_prefill)
