"""Decode session: the reference's token loop (generate.py:61-87) with the per-token work
captured once into a HIP graph.

One decode step = embedding of the current token (which also advances the device-side
position), the n_layer fused blocks, ln_f + lm_head and the next-token choice -- the greedy
argmax (top_k = 1) or the temperature / top-k sampler (llj_sample, generate.py:66-74; its
uniform comes from a counter hash of (seed, position, row), or from a caller's table of
uniforms per position) -- which writes the next token both into `cur` and into the output id
buffer. Nothing in the step reads the host, so replaying the graph K times generates K tokens
with no host round trip (the reference syncs per layer at model.py:221 and per token at
generate.py:86).

Batch B > 1 decodes B equal-length prompts together (each row equals an independent B=1
run: tests/test_model_gpu.py); the reference's generate() is batch 1 only (generate.py:62). Up to 8
rows share every fused launch; larger batches take the ops in row slices. Prompts of different
lengths decode together after prefill_ragged: the step position stays shared, each row's own position
is pos - off[b], and c_attn's plain store + llj_attention_ragged replace the fused c_attn epilogue and
the decode attention. prefill_ragged(packed=True) also prefills them as one batch of packed
rows.
"""
from __future__ import annotations

import torch

from . import _hip
from . import model as _model
from .model import LLaMA, _Work


def ragged_layout(lengths) -> tuple:
    """(Tmax, off) of prompts of these lengths decoded as one batch (prefill_ragged): off[b] = Tmax - T_b, the
    padding on the left of row b in the token buffer and the distance of row b's own position from the shared
    step position."""
    lengths = [int(t) for t in lengths]
    if not lengths or min(lengths) < 1:
        raise ValueError(f"every prompt needs at least one token, got lengths {lengths}")
    tmax = max(lengths)
    return tmax, [tmax - t for t in lengths]


PACKED_QUERIES = 64  # queries per workgroup of llj_attention_prefill_packed


def packed_layout(lengths) -> tuple:
    """(cu, tiles) of prompts of these lengths prefilled as one packed batch (prefill_ragged(packed=True)): cu[b] is
    the first of prompt b's rows in the M = cu[B] packed rows; tiles lists every (b, qb), the 64-query block qb of
    prompt b, by descending key count min(T_b, 64 qb + 64) -- the causal attention's work per block, so the long
    blocks start first -- with ties in (b, qb) order."""
    lengths = [int(t) for t in lengths]
    if not lengths or min(lengths) < 1:
        raise ValueError(f"every prompt needs at least one token, got lengths {lengths}")
    cu = [0]
    for t in lengths:
        cu.append(cu[-1] + t)
    Q = PACKED_QUERIES
    tiles = [(b, qb) for b, t in enumerate(lengths) for qb in range((t + Q - 1) // Q)]
    tiles.sort(key=lambda bq: (-min(lengths[bq[0]], Q * bq[1] + Q), bq))
    return cu, tiles


def left_padded(prompts, total_len: int, tokens: torch.Tensor | None = None) -> torch.Tensor:
    """The (B, total_len) int32 token buffer of a ragged session: row b's prompt in columns off[b] .. Tmax - 1
    (zeros on its left), so that every row's new tokens start at column Tmax. Fills `tokens` if given."""
    tmax, off = ragged_layout([p.numel() for p in prompts])
    if tokens is None:
        tokens = torch.zeros(len(prompts), total_len, dtype=torch.int32, device=prompts[0].device)
    for b, p in enumerate(prompts):
        tokens[b, off[b]:tmax] = p.reshape(-1).to(device=tokens.device, dtype=torch.int32)
    return tokens


def rows_of(tokens: torch.Tensor, off, end: int) -> list:
    """Row b of a left-padded token buffer without its padding: tokens[b, off[b]:end]."""
    return [tokens[b, o:end] for b, o in enumerate(off)]


class DecodeSession:
    def __init__(self, model: LLaMA, batch: int, max_seq_length: int, total_len: int, use_graph: bool = True,
                 temperature: float = 1.0, top_k: int | None = 1, seed: int = 0,
                 uniforms: torch.Tensor | None = None):
        """top_k == 1: greedy; otherwise sampling at `temperature` over the top_k logits (None:
        all). uniforms: optional (total_len, batch) fp32 device table, row p = the uniforms of the
        token at position p (tests replay a reference run's draws)."""
        cfg = model.config
        assert max_seq_length <= cfg.block_size
        self.model, self.B, self.S, self.total = model, batch, max_seq_length, total_len
        dev = model.transformer.wte.weight.device
        _hip.require_device(model.transformer.wte.weight, "model")
        self.dev = dev
        if batch < 1:
            raise ValueError(f"decode batch {batch} < 1")
        # batches past QKV_ROWS (8) run every fused op in row slices of 8 (16 for the plain linears)
        self.cur = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.pos = torch.zeros(1, dtype=torch.int32, device=dev)
        self.tokens = torch.zeros(batch, total_len, dtype=torch.int32, device=dev)
        self.logits = torch.empty(batch, cfg.padded_vocab_size, dtype=model.act_dtype(), device=dev)
        self.use_graph = use_graph
        self.graph = None
        self.t_prompt = 0
        self.steps_done = 0
        self.specs = None
        self.work = None
        self.packed_prefill = False  # prefill_ragged(packed=True) ran the prompts as one packed batch
        self.off = None       # prefill_ragged: (B,) int32 on the device, row b stands at pos - off[b]
        self.offsets = None   # ... and the same as a host list
        self.temperature = float(temperature)
        self.top_k = 0 if top_k is None else int(top_k)
        self.seed = int(seed) & ((1 << 64) - 1)
        if uniforms is not None:
            assert uniforms.dtype == torch.float32 and uniforms.shape == (total_len, batch) and uniforms.is_contiguous()
            _hip.require_device(uniforms, "uniforms")
        self.uniforms = uniforms

    def _choose(self, st):
        """next token of every row from self.logits -> cur and tokens[:, pos + 1]"""
        cfg = self.model.config
        if self.logits.dtype == torch.float32 and self.top_k != 1:  # the fp32 model: sampled in fp32
            _hip.call("llj_g_sample", self.logits.data_ptr(), self.logits.stride(0), self.B, cfg.padded_vocab_size,
                      self.temperature, self.top_k, _hip.ptr(self.uniforms), self.seed, self.cur.data_ptr(),
                      self.tokens.data_ptr(), self.total, self.pos.data_ptr(), st)
        elif self.logits.dtype == torch.float32:
            _hip.call("llj_g_argmax", self.logits.data_ptr(), self.logits.stride(0), self.B, cfg.padded_vocab_size,
                      self.cur.data_ptr(), self.tokens.data_ptr(), self.total, self.pos.data_ptr(), st)
        elif self.top_k == 1:
            _hip.call("llj_argmax", self.logits.data_ptr(), self.logits.stride(0), self.B, cfg.padded_vocab_size,
                      self.cur.data_ptr(), self.tokens.data_ptr(), self.total, self.pos.data_ptr(), st)
        else:
            _hip.call("llj_sample", self.logits.data_ptr(), self.logits.stride(0), self.B, cfg.padded_vocab_size,
                      self.temperature, self.top_k, _hip.ptr(self.uniforms), self.seed, self.cur.data_ptr(),
                      self.tokens.data_ptr(), self.total, self.pos.data_ptr(), st)

    # -- prefill: eager (rows = B*T); fills the caches, picks the first new token
    @torch.no_grad()
    def prefill(self, prompts: torch.Tensor) -> None:
        m = self.model
        B, T = prompts.shape
        assert B == self.B and T + 1 <= self.total
        m.reset_cache()
        m.kv_caches = m._alloc_kv(B, self.S, self.dev)
        if m.rope_cache is None:
            m.rope_cache = m.build_rope_cache(prompts)
        pos = torch.arange(T, device=self.dev, dtype=torch.int32)
        m._run(prompts.to(self.dev), pos, self.S, m.kv_caches, last_only_out=self.logits)
        st = _hip.stream()
        self.tokens[:, :T] = prompts.to(torch.int32)
        self.pos.fill_(T - 1)
        self._choose(st)
        self.t_prompt = T
        self.steps_done = 1
        self._setup_work()

    def _setup_work(self, shared_prefix: int = 0, ragged: bool = False) -> None:
        """decode-step operands (fixed for the session); shared_prefix: see prefill_shared; ragged: see
        prefill_ragged (which has checked model.ragged_support())"""
        m, B = self.model, self.B
        self.specs = m._layer_specs()
        if ragged:
            self.work = _Work(m.config, B, self.dev, False, self.S, ragged=True)
            self.work.off = self.off
            self.graph = None
            return
        self.off = self.offsets = None
        if m._generic():  # the any-shape kernels (csrc/generic.hip)
            self.work = _Work(m.config, B, self.dev, False, self.S, generic=True, dtype=m.act_dtype(),
                              lora_cols=self.specs.get("lora_cols", 0))
        else:
            need_i8 = any(s[0] == 2 for layer in self.specs["layers"] for s in layer) or self.specs["head"][0] == 2
            self.work = _Work(m.config, B, self.dev, need_i8, self.S, lora_cols=self.specs.get("lora_cols", 0),
                              shared_prefix=shared_prefix)
            m._enable_i8_handoff(self.work, self.specs)
            if self.work.i8s:  # the attention is llj_attention_i8 (it hands y's statistics on): no shared route
                self.work.shared_prefix, self.work.shared_ws = 0, None
        self.graph = None  # the caches / operands may have changed

    @torch.no_grad()
    def prefill_shared(self, prompt: torch.Tensor) -> None:
        """prefill() for one prompt (1-D or (1, T)) that all B rows continue: the prompt runs once, as one row,
        into row 0 of the caches; its T slots are copied to the other rows and its last-position logits to
        all B rows of self.logits, from which every row draws its own first token (row b with hash(seed, pos,
        b) or uniforms[T, b]). The caches then hold what prefill(prompt.repeat(B, 1)) leaves up to the
        row count of the prefill launches, so every model kind decodes from them. Where the per-row decode
        attention would be llj_attention / llj_attention_split (streaming kernels, bf16; not an adapter
        prefix layer, the LLM.int8 hand-off or ATT_MERGE), the ring cannot wrap (total_len <= S) and
        T >= model.SHARED_PREFIX_MIN, the decode steps run llj_attention_shared instead, which reads the
        prompt's keys and values from row 0 only: work.shared_prefix = T, else 0."""
        m, B = self.model, self.B
        prompt = prompt.reshape(1, -1)
        T = prompt.shape[1]
        assert T >= 1 and T + 1 <= self.total
        m.reset_cache()
        m.kv_caches = m._alloc_kv(B, self.S, self.dev)
        if m.rope_cache is None:
            m.rope_cache = m.build_rope_cache(prompt)
        pos = torch.arange(T, device=self.dev, dtype=torch.int32)
        row0 = [(kc[:1], vc[:1]) for kc, vc in m.kv_caches]  # contiguous views: a one-row cache
        m._run(prompt.to(self.dev), pos, self.S, row0, last_only_out=self.logits[:1])
        if B > 1:
            # token t lives in slot t % S; a prompt longer than the ring fills every slot
            n = min(T, self.S)
            for kc, vc in m.kv_caches:
                kc[1:, :, :n] = kc[:1, :, :n]
                vc[1:, :, :n] = vc[:1, :, :n]
            self.logits[1:] = self.logits[:1]
        st = _hip.stream()
        self.tokens[:, :T] = prompt.to(torch.int32)
        self.pos.fill_(T - 1)
        self._choose(st)
        self.t_prompt = T
        self.steps_done = 1
        shared = T if (self.total <= self.S and T >= _model.SHARED_PREFIX_MIN) else 0
        self._setup_work(shared)

    @torch.no_grad()
    def prefill_ragged(self, prompts, packed: bool = False) -> None:
        """prefill() for B prompts of different lengths (a list of 1-D tensors, T_b >= 1 tokens each) that then
        decode as one batch. With Tmax = max T_b and off[b] = Tmax - T_b:
          * row b is prefilled exactly as a B = 1 session prefills it, into row b of the caches (slot p holds
            its token at its own position p) and row b of self.logits: bitwise a B = 1 session's;
          * the token buffer is left-padded: row b's prompt in tokens[b, off[b]:Tmax], every row's new tokens
            from column Tmax on (output_rows() drops the padding);
          * the step position stays the one device int `pos` (Tmax - 1 after the prefill, advanced by the
            embedding launch); row b's own position is pos - off[b], which only llj_attention_ragged needs
            (RoPE angle, cache slot, key count). The samplers' counter hash (seed, pos, row) and a `uniforms`
            table are indexed by the shared step position, not by the row's own.
        The ring must not wrap: Tmax + 1 <= total_len <= S. Raises NotImplementedError with the reason where
        model.ragged_support() gives one. t_prompt = Tmax, so decode()'s bounds hold unchanged.
        packed=True: the B prompts are prefilled as one batch of M = sum T_b packed rows (LLaMA._run_packed: every
        Linear streams its weights once instead of B times) where model.packed_prefill_support(M) gives no reason,
        and one after the other as above where it does. The packed rows run other GEMM kernels than a T_b-row
        prefill, so its logits and K / V agree with the loop's to a tolerance, not bitwise. self.packed_prefill
        records which route ran."""
        m, B = self.model, self.B
        if len(prompts) != B:
            raise ValueError(f"{len(prompts)} prompts for a session of batch {B}")
        tmax, offsets = ragged_layout([p.numel() for p in prompts])
        if not (tmax + 1 <= self.total <= self.S):
            raise ValueError(f"the longest prompt ({tmax} tokens) and the new tokens must fit the cache without "
                             f"wrapping: need {tmax} + 1 <= total_len ({self.total}) <= max_seq_length ({self.S})")
        why = m.ragged_support()
        if why is not None:
            raise NotImplementedError(why)
        m.reset_cache()
        m.kv_caches = m._alloc_kv(B, self.S, self.dev)
        if m.rope_cache is None:
            m.rope_cache = m.build_rope_cache(prompts[0].to(self.dev))  # (the table lives where the idx does)
        self.packed_prefill = bool(packed) and m.packed_prefill_support(sum(p.numel() for p in prompts)) is None
        if self.packed_prefill:
            m._run_packed([p.to(self.dev) for p in prompts], self.S, m.kv_caches, self.logits)
        else:
            for b, p in enumerate(prompts):
                T = p.numel()
                pos = torch.arange(T, device=self.dev, dtype=torch.int32)
                row = [(kc[b:b + 1], vc[b:b + 1]) for kc, vc in m.kv_caches]  # contiguous views: a one-row cache
                m._run(p.reshape(1, -1).to(self.dev), pos, self.S, row, last_only_out=self.logits[b:b + 1])
        st = _hip.stream()
        self.tokens.zero_()
        left_padded(prompts, self.total, self.tokens)
        self.offsets = offsets
        self.off = torch.tensor(offsets, dtype=torch.int32, device=self.dev)
        self.pos.fill_(tmax - 1)
        self._choose(st)
        self.t_prompt = tmax
        self.steps_done = 1
        self._setup_work(ragged=True)

    def output_rows(self) -> list:
        """The rows of output() without the left padding of a ragged session: tokens[b, off[b] : t_prompt +
        steps_done] (prompt and new tokens of row b); off = 0 after prefill / prefill_shared."""
        off = self.offsets if self.offsets is not None else [0] * self.B
        return rows_of(self.tokens, off, self.t_prompt + self.steps_done)

    def _reset_handoff(self):
        """The LLM.int8 hand-off blocks (_Work.y_st / h_st) must be zero when a step starts; a
        completed step leaves them so, a step that raised part-way may not: zero them again."""
        w = self.work
        if w is not None and getattr(w, "y_st", None) is not None:
            w.y_st.zero_()
            w.h_st.zero_()

    def _step(self):
        try:
            self._step_launches()
        except BaseException:
            self._reset_handoff()
            raise

    def _step_launches(self):
        m, w, B = self.model, self.work, self.B
        cfg = m.config
        st = _hip.stream()
        if w.generic:
            _hip.call("llj_g_embedding", self.cur.data_ptr(), m.transformer.wte.weight.data_ptr(), w.x.data_ptr(), B,
                      cfg.n_embd, self.pos.data_ptr(), w.dt, st)
        else:
            _hip.call("llj_embedding", self.cur.data_ptr(), m.transformer.wte.weight.data_ptr(), w.x.data_ptr(), B,
                      cfg.n_embd, self.pos.data_ptr(), st)
        m._blocks(w, self.specs, m.kv_caches, self.pos, B, 1, self.S, st)
        m._head(w.x, B, self.specs, self.logits, st, w)
        self._choose(st)

    def capture(self):
        if self.graph is not None or not self.use_graph:
            return
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._step()
        self.graph = g

    @torch.no_grad()
    def decode(self, n: int) -> None:
        """Generate n more tokens per row (positions t_prompt + steps_done ...)."""
        assert self.t_prompt + self.steps_done + n <= self.total, "beyond the output buffer"
        assert self.t_prompt + self.steps_done + n - 1 <= self.model.config.block_size, "beyond block_size"
        if self.use_graph:
            self.capture()
            for _ in range(n):
                self.graph.replay()
        else:
            for _ in range(n):
                self._step()
        self.steps_done += n

    def output(self) -> torch.Tensor:
        return self.tokens[:, :self.t_prompt + self.steps_done]
