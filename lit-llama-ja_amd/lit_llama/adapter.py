"""LLaMA-Adapter inference on the MI355X path: the module tree, state-dict contract and API of the
reference's lit_llama/adapter.py (LLaMAConfig 53-56, CausalSelfAttention 59-188, Block 191-217,
LLaMA 220-302, adapter_state_from_state_dict 311-313) over the kernels of lit_llama.model.

From `adapter_start_layer` upwards every attention layer owns a learned prefix (`adapter_wte`,
aT = adapter_prompt_length rows) and a per-head `gating_factor`; its output is
    y = softmax_causal(q . K^T / sqrt(hs)) . V + gating_factor[h] * softmax(q . AK^T / sqrt(hs)) . AV
with AK, AV = the K / V thirds of c_attn(adapter_wte.weight) (adapter.py:149-165; no RoPE, no
mask, the same for every batch row). They are computed once per reset_cache() through c_attn's
own forward (dense, ColBlockQuantizedLinear or Linear8bitLt alike) and kept per layer in
`adapter_kv_caches` as ((n_head, aT, hs) keys, values, fp32 gates).

One decode row block attends through llj_attention_adapter (the prefix term inside the decode
attention launch, ADAPTER_FUSED); prompts on the flash kernel, long caches on the split-K kernel and
the any-shape / fp32 models run their attention kernel followed by llj_adapter_prefix_add.
Fine-tuning (adapter.py:305-308, finetune/adapter.py) is not part of this package.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import torch
import torch.nn as nn

from . import model as llama
from .model import MLP, RMSNorm

# longest prefix the kernels take (csrc/attention.h kAdpMaxT: one LDS float per prefix key)
MAX_ADAPTER_PROMPT_LENGTH = 64

# decode attention of an adapted layer: 1 = llj_attention_adapter (one launch), 0 = llj_attention +
# llj_adapter_prefix_add (two; A/B: tools/adapter_decode_ab.py)
ADAPTER_FUSED = 1


@dataclass
class LLaMAConfig(llama.LLaMAConfig):
    adapter_prompt_length: int = 10
    adapter_start_layer: int = 2


class CausalSelfAttention(llama.CausalSelfAttention):
    """lit_llama.model.CausalSelfAttention plus, from adapter_start_layer on, the learned prefix
    embedding and the zero-initialised per-head gate (reference adapter.py:72-77)."""

    def __init__(self, config: LLaMAConfig, block_idx: int) -> None:
        super().__init__(config)
        if not 1 <= config.adapter_prompt_length <= MAX_ADAPTER_PROMPT_LENGTH:
            raise ValueError(f"adapter_prompt_length {config.adapter_prompt_length} is outside 1.."
                             f"{MAX_ADAPTER_PROMPT_LENGTH}, the prefix lengths the attention kernels take")
        if block_idx >= config.adapter_start_layer:
            self.adapter_wte = nn.Embedding(config.adapter_prompt_length, config.n_embd)
            self.gating_factor = nn.Parameter(torch.zeros(1, config.n_head, 1, 1))
        self.block_idx = block_idx
        self.adapter_prompt_length = config.adapter_prompt_length
        self.adapter_start_layer = config.adapter_start_layer

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        """Checkpoints from before the per-head gate hold one gating value for the whole layer
        (fewer than four dimensions): every head gets it (reference adapter.py:174-188)."""
        key = prefix + "gating_factor"
        g = state_dict.get(key)
        if g is not None:
            g = g._load_tensor() if hasattr(g, "_load_tensor") else g
            if g.dim() < 4:
                g = g.reshape(1, 1, 1, 1).expand(1, self.n_head, 1, 1).contiguous()
            state_dict[key] = g
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


class Block(nn.Module):
    """reference adapter.py:191-217 (module tree / parameter names); computed by LLaMA.forward."""

    def __init__(self, config: LLaMAConfig, block_idx: int) -> None:
        super().__init__()
        self.rms_1 = RMSNorm(config.n_embd)
        self.attn = CausalSelfAttention(config, block_idx)
        self.rms_2 = RMSNorm(config.n_embd)
        self.mlp = MLP(config)
        self.config = config

    def forward(self, *args, **kwargs):
        raise NotImplementedError("an adapter Block runs inside lit_llama.adapter.LLaMA.forward on this path")


class LLaMA(llama.LLaMA):
    """lit_llama.model.LLaMA whose blocks know their index (reference adapter.py:220-302)."""

    def __init__(self, config: LLaMAConfig) -> None:
        nn.Module.__init__(self)
        assert config.padded_vocab_size is not None
        self.config = config
        self.lm_head = nn.Linear(config.n_embd, config.padded_vocab_size, bias=False)
        self.transformer = nn.ModuleDict(
            dict(
                wte=nn.Embedding(config.padded_vocab_size, config.n_embd),
                h=nn.ModuleList(Block(config, i) for i in range(config.n_layer)),
                ln_f=RMSNorm(config.n_embd),
            )
        )
        self.rope_cache = None
        self.mask_cache = None
        self.kv_caches = []
        self.adapter_kv_caches: List[Optional[tuple]] = []

    @classmethod
    def from_name(cls, name: str):
        return cls(LLaMAConfig.from_name(name))

    def reset_cache(self) -> None:
        super().reset_cache()
        self.adapter_kv_caches.clear()

    # ------------------------------------------------------------------ hooks of lit_llama.model.LLaMA
    @torch.no_grad()
    def _build_adapter_kv(self) -> None:
        """adapter_kv_caches[i] = (ak, av, gate, aT) per adapted layer, None below the start layer
        (reference adapter.py:153-158 once per reset_cache(), for one batch row: the kernels
        share it between rows)."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the adapter prefix keys / values must exist before a decode step is captured: "
                               "run a forward (DecodeSession.prefill) first")
        cfg = self.config
        C, nh, aT = cfg.n_embd, cfg.n_head, cfg.adapter_prompt_length
        dt = self.act_dtype()
        out = []
        for i, blk in enumerate(self.transformer.h):
            if i < cfg.adapter_start_layer:
                out.append(None)
                continue
            attn = blk.attn
            llama._hip.require_device(attn.adapter_wte.weight, "adapter_wte")
            qkv = attn.c_attn(attn.adapter_wte.weight.detach().to(dt).reshape(aT, C))  # (aT, 3 C)
            ak = qkv[:, C:2 * C].reshape(aT, nh, C // nh).transpose(0, 1).contiguous()
            av = qkv[:, 2 * C:].reshape(aT, nh, C // nh).transpose(0, 1).contiguous()
            gate = attn.gating_factor.detach().reshape(nh).to(torch.float32).contiguous()  # bf16 -> fp32: exact
            out.append((ak, av, gate, aT))
        self.adapter_kv_caches = out

    def _adapter(self, i):
        if i < self.config.adapter_start_layer:
            return None
        if not self.adapter_kv_caches:
            self._build_adapter_kv()
        return self.adapter_kv_caches[i]

    def _adapter_fused(self) -> bool:
        return bool(ADAPTER_FUSED)

    def _enable_i8_handoff(self, w, specs) -> None:
        # llj_attention_i8 emits y's LLM.int8 statistics before a prefix term could be added: the
        # int8 c_proj takes its statistics from llj_i8_stats of the finished y instead
        w.i8s = False


def adapter_state_from_state_dict(state_dict: dict) -> dict:
    """The adapter's own tensors of a model state dict (what an adapter checkpoint holds)."""
    return {k: v for k, v in state_dict.items() if "adapter_wte" in k or "gating_factor" in k}
