"""LoRA inference on the MI355X path: the names and state-dict contract of the reference's
lit_llama/lora.py (LoRALayer 58-87, MergedLinear 90-324, mark_only_lora_as_trainable 327-359,
lora_state_dict 362-393, LoRAConfig 396-400, CausalSelfAttention 403-444, lora 447-476).

LoRA gives c_attn two low-rank matrices over the enabled ones of its three output groups q, k, v
(enable_lora = [True, False, True] in the reference's attention; n_en = their count):
    lora_A (r * n_en, n_embd),  lora_B (3 * n_embd / 3 * n_en, r),  scaling = lora_alpha / r
and the Linear computes x . W^T + zero_pad((x . A^T) (*) B^T) * scaling, (*) being one product per
enabled group. Two forms run here:

  merged    eval() folds W += scaling * zero_pad(B . A) into the dense weight (llj_lora_merge, the
            reference's three rounding points) and train() takes it out again: the reference's only
            inference form. A merged model *is* the base model: it issues the base model's launches.
  unmerged  the low-rank term stays beside the weight: the down-projection t = x_n . A^T is one small
            dense Linear launch, the up-projection and the add ride in the epilogue of the kernel that
            produces c_attn's output, before RoPE and the KV write (the `*_lora` entry points of
            include/lit_llama_amd.h). A dense Linear runs it in train mode, as the reference does.

Inside quantization("gptq.int4" | "gptq.int8") c_attn is a ColBlockQuantizedLinear carrying lora_A /
lora_B and the attributes of LoRALayer / MergedLinear. A low-rank update cannot be folded into int4 or
int8 codes, so such a Linear never merges and always runs the unmerged form. This is this package's
extension: the reference's generate/lora.py refuses any --quantize (59-60).

Refused before any launch: LLM.int8 Linears (NotImplementedError), LoRA together with adapter v2
parameters on one Linear (TypeError), fan_in_fan_out (NotImplementedError), and a forward in train
mode with lora_dropout > 0 (NotImplementedError): nothing trains here, mark_only_lora_as_trainable
only sets requires_grad.
"""
from __future__ import annotations

import math
from contextlib import contextmanager
from dataclasses import dataclass
from typing import Dict, List

import torch
import torch.nn as nn

from . import _hip
from . import model as llama
from .quantization import ColBlockQuantizedLinear, Linear8bitLt


class LoRALayer:
    def __init__(self, r: int, lora_alpha: int, lora_dropout: float, merge_weights: bool):
        """The LoRA attributes of a layer (reference lora.py:58-87): rank, alpha, the dropout probability of
        the LoRA branch's input (kept as `lora_dropout_p`; `lora_dropout` is the reference's module or
        identity), and whether eval() merges the update into the weight."""
        self.r = r
        self.lora_alpha = lora_alpha
        self.lora_dropout_p = float(lora_dropout)
        self.lora_dropout = nn.Dropout(p=lora_dropout) if lora_dropout > 0.0 else (lambda x: x)
        self.merged = False
        self.merge_weights = merge_weights


def _enable_mask(enable_lora) -> int:
    return sum(1 << g for g, on in enumerate(enable_lora) if on)


def _init_lora(layer, in_features: int, out_features: int, r: int, enable_lora: List[bool], device, dtype) -> None:
    """lora_A / lora_B, scaling and lora_ind on `layer` (reference lora.py:148-189)."""
    if out_features % len(enable_lora):
        raise ValueError("The length of enable_lora must divide out_features")
    layer.enable_lora = list(enable_lora)
    if r > 0 and any(enable_lora):
        n_en = sum(enable_lora)
        layer.lora_A = nn.Parameter(torch.zeros((r * n_en, in_features), device=device, dtype=dtype))
        layer.lora_B = nn.Parameter(torch.zeros((out_features // len(enable_lora) * n_en, r), device=device,
                                                dtype=dtype))
        layer.scaling = layer.lora_alpha / layer.r
        ind = torch.zeros((len(enable_lora), out_features // len(enable_lora)), dtype=torch.bool)
        ind[torch.tensor(enable_lora, dtype=torch.bool), :] = True
        layer.lora_ind = ind.view(-1)  # which output features carry an update (lora.py:185-189)


def _zero_pad(layer, x: torch.Tensor) -> torch.Tensor:
    """The update of the enabled groups scattered to out_features, zeros elsewhere (lora.py:203-239)."""
    out_features = layer.lora_ind.numel()
    x = x.transpose(0, 1)
    result = x.new_zeros((*x.shape[:-1], out_features)).view(-1, out_features)
    result[:, layer.lora_ind.to(x.device)] = x.reshape(-1, int(layer.lora_ind.sum()))
    return result.view((*x.shape[:-1], out_features)).transpose(0, 1)


def has_lora(lin) -> bool:
    prm = lin.__dict__.get("_parameters") or {}
    return prm.get("lora_A") is not None and prm.get("lora_B") is not None


def lora_operands(lin, dtype):
    """The unmerged LoRA operands of a Linear for the `*_lora` entry points, checked before any launch:
    None for a Linear without LoRA, with rank 0, or merged (then the weight holds the update), else a
    dict(A, B, r, mask, scaling, cols) with A / B contiguous device tensors of the activation type."""
    if not has_lora(lin):
        return None
    if isinstance(lin, Linear8bitLt) or hasattr(lin, "SCB"):
        raise NotImplementedError("LoRA on an LLM.int8 Linear (Linear8bitLt) is not supported: use bf16 / fp32 weights "
                                  "(merged) or gptq.int4 / gptq.int8 (unmerged)")
    prm = lin._parameters
    if prm.get("adapter_scale") is not None or prm.get("adapter_bias") is not None:
        raise TypeError("LoRA and adapter v2 parameters on the same Linear are not supported")
    if getattr(lin, "fan_in_fan_out", False):
        raise NotImplementedError("LoRA with fan_in_fan_out=True is not supported")
    if getattr(lin, "merged", False) or lin.r <= 0 or not any(lin.enable_lora):
        return None
    if lin.training and lin.lora_dropout_p > 0.0:
        raise NotImplementedError("an unmerged LoRA forward in train mode with lora_dropout > 0: nothing trains on "
                                  "this path; call eval() or build the model with dropout 0")
    if len(lin.enable_lora) != 3:
        raise NotImplementedError("the LoRA kernels take c_attn's three groups (len(enable_lora) == 3)")
    A, B = prm["lora_A"], prm["lora_B"]
    n_en, r = sum(lin.enable_lora), lin.r
    N = lin.weight.shape[0] if isinstance(lin, nn.Linear) else lin.out_features
    K = lin.weight.shape[1] if isinstance(lin, nn.Linear) else lin.in_features
    if not 1 <= r <= 64:
        raise NotImplementedError(f"LoRA rank {r}: the kernels take 1..64")
    for t, what, shape in ((A, "lora_A", (r * n_en, K)), (B, "lora_B", (N // 3 * n_en, r))):
        _hip.require_device(t, what)
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise TypeError(f"{what} must be contiguous {shape}, got {tuple(t.shape)}")
        if t.dtype != dtype:
            raise TypeError(f"{what} is {t.dtype} on a model computing in {dtype}: cast the model as a whole")
    return dict(A=A, B=B, r=r, mask=_enable_mask(lin.enable_lora), scaling=float(lin.scaling), cols=r * n_en, lin=lin)


LORA_IMG_ROWS = 128  # rows of the zero-padded lora_A image: one prefill GEMM column tile


def lora_a_image(lin) -> torch.Tensor:
    """lora_A as the streaming kernels' dense bf16 Linear: zero-padded to 128 rows, so that decode (the
    first ceil(r * n_en / 16) * 16 rows, llj_norm_linear) and the prefill GEMM (all 128, llj_gemm_linear)
    read one image. Rebuilt when lora_A was written."""
    A = lin._parameters["lora_A"]
    key = (A.data_ptr(), A._version, A.device)
    img = lin.__dict__.get("_lora_img")
    if img is None or img[0] != key:
        rows = max(LORA_IMG_ROWS, (A.shape[0] + 127) // 128 * 128)
        t = torch.zeros((rows, A.shape[1]), dtype=torch.bfloat16, device=A.device)
        t[:A.shape[0]].copy_(A.detach())
        lin.__dict__["_lora_img"] = img = (key, t)
    return img[1]


def lora_linear_forward(lin, x: torch.Tensor) -> torch.Tensor:
    """The unmerged forward of one Linear for any M and any shape (reference lora.py:310-323):
    llj_g_linear for t = x . A^T, then llj_g_linear_lora for x . W^T with the low-rank term."""
    _hip.require_device(x, "input")
    if x.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"LoRA Linear computes in bfloat16 or float32, got {x.dtype}")
    op = lora_operands(lin, x.dtype)
    spec = llama._gspec(lin)
    N = lin.weight.shape[0] if isinstance(lin, nn.Linear) else lin.out_features
    K = x.shape[-1]
    x2 = x.reshape(-1, K).contiguous()
    M = x2.shape[0]
    out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    st = _hip.stream()
    if op is None:
        llama.LLaMA._glinear(spec, x2, M, K, N, out, None, st)
        return out.reshape(*x.shape[:-1], N)
    t = torch.empty((M, op["cols"]), dtype=x.dtype, device=x.device)
    llama.LLaMA._glinear((1, op["A"], None, None, 16, K), x2, M, K, op["cols"], t, None, st)
    llama.LLaMA._glinear(spec, x2, M, K, N, out, None, st, None, (t, op))
    return out.reshape(*x.shape[:-1], N)


class MergedLinear(nn.Linear, LoRALayer):
    """The reference's LoRA wrapper of the dense c_attn (lora.py:90-324): `weight` is the pretrained
    matrix, `lora_A` / `lora_B` the update of the enabled groups. eval() merges (llj_lora_merge), train()
    unmerges; an unmerged forward runs the kernels' LoRA form."""

    def __init__(self, in_features: int, out_features: int, r: int = 0, lora_alpha: int = 1,
                 lora_dropout: float = 0.0, enable_lora: List[bool] = [False], fan_in_fan_out: bool = False,
                 merge_weights: bool = True, **kwargs):
        if fan_in_fan_out:
            raise NotImplementedError("LoRA with fan_in_fan_out=True is not supported")
        nn.Linear.__init__(self, in_features, out_features, **kwargs)
        LoRALayer.__init__(self, r=r, lora_alpha=lora_alpha, lora_dropout=lora_dropout, merge_weights=merge_weights)
        self.fan_in_fan_out = fan_in_fan_out
        _init_lora(self, in_features, out_features, r, enable_lora, self.weight.device, self.weight.dtype)
        if has_lora(self):
            self.weight.requires_grad = False  # the pretrained matrix stays frozen (lora.py:172)
        self.reset_parameters()

    def reset_parameters(self):
        """reference lora.py:194-201: A as nn.Linear's default, B zero (so a fresh update is zero)."""
        nn.Linear.reset_parameters(self)
        if hasattr(self, "lora_A"):
            nn.init.kaiming_uniform_(self.lora_A, a=math.sqrt(5))
            nn.init.zeros_(self.lora_B)

    def zero_pad(self, x: torch.Tensor) -> torch.Tensor:
        return _zero_pad(self, x)

    def train(self, mode: bool = True):
        """reference lora.py:241-278: train(True) takes a merged update out of the weight, train(False)
        (eval) puts it in, with the reference's rounding points (llj_lora_merge)."""
        nn.Linear.train(self, mode)
        should = self.merged if mode else not self.merged
        if self.merge_weights and should:
            if self.r > 0 and any(self.enable_lora):
                self._merge(-1 if mode else 1)
            self.merged = not mode
        return self

    def _merge(self, sign: int) -> None:
        W, A, B = self.weight.data, self.lora_A.data, self.lora_B.data
        _hip.require_device(W, "MergedLinear.weight")
        if W.dtype not in (torch.bfloat16, torch.float32) or A.dtype != W.dtype or B.dtype != W.dtype:
            raise TypeError(f"LoRA merge: weight, lora_A and lora_B must share bfloat16 or float32, got {W.dtype}, "
                            f"{A.dtype}, {B.dtype}")
        if len(self.enable_lora) != 3 or not (W.is_contiguous() and A.is_contiguous() and B.is_contiguous()):
            raise NotImplementedError("LoRA merge: contiguous tensors and c_attn's three groups")
        N, K = W.shape
        _hip.call("llj_lora_merge", W.data_ptr(), A.data_ptr(), B.data_ptr(), N, K, self.r,
                  _enable_mask(self.enable_lora), float(self.scaling), sign, llama._dt_code(W.dtype), _hip.stream())

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.merged or lora_operands(self, x.dtype) is None:
            return nn.Linear.forward(self, x)
        return lora_linear_forward(self, x)


def _quantized_lora_linear(in_features: int, out_features: int, cfg: "LoRAConfig", enable_lora: List[bool]):
    """c_attn inside quantization(mode): the mode's Linear carrying lora_A / lora_B and MergedLinear's
    attributes. It never merges: `merged` stays False and every forward is the unmerged form."""
    layer = torch.nn.Linear(in_features, out_features, bias=False)
    if isinstance(layer, Linear8bitLt):
        raise NotImplementedError("LoRA on an LLM.int8 Linear (Linear8bitLt) is not supported: use bf16 / fp32 weights "
                                  "(merged) or gptq.int4 / gptq.int8 (unmerged)")
    if not isinstance(layer, ColBlockQuantizedLinear):
        raise TypeError(f"LoRA on {type(layer).__name__} is not supported")
    LoRALayer.__init__(layer, r=cfg.r, lora_alpha=cfg.alpha, lora_dropout=cfg.dropout, merge_weights=False)
    layer.fan_in_fan_out = False
    # (dtype None: the default dtype, or EmptyInitOnDevice's while the model is being built under it)
    _init_lora(layer, in_features, out_features, cfg.r, enable_lora, layer.quant_weight.device, None)
    if has_lora(layer):
        nn.init.kaiming_uniform_(layer.lora_A, a=math.sqrt(5))
    return layer


def mark_only_lora_as_trainable(model: nn.Module, bias: str = "none") -> None:
    """requires_grad on the LoRA matrices only, plus biases per `bias` (reference lora.py:327-359)."""
    for n, p in model.named_parameters():
        if "lora_" not in n:
            p.requires_grad = False
    if bias == "none":
        return
    if bias == "all":
        for n, p in model.named_parameters():
            if "bias" in n:
                p.requires_grad = True
    elif bias == "lora_only":
        for m in model.modules():
            if isinstance(m, LoRALayer) and getattr(m, "bias", None) is not None:
                m.bias.requires_grad = True
    else:
        raise NotImplementedError


def lora_state_dict(model: nn.Module, bias: str = "none") -> Dict[str, torch.Tensor]:
    """The LoRA matrices of a model's state dict, plus biases per `bias` (reference lora.py:362-393)."""
    sd = model.state_dict()
    if bias == "none":
        return {k: v for k, v in sd.items() if "lora_" in k}
    if bias == "all":
        return {k: v for k, v in sd.items() if "lora_" in k or "bias" in k}
    if bias == "lora_only":
        out = {}
        for k, v in sd.items():
            if "lora_" in k:
                out[k] = v
                bias_name = k.split("lora_")[0] + "bias"
                if bias_name in sd:
                    out[bias_name] = sd[bias_name]
        return out
    raise NotImplementedError


@dataclass
class LoRAConfig:
    r: float = 0.0
    alpha: float = 1.0
    dropout: float = 0.0


class CausalSelfAttention(llama.CausalSelfAttention):
    """reference lora.py:403-444: the attention's parameters with c_attn as a LoRA Linear on q and v."""
    lora_config = None

    def __init__(self, config: llama.LLaMAConfig) -> None:
        nn.Module.__init__(self)  # (the parent's Linears are not allocated first)
        assert config.n_embd % config.n_head == 0
        cfg, enable = self.lora_config, [True, False, True]
        if torch.nn.Linear is torch.nn.modules.linear.Linear:
            self.c_attn = MergedLinear(in_features=config.n_embd, out_features=3 * config.n_embd, r=cfg.r,
                                       lora_alpha=cfg.alpha, lora_dropout=cfg.dropout, enable_lora=enable,
                                       fan_in_fan_out=False, merge_weights=True, bias=False)
        else:  # inside quantization(mode): the mode's Linear class
            self.c_attn = _quantized_lora_linear(config.n_embd, 3 * config.n_embd, cfg, enable)
        self.c_proj = nn.Linear(config.n_embd, config.n_embd, bias=False)
        self.n_head = config.n_head
        self.n_embd = config.n_embd
        self.block_size = config.block_size
        self.rope_cache = None


@contextmanager
def lora(r, alpha, dropout, enabled: bool = True):
    """While active, lit_llama.model.CausalSelfAttention is the LoRA variant, so a model built inside
    carries LoRA on c_attn (reference lora.py:447-476). Unlike the reference, the original class is
    restored even if the body raises. enabled=False does nothing."""
    if not enabled:
        yield
        return
    CausalSelfAttention.lora_config = LoRAConfig(r=r, alpha=alpha, dropout=dropout)
    original = llama.CausalSelfAttention
    llama.CausalSelfAttention = CausalSelfAttention
    try:
        yield
    finally:
        llama.CausalSelfAttention = original
        CausalSelfAttention.lora_config = None
