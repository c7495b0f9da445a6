"""LLaMA-Adapter v2 inference on the MI355X path: the names and state-dict contract of the reference's
lit_llama/adapter_v2.py (get_adapter_substrings 9-13, mark_only_adapter_v2_as_trainable 16-19,
adapter_v2_state_from_state_dict 22-25, adapter_v2_new_forward 28-31,
adapter_v2_linear_with_bias_and_scale 34-39, add_adapter_v2_parameters_to_linear_layers 42-45) over
lit_llama.adapter.LLaMA.

v2 keeps the v1 prefix and gates and gives every Linear of the model, lm_head included, two learned
vectors of out_features, `adapter_bias` (zeros) and `adapter_scale` (ones); the Linear computes
    adapter_scale * (F.linear(x, W) + adapter_bias).
On this path the affine is an epilogue of the kernel that produces the Linear's output (the decode
GEMVs, the prefill GEMMs and the any-shape kernel: the `*_v2` entry points of include/lit_llama_amd.h),
applied before RoPE and the KV write, the residual add, silu * mul or the store -- no launch is added.
LLaMA.forward, MLP.forward and the Linears' own forwards pick the parameters up wherever they are
present; a model without them runs exactly the launches it ran before.

The parameters can be added to torch.nn.Linear and to ColBlockQuantizedLinear (gptq.int4 / gptq.int8;
inside quantization(mode) `torch.nn.Linear` is that class, as in the reference's generate/adapter_v2.py).
For quantized Linears the semantics are this package's extension, scale * (quantized_linear(x) + bias):
the reference's v2 forward calls F.linear on `self.weight` and does not run on them. LLM.int8 Linears
(Linear8bitLt) are not supported: the parameters can be added (the state-dict contract holds), the
first forward raises NotImplementedError before any launch.
Fine-tuning (finetune/adapter_v2.py) is not part of this package; mark_only_adapter_v2_as_trainable
only sets requires_grad.
"""
from __future__ import annotations

import types

import torch
from torch import Tensor

from . import _hip
from . import model as llama
from .adapter import LLaMA
from .quantization import ColBlockQuantizedLinear, Linear8bitLt, _linear_rows


ADAPTER_V2_SUBSTRINGS = (
    "adapter_wte", "gating_factor",   # the v1 prefix embedding and its gates
    "adapter_scale", "adapter_bias",  # v2: the per-Linear vectors
    "rms_1", "rms_2", "ln_f",         # v2: the RMSNorm scales belong to the adapter checkpoint
)


def get_adapter_substrings():
    """Name fragments of the tensors an adapter v2 checkpoint holds (reference adapter_v2.py:9-13)."""
    return list(ADAPTER_V2_SUBSTRINGS)


def _is_adapter_v2_name(name: str) -> bool:
    return any(part in name for part in ADAPTER_V2_SUBSTRINGS)


def mark_only_adapter_v2_as_trainable(model: LLaMA) -> None:
    """requires_grad on exactly the adapter v2 parameters (reference adapter_v2.py:16-19). Nothing here
    trains: the flag is set for code that inspects it."""
    for name, prm in model.named_parameters():
        prm.requires_grad_(_is_adapter_v2_name(name))


def adapter_v2_state_from_state_dict(state_dict: dict) -> dict:
    """The entries of a model state dict that make up an adapter v2 checkpoint (reference adapter_v2.py:22-25)."""
    return {k: v for k, v in state_dict.items() if _is_adapter_v2_name(k)}


def adapter_v2_new_forward(self, input: Tensor) -> Tensor:
    """adapter_scale * (F.linear(input, weight, bias) + adapter_bias) of a dense Linear in one launch:
    llj_linear_v2 for bf16 rows on the streaming tiling (the Linear's own bias, if any, is added in
    fp32 before the Linear's output is rounded), llj_g_linear_v2 for fp32 or any other shape, where a
    biased Linear is refused."""
    _hip.require_device(input, "input")
    if input.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"adapter v2 Linear computes in bfloat16 or float32, got {input.dtype}")
    af = llama._affine(self, input.dtype)
    W = self.weight
    N, K = W.shape
    x2 = input.reshape(-1, K).contiguous()
    out = torch.empty((x2.shape[0], N), dtype=input.dtype, device=input.device)
    if input.dtype == torch.bfloat16 and K % 128 == 0 and N % 16 == 0:
        _hip.require_device(W, "Linear.weight")
        if W.dtype != torch.bfloat16 or not W.is_contiguous():
            raise TypeError("dense Linear weights must be contiguous bfloat16 on the GPU")
        bias = None if self.bias is None else self.bias.detach().to(torch.bfloat16).contiguous()
        _linear_rows(1, x2, W, None, bias, out, N, K, af)
    else:  # (_gspec raises NotImplementedError for a biased Linear)
        llama.LLaMA._glinear(llama._gspec(self), x2, x2.shape[0], K, N, out, None, _hip.stream(), af)
    return out.reshape(*input.shape[:-1], N)


def adapter_v2_linear_with_bias_and_scale(layer):
    """adapter_bias (zeros) and adapter_scale (ones) of out_features on `layer`'s device (reference
    adapter_v2.py:34-39). A dense Linear then computes through adapter_v2_new_forward; the quantized
    classes' own forwards take the parameters up."""
    quantized = isinstance(layer, (ColBlockQuantizedLinear, Linear8bitLt))
    if quantized:
        n, ref, dtype = layer.out_features, (layer.quant_weight if hasattr(layer, "quant_weight") else layer.weight), None
    else:
        n, ref, dtype = layer.weight.shape[0], layer.weight, layer.weight.dtype
    # (dtype None: the default dtype, or EmptyInitOnDevice's while the model is being built under it)
    layer.adapter_bias = torch.nn.Parameter(torch.zeros(n, device=ref.device, dtype=dtype))
    layer.adapter_scale = torch.nn.Parameter(torch.ones(n, device=ref.device, dtype=dtype))
    if not quantized:  # this instance only: other Linears of the class keep their forward
        layer.forward = types.MethodType(adapter_v2_new_forward, layer)
    return layer


def add_adapter_v2_parameters_to_linear_layers(model):
    """Every Linear of `model`: the dense class and this package's quantized Linear classes -- named
    directly, since inside quantization(mode) `torch.nn.Linear` is a constructor of the quantized class
    (a functools.partial for the GPTQ modes), not a type."""
    for module in model.modules():
        if isinstance(module, (torch.nn.modules.linear.Linear, ColBlockQuantizedLinear, Linear8bitLt)):
            adapter_v2_linear_with_bias_and_scale(module)
