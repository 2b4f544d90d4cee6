"""Torch goldens of the dense W8A8 quantiser ops (`QUANT_DENSE_OPS`).

Importing this module registers the ``Torch<Op>`` classes as the ``torch`` backend of the API classes.

Semantics and rounding points restate `mojo_opset/core/operators/quantize.py:9-117`, `:250-354` and
`mojo_opset/core/operators/normalization.py:9-16`, `:136-305`, `:536-646`; `tests/golden/quant_dense.pt` pins every class bit for
bit (tests/make_quant_dense_golden.py records it from the reference).  Defined beyond the reference, as the hip backend defines
it: `TorchDequantSwiGLUQuant` does not raise when ``token_count`` sums to fewer rows than there are — negative counts read as
zero, and the rows at or past the sum come back as int8 zeros with scale 1.
"""
from typing import Optional

import torch
import torch.nn.functional as F

from mojo_opset_amd.core.operators import quantize as _q


def _smoothed(normed: torch.Tensor, smooth_scale: Optional[torch.Tensor]) -> torch.Tensor:
    if smooth_scale is None:
        return normed
    scale_fp = smooth_scale.float()
    while scale_fp.dim() < normed.dim():
        scale_fp = scale_fp.unsqueeze(0)
    return normed * scale_fp


def _quantise_rows(op, y: torch.Tensor):
    scale = y.abs().amax(dim=-1, keepdim=True).clamp(min=1e-12) / op.q_max
    q = torch.clamp(torch.round(y / scale), op.q_min, op.q_max)
    return q.to(op.quant_dtype), scale


class TorchRMSNormQuant(_q.MojoRMSNormQuant):
    supported_platforms_list = ["rocm", "cpu"]

    def forward(self, hidden_state, smooth_scale=None):
        normed = F.rms_norm(hidden_state.float(), [hidden_state.shape[-1]], weight=self.weight, eps=self.variance_epsilon)
        return _quantise_rows(self, _smoothed(normed, smooth_scale))


class TorchLayerNormQuant(_q.MojoLayerNormQuant):
    supported_platforms_list = ["rocm", "cpu"]

    def forward(self, hidden_state, smooth_scale=None):
        normed = F.layer_norm(hidden_state.float(), [hidden_state.shape[-1]], weight=self.weight, bias=self.bias,
                              eps=self.variance_epsilon)
        return _quantise_rows(self, _smoothed(normed, smooth_scale))


class TorchResidualAddLayerNormQuant(_q.MojoResidualAddLayerNormQuant):
    supported_platforms_list = ["rocm", "cpu"]

    def forward(self, hidden_state, residual, smooth_scale=None):
        summed = hidden_state + residual                      # one rounding to the input dtype; returned for both norm_pos
        normed = F.layer_norm(summed.float(), [summed.shape[-1]], weight=self.weight, bias=self.bias, eps=self.variance_epsilon)
        q, scale = _quantise_rows(self, _smoothed(normed, smooth_scale))
        return q, summed, scale


class TorchStaticQuant(_q.MojoStaticQuant):
    supported_platforms_list = ["rocm", "cpu"]

    def forward(self, input):
        self.check_call_contract(input)
        q = torch.clamp(torch.round(input.float() / self.scale.float()), self.q_min, self.q_max)
        return q.to(self.quant_dtype), self.scale


class TorchDequant(_q.MojoDequant):
    supported_platforms_list = ["rocm", "cpu"]

    def forward(self, input, scale):
        return (input.float() * scale.float()).to(self.output_dtype)


class TorchDequantSwiGLUQuant(_q.MojoDequantSwiGLUQuant):
    supported_platforms_list = ["rocm", "cpu"]

    def forward(self, x, activation_scale=None, bias=None, quant_offset=None, token_count=None):
        if x.dim() != 2:
            raise ValueError(f"x must be 2D with shape (tokens, 2H), but got {tuple(x.shape)}")
        if x.shape[-1] % 2 != 0:
            raise ValueError(f"x last dimension must be even for SwiGLU split, but got {x.shape[-1]}")
        if quant_offset is not None:
            raise NotImplementedError("quant_offset is not supported by the torch reference implementation.")
        tokens = x.shape[0]
        if token_count is None:
            if self.expert_num != 1:
                raise ValueError(f"token_count is required with expert_num={self.expert_num} (only a single expert can own every row).")
            live = tokens
            expert = torch.zeros(tokens, dtype=torch.long)
        else:
            counts = token_count.to(torch.long).clamp(min=0)
            ends = counts.cumsum(0).clamp(max=tokens)
            live = int(ends[-1])
            expert = torch.searchsorted(ends, torch.arange(tokens), right=True).clamp(max=self.expert_num - 1)
        y = x.float() * self.weight_scale.float()[expert]
        if activation_scale is not None:
            y = y * activation_scale.float().reshape(-1).unsqueeze(-1)
        if bias is not None:
            bias_fp = bias.float()
            y = y + (bias_fp[expert] if bias_fp.dim() == 2 else bias_fp)
        left, right = y.chunk(2, dim=-1)
        z = F.silu(left) * right if self.activate_left else F.silu(right) * left
        z = z * self.quant_scale.float()[expert]
        scale = z.abs().amax(dim=-1, keepdim=True).clamp(min=1e-12) / self.q_max
        q = torch.clamp(torch.round(z / scale), self.q_min, self.q_max).to(self.quant_dtype)
        if live < tokens:
            q[live:] = 0
            scale[live:] = 1.0
        return q, scale
