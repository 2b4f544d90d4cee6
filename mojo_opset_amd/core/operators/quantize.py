"""API classes of the activation quantisers that feed `MojoQuantGemm`.

Follows `mojo_opset/core/operators/quantize.py:120-172` (`MojoDynamicQuant`), `:178-247` (`MojoMoEDynamicQuant`) and
`mojo_opset/core/operators/normalization.py:434-533` (`MojoResidualAddRMSNormQuant`).

The dense W8A8 set (`QUANT_DENSE_OPS`, core/operators/__init__.py) follows `quantize.py:9-117` (`MojoStaticQuant`, `MojoDequant`),
`:250-354` (`MojoDequantSwiGLUQuant`) and `normalization.py:136-305`, `:536-646` (`MojoRMSNormQuant`, `MojoLayerNormQuant`,
`MojoResidualAddLayerNormQuant`): constructor signatures, parameter names and shapes, constructor-time errors and `extra_repr`
are the reference's, so a `state_dict` moves between the two.
"""
from typing import Optional

import torch

from ..operator import MojoOperator


class MojoDynamicQuant(MojoOperator):
    """forward(input [*, K]) -> (int8 [*, K], fp32 scale [*, 1]): per-token symmetric quantisation,
    ``scale = max(amax|x * inv_smooth_scale|, 1e-12) / 127`` (``1.0`` where that is below 1e-6),
    ``q = clamp(round_half_even(x / scale), -128, 127)``.  ``inv_smooth_scale [K]`` fp32 is optional (``input_size=None``)."""

    def __init__(self, input_size: Optional[int] = None, quant_dtype: torch.dtype = torch.int8, **kwargs):
        super().__init__(**kwargs)
        self.input_size = input_size
        if input_size is None:
            self.register_parameter("inv_smooth_scale", None)
        else:
            self.inv_smooth_scale = torch.nn.Parameter(torch.empty(input_size, **self.tensor_factory_kwargs))
            setattr(self.inv_smooth_scale, "force_dtype", torch.float32)
        self.quant_dtype = quant_dtype
        if quant_dtype != torch.int8:
            raise NotImplementedError(f"Unsupported quant_dtype: {quant_dtype}, expected torch.int8.")
        self.q_max = 127
        self.q_min = -128

    def extra_repr(self) -> str:
        return f"input_size={self.input_size}, quant_dtype={self.quant_dtype}"


class MojoMoEDynamicQuant(MojoOperator):
    """forward(input [*, K], token_count int32 | int64 [E]) -> (int8 like input, fp32 scale input.shape[:-1] + (1,)):
    `MojoDynamicQuant`'s arithmetic with the smooth scale of the row's expert.  The rows arrive sorted by expert,
    ``token_count[e]`` of them for expert ``e``; ``inv_smooth_scale [expert_num, input_size]`` is fp32 (``force_dtype``)."""

    def __init__(self, expert_num: int, input_size: int, quant_dtype: torch.dtype = torch.int8, **kwargs):
        super().__init__(**kwargs)
        self.expert_num = expert_num
        self.input_size = input_size
        self.inv_smooth_scale = torch.nn.Parameter(torch.empty((expert_num, input_size), **self.tensor_factory_kwargs))
        setattr(self.inv_smooth_scale, "force_dtype", torch.float32)
        self.quant_dtype = quant_dtype
        if quant_dtype != torch.int8:
            raise NotImplementedError(f"Unsupported quant_dtype: {quant_dtype}, expected torch.int8.")
        self.q_max = 127
        self.q_min = -128

    def check_call_contract(self, input, token_count):
        """The reference's shape and dtype checks (:223-228); what needs the VALUES of ``token_count`` is the backend's call."""
        if input.dim() < 2:
            raise ValueError(f"input must have at least 2 dimensions for MoE dynamic quant, got {input.dim()}.")
        if token_count.dim() != 1:
            raise ValueError(f"token_count must be 1D, got shape {tuple(token_count.shape)}.")
        if token_count.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"token_count must be int32 or int64, got {token_count.dtype}.")

    def extra_repr(self) -> str:
        return f"expert_num={self.expert_num}, input_size={self.input_size}, quant_dtype={self.quant_dtype}"


class MojoResidualAddRMSNormQuant(MojoOperator):
    """forward(hidden_state, residual, smooth_scale=None) -> (quant_output, residual_out, scale [*, 1]).

    ``pre``: ``residual_out = hidden + residual`` (input dtype); ``post``: ``residual_out`` is the fp32 normed tensor.
    ``normed = rms_norm(sum.float(), weight, eps)`` stays fp32; ``scale = max(amax|normed * smooth|, 1e-12) / q_max``;
    ``q = clamp(round_half_even(normed / scale), q_min, q_max)`` cast to int8 or float8_e4m3fn.
    """

    def __init__(self, norm_size: int, eps: float = 1e-5, norm_pos: str = "pre", quant_dtype: torch.dtype = torch.int8,
                 symmetric: bool = True, **kwargs):
        super().__init__(**kwargs)
        if norm_pos not in ("pre", "post"):
            raise ValueError("norm_pos should be 'pre' or 'post'")
        self.norm_size = norm_size
        self.variance_epsilon = float(eps)
        self.norm_pos = norm_pos
        self.weight = torch.nn.Parameter(torch.empty(norm_size, **self.tensor_factory_kwargs))
        self.quant_dtype = quant_dtype
        self.symmetric = symmetric
        if quant_dtype == torch.int8:
            self.q_max = 127
            self.q_min = -128 if symmetric else 0
        elif quant_dtype == torch.float8_e4m3fn:
            self.q_max = torch.finfo(torch.float8_e4m3fn).max
            self.q_min = -torch.finfo(torch.float8_e4m3fn).max
        else:
            raise NotImplementedError(
                f"Unsupported quant_dtype: {quant_dtype}, "
                f"expected torch.int8 or torch.float8_e4m3fn"
            )

    def extra_repr(self) -> str:
        return (
            f"norm_size={self.norm_size}, variance_epsilon={self.variance_epsilon}, "
            f"norm_pos={self.norm_pos!r}, quant_dtype={self.quant_dtype}, "
            f"symmetric={self.symmetric}"
        )


def _quant_range(quant_dtype: torch.dtype, symmetric: bool = True):
    """(q_max, q_min) of the norm+quant family; raises the reference's NotImplementedError for another dtype."""
    if quant_dtype == torch.int8:
        return 127, (-128 if symmetric else 0)
    if quant_dtype == torch.float8_e4m3fn:
        return torch.finfo(torch.float8_e4m3fn).max, -torch.finfo(torch.float8_e4m3fn).max
    raise NotImplementedError(
        f"Unsupported quant_dtype: {quant_dtype}, "
        f"expected torch.int8 or torch.float8_e4m3fn"
    )


class MojoRMSNormQuant(MojoOperator):
    """forward(hidden_state [*, D], smooth_scale=None) -> (quant_output, scale [*, 1]).

    ``normed = rms_norm(hidden_state.float(), weight, eps)`` stays fp32, ``* smooth_scale`` when given;
    ``scale = max(amax|normed|, 1e-12) / q_max``; ``q = clamp(round_half_even(normed / scale), q_min, q_max)`` cast to int8 (``q_min``
    -128, or 0 with ``symmetric=False``) or float8_e4m3fn."""

    def __init__(self, norm_size: int, eps: float = 1e-5, quant_dtype: torch.dtype = torch.int8, symmetric: bool = True, **kwargs):
        super().__init__(**kwargs)
        self.norm_size = norm_size
        self.variance_epsilon = eps
        self.weight = torch.nn.Parameter(torch.empty(norm_size, **self.tensor_factory_kwargs))
        self.quant_dtype = quant_dtype
        self.symmetric = symmetric
        self.q_max, self.q_min = _quant_range(quant_dtype, symmetric)

    def extra_repr(self) -> str:
        return (
            f"norm_size={self.norm_size}, variance_epsilon={self.variance_epsilon}, "
            f"quant_dtype={self.quant_dtype}, symmetric={self.symmetric}"
        )


class MojoLayerNormQuant(MojoOperator):
    """forward(hidden_state [*, D], smooth_scale=None) -> (quant_output, scale [*, 1]): `MojoRMSNormQuant` with
    ``layer_norm(hidden_state.float(), weight, bias, eps)`` (mean and biased variance over the row, fp32); ``weight`` and ``bias``
    are both parameters or, with ``elementwise_affine=False``, both ``None``."""

    def __init__(self, norm_size: int, eps: float = 1e-5, elementwise_affine: bool = True, quant_dtype: torch.dtype = torch.int8,
                 symmetric: bool = True, **kwargs):
        super().__init__(**kwargs)
        self.norm_size = norm_size
        self.variance_epsilon = eps
        self.elementwise_affine = elementwise_affine
        self.quant_dtype = quant_dtype
        self.symmetric = symmetric
        if elementwise_affine:
            self.weight = torch.nn.Parameter(torch.empty(norm_size, **self.tensor_factory_kwargs))
            self.bias = torch.nn.Parameter(torch.empty(norm_size, **self.tensor_factory_kwargs))
        else:
            self.weight = None
            self.bias = None
        self.q_max, self.q_min = _quant_range(quant_dtype, symmetric)

    def extra_repr(self) -> str:
        return (
            f"norm_size={self.norm_size}, variance_epsilon={self.variance_epsilon}, "
            f"elementwise_affine={self.elementwise_affine}, "
            f"quant_dtype={self.quant_dtype}, symmetric={self.symmetric}"
        )


class MojoResidualAddLayerNormQuant(MojoOperator):
    """forward(hidden_state, residual, smooth_scale=None) -> (quant_output, residual_out, scale [*, 1]).

    ``residual_out = hidden_state + residual`` in the input dtype for BOTH ``norm_pos`` (unlike `MojoResidualAddRMSNormQuant`,
    whose ``post`` returns the fp32 normed tensor); the quantised tensor is `MojoLayerNormQuant` of that sum."""

    def __init__(self, norm_size: int, eps: float = 1e-5, elementwise_affine: bool = True, norm_pos: str = "pre",
                 quant_dtype: torch.dtype = torch.int8, symmetric: bool = True, **kwargs):
        super().__init__(**kwargs)
        if norm_pos not in ("pre", "post"):
            raise ValueError("norm_pos should be 'pre' or 'post'")
        self.norm_size = norm_size
        self.variance_epsilon = float(eps)
        self.norm_pos = norm_pos
        self.elementwise_affine = elementwise_affine
        self.quant_dtype = quant_dtype
        self.symmetric = symmetric
        if elementwise_affine:
            self.weight = torch.nn.Parameter(torch.empty(norm_size, **self.tensor_factory_kwargs))
            self.bias = torch.nn.Parameter(torch.empty(norm_size, **self.tensor_factory_kwargs))
        else:
            self.weight = None
            self.bias = None
        self.q_max, self.q_min = _quant_range(quant_dtype, symmetric)

    def extra_repr(self) -> str:
        return (
            f"norm_size={self.norm_size}, variance_epsilon={self.variance_epsilon}, "
            f"elementwise_affine={self.elementwise_affine}, norm_pos={self.norm_pos!r}, "
            f"quant_dtype={self.quant_dtype}, symmetric={self.symmetric}"
        )


class MojoStaticQuant(MojoOperator):
    """forward(input [..., *input_size]) -> (quantised like input, self.scale):
    ``clamp(round_half_even(input.float() / scale.float()), q_min, q_max)`` cast to int8 or float8_e4m3fn.  ``scale`` has shape
    ``input_size`` (an int or a tuple), which must equal the trailing dimensions of the input."""

    def __init__(self, input_size, quant_dtype: torch.dtype = torch.int8, **kwargs):
        super().__init__(**kwargs)
        if isinstance(input_size, int):
            self.input_size = (input_size,)
        else:
            self.input_size = tuple(input_size)
        self.scale = torch.nn.Parameter(torch.empty(self.input_size, **self.tensor_factory_kwargs))
        self.quant_dtype = quant_dtype
        if quant_dtype == torch.int8:
            self.q_max = 127
            self.q_min = -128
        elif quant_dtype == torch.float8_e4m3fn:
            self.q_max = torch.finfo(torch.float8_e4m3fn).max
            self.q_min = -torch.finfo(torch.float8_e4m3fn).max
        else:
            raise NotImplementedError(
                f"Unsupported quant_dtype: {quant_dtype}, expected torch.int8 or torch.float8_e4m3fn"
            )

    def check_call_contract(self, input):
        """The reference's two shape checks (quantize.py:59-68)."""
        if input.dim() < len(self.input_size):
            raise ValueError(
                f"input must have at least {len(self.input_size)} dims for scale shape "
                f"{self.input_size}, got {tuple(input.shape)}."
            )
        if tuple(input.shape[-len(self.input_size):]) != self.input_size:
            raise ValueError(
                f"input trailing dims {tuple(input.shape[-len(self.input_size):])} must "
                f"match scale shape {self.input_size}."
            )

    def extra_repr(self) -> str:
        return f"input_size={self.input_size}, quant_dtype={self.quant_dtype}, q_max={self.q_max}, q_min={self.q_min}"


class MojoDequant(MojoOperator):
    """forward(input int8 | float8_e4m3fn, scale) -> ``(input.float() * scale.float())`` rounded once to ``output_dtype`` (fp16,
    bf16 or fp32).  ``scale`` broadcasts against the input."""

    def __init__(self, output_dtype: torch.dtype = torch.bfloat16, **kwargs):
        super().__init__(**kwargs)
        if output_dtype not in (torch.float16, torch.bfloat16, torch.float32):
            raise NotImplementedError(
                f"Unsupported output_dtype: {output_dtype}, expected torch.float16, torch.bfloat16, or torch.float32."
            )
        self.output_dtype = output_dtype

    def extra_repr(self) -> str:
        # (the reference's also prints `self.input_size`, a field its constructor never sets: it raises)
        return f"output_dtype={self.output_dtype}"


class MojoDequantSwiGLUQuant(MojoOperator):
    """forward(x [T, 2H], activation_scale=None, bias=None, quant_offset=None, token_count=None) -> (int8 [T, H], fp32 scale [T, 1]):
    the stage between fc1 and fc2 of a W8A8 MLP.  ``y = x.float() * weight_scale[e]``, ``* activation_scale[t]``, ``+ bias``
    (``[2H]`` or ``[E, 2H]``); ``z = silu(right) * left`` of the two halves (``activate_left``: ``silu(left) * right``),
    ``* quant_scale[e]``; ``scale = max(amax|z|, 1e-12) / 127``; ``q = clamp(round_half_even(z / scale), -128, 127)``.  ``e`` is the
    row's expert: the rows arrive sorted by expert, ``token_count[e]`` of them for expert ``e``."""

    def __init__(self, expert_num: int, hidden_size: int, quant_dtype: torch.dtype = torch.int8, activate_left: bool = False,
                 quant_mode: int = 1, **kwargs):
        super().__init__(**kwargs)
        self.expert_num = expert_num
        self.hidden_size = hidden_size
        self.weight_scale = torch.nn.Parameter(torch.empty((expert_num, hidden_size * 2), **self.tensor_factory_kwargs))
        self.quant_scale = torch.nn.Parameter(torch.empty((expert_num, hidden_size), **self.tensor_factory_kwargs))
        self.quant_dtype = quant_dtype
        self.activate_left = activate_left
        self.quant_mode = quant_mode
        if quant_dtype != torch.int8:
            raise NotImplementedError(f"Unsupported quant_dtype: {quant_dtype}, expected torch.int8.")
        if quant_mode != 1:
            raise NotImplementedError("Only dynamic quant_mode=1 is currently supported.")
        self.q_max = 127
        self.q_min = -128

    def extra_repr(self) -> str:
        return (
            f"expert_num={self.expert_num}, hidden_size={self.hidden_size}, quant_dtype={self.quant_dtype}, "
            f"activate_left={self.activate_left}, quant_mode={self.quant_mode}"
        )


__all__ = ["MojoDynamicQuant", "MojoResidualAddRMSNormQuant"]      # (MojoMoEDynamicQuant: QUANT_MOE_OPS; the dense set: QUANT_DENSE_OPS, core/operators/__init__.py)
