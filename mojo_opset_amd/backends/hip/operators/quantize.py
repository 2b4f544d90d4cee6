"""HIP<Op> classes of the per-token activation quantisers."""
from typing import Optional

import torch

from ....core.operators.quantize import (MojoDequant, MojoDequantSwiGLUQuant, MojoDynamicQuant, MojoLayerNormQuant,
                                         MojoMoEDynamicQuant, MojoResidualAddLayerNormQuant, MojoResidualAddRMSNormQuant,
                                         MojoRMSNormQuant, MojoStaticQuant)
from .. import lib as L

_ROCM = ["rocm"]


def _dense(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous() else t.contiguous()


def _fp32_vector(t: Optional[torch.Tensor], dim: int, what: str):
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise NotImplementedError(f"hip quantiser: {what} must be float32 (the reference pins it with force_dtype), got {t.dtype}")
    t = _dense(t.detach()).reshape(-1)
    if t.numel() != dim:
        raise ValueError(f"{what} has {t.numel()} elements, the last input dimension is {dim}")
    return t


class HIPDynamicQuant(MojoDynamicQuant):
    supported_platforms_list = _ROCM

    def forward(self, input: torch.Tensor):
        if input.dim() < 1:
            raise ValueError("input must have at least one dimension.")
        L.require_cuda(input, self.inv_smooth_scale)
        x = _dense(input)
        dim = x.shape[-1]
        rows = x.numel() // dim if dim else 0
        inv = _fp32_vector(self.inv_smooth_scale, dim, "inv_smooth_scale")
        out = torch.empty(x.shape, dtype=torch.int8, device=x.device)
        scale = torch.empty(*x.shape[:-1], 1, dtype=torch.float32, device=x.device)
        L.check(L.load().mojo_hip_dynamic_quant(L.ptr(x), L.ptr(inv), L.ptr(out), L.ptr(scale), rows, dim,
                                                L.dtype_code(x.dtype), L.stream_of(x)), "HIPDynamicQuant")
        return out, scale


def moe_dynamic_quant(x: torch.Tensor, inv_smooth: torch.Tensor, counts: torch.Tensor, dim: int, glu: bool, what: str):
    """One launch of ``mojo_hip_moe_dynamic_quant`` on a dense ``x [rows, dim]`` (``glu``: ``[rows, 2 * dim]`` = [gate | up]):
    returns ``(int8 [rows, dim], fp32 scale [rows, 1])``."""
    if inv_smooth.dtype != torch.float32:
        raise NotImplementedError(f"{what}: inv_smooth_scale must be float32 (the reference pins it with force_dtype), got {inv_smooth.dtype}")
    if inv_smooth.dim() != 2 or inv_smooth.shape[1] != dim or inv_smooth.shape[0] != counts.numel():
        raise ValueError(f"{what}: inv_smooth_scale {tuple(inv_smooth.shape)} does not match {counts.numel()} experts x {dim}")
    rows = x.shape[0]
    out = torch.empty(rows, dim, dtype=torch.int8, device=x.device)
    scale = torch.empty(rows, 1, dtype=torch.float32, device=x.device)
    L.check(L.load().mojo_hip_moe_dynamic_quant(L.ptr(x), L.ptr(inv_smooth), L.ptr(counts), 1 if counts.dtype == torch.int64 else 0,
                                                L.ptr(out), L.ptr(scale), rows, dim, counts.numel(), 1 if glu else 0,
                                                L.dtype_code(x.dtype), L.stream_of(x)), what)
    return out, scale


class HIPMoEDynamicQuant(MojoMoEDynamicQuant):
    """The expert of a row is found on the device from ``token_count``; nothing synchronises with the host.  The reference
    validates ``token_count`` on the host (non-negative, summing to the row count); this class does NOT: negative counts
    read as zero, and rows at or past ``sum(token_count)`` come back as int8 zeros with scale 1."""

    supported_platforms_list = _ROCM

    def forward(self, input: torch.Tensor, token_count: torch.Tensor):
        # (the reference's own shape / dtype checks, spelled out so the body also binds to the reference's class)
        if input.dim() < 2:
            raise ValueError(f"input must have at least 2 dimensions for MoE dynamic quant, got {input.dim()}.")
        if token_count.dim() != 1:
            raise ValueError(f"token_count must be 1D, got shape {tuple(token_count.shape)}.")
        if token_count.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"token_count must be int32 or int64, got {token_count.dtype}.")
        if input.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise NotImplementedError(f"HIPMoEDynamicQuant: input dtype {input.dtype}")
        inv = self.inv_smooth_scale.detach()
        L.require_cuda(input, inv)
        x = _dense(input)
        dim = x.shape[-1]
        counts = _dense(token_count.to(x.device, non_blocking=True))
        out, scale = moe_dynamic_quant(x.reshape(-1, dim), _dense(inv), counts, dim, False, "HIPMoEDynamicQuant")
        return out.reshape(x.shape), scale.reshape(*x.shape[:-1], 1)


class HIPResidualAddRMSNormQuant(MojoResidualAddRMSNormQuant):
    supported_platforms_list = _ROCM

    def forward(self, hidden_state: torch.Tensor, residual: torch.Tensor, smooth_scale: Optional[torch.Tensor] = None):
        L.require_cuda(hidden_state, residual, smooth_scale, self.weight)
        if residual.shape != hidden_state.shape or residual.dtype != hidden_state.dtype:
            raise NotImplementedError("HIPResidualAddRMSNormQuant: hidden_state and residual must share shape and dtype")
        h, r = _dense(hidden_state), _dense(residual)
        dim = h.shape[-1]
        rows = h.numel() // dim if dim else 0
        weight = _fp32_vector(self.weight, dim, "weight")
        smooth = _fp32_vector(smooth_scale, dim, "smooth_scale")
        dev = h.device
        out = torch.empty(h.shape, dtype=self.quant_dtype, device=dev)
        scale = torch.empty(*h.shape[:-1], 1, dtype=torch.float32, device=dev)
        pre = self.norm_pos == "pre"
        summed = torch.empty_like(h) if pre else None
        normed = None if pre else torch.empty(h.shape, dtype=torch.float32, device=dev)
        L.check(L.load().mojo_hip_residual_add_rmsnorm_quant(
            L.ptr(h), L.ptr(r), L.ptr(weight), L.ptr(smooth), L.ptr(out), L.ptr(summed), L.ptr(normed), L.ptr(scale), rows, dim,
            L.dtype_code(h.dtype), L.dtype_code(self.quant_dtype), float(self.q_min), float(self.variance_epsilon),
            L.stream_of(h)), "HIPResidualAddRMSNormQuant")
        return out, (summed if pre else normed), scale


# ---- the dense W8A8 set (QUANT_DENSE_OPS) ----------------------------------------------------------------------------------
def _as_fp32(t: Optional[torch.Tensor]):
    """``t.float()`` as a dense tensor (exact for every dtype the parameters come in); fp32 passes straight through."""
    if t is None:
        return None
    t = t.detach()
    return _dense(t if t.dtype == torch.float32 else t.float())


def _norm_quant_buffers(op, x: torch.Tensor):
    out = torch.empty(x.shape, dtype=op.quant_dtype, device=x.device)
    scale = torch.empty(*x.shape[:-1], 1, dtype=torch.float32, device=x.device)
    return out, scale


def _check_float_input(x: torch.Tensor, what: str):
    if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise NotImplementedError(f"{what}: input dtype {x.dtype} (float32, float16 or bfloat16)")
    if x.dim() < 1:
        raise ValueError(f"{what}: input must have at least one dimension.")


class HIPRMSNormQuant(MojoRMSNormQuant):
    """`HIPResidualAddRMSNormQuant`'s kernel with no residual and no sum output (launch tags ``rmsnorm_quant:...``)."""

    supported_platforms_list = _ROCM

    def forward(self, hidden_state: torch.Tensor, smooth_scale: Optional[torch.Tensor] = None):
        _check_float_input(hidden_state, "HIPRMSNormQuant")
        L.require_cuda(hidden_state, smooth_scale, self.weight)
        x = _dense(hidden_state)
        dim = x.shape[-1]
        rows = x.numel() // dim if dim else 0
        weight = _fp32_vector(self.weight, dim, "weight")
        smooth = _fp32_vector(_as_fp32(smooth_scale), dim, "smooth_scale")
        out, scale = _norm_quant_buffers(self, x)
        L.check(L.load().mojo_hip_rmsnorm_quant(
            L.ptr(x), L.ptr(weight), L.ptr(smooth), L.ptr(out), L.ptr(scale), rows, dim, L.dtype_code(x.dtype),
            L.dtype_code(self.quant_dtype), float(self.q_min), float(self.variance_epsilon), L.stream_of(x)), "HIPRMSNormQuant")
        return out, scale


def _layernorm_quant(op, hidden: torch.Tensor, residual: Optional[torch.Tensor], smooth_scale, what: str):
    """One launch of ``mojo_hip_layernorm_quant``: ``(q, hidden + residual or None, scale)``."""
    _check_float_input(hidden, what)
    if (op.weight is None) != (op.bias is None):
        raise ValueError(f"{what}: weight and bias come together (elementwise_affine) or not at all")
    if residual is not None and (residual.shape != hidden.shape or residual.dtype != hidden.dtype):
        raise NotImplementedError(f"{what}: hidden_state and residual must share shape and dtype")
    L.require_cuda(hidden, residual, smooth_scale, op.weight, op.bias)
    h = _dense(hidden)
    r = None if residual is None else _dense(residual)
    dim = h.shape[-1]
    rows = h.numel() // dim if dim else 0
    weight = _fp32_vector(op.weight, dim, "weight")
    bias = _fp32_vector(op.bias, dim, "bias")
    smooth = _fp32_vector(_as_fp32(smooth_scale), dim, "smooth_scale")
    out, scale = _norm_quant_buffers(op, h)
    summed = None if r is None else torch.empty_like(h)
    L.check(L.load().mojo_hip_layernorm_quant(
        L.ptr(h), L.ptr(r), L.ptr(weight), L.ptr(bias), L.ptr(smooth), L.ptr(out), L.ptr(summed), L.ptr(scale), rows, dim,
        L.dtype_code(h.dtype), L.dtype_code(op.quant_dtype), float(op.q_min), float(op.variance_epsilon), L.stream_of(h)), what)
    return out, summed, scale


class HIPLayerNormQuant(MojoLayerNormQuant):
    supported_platforms_list = _ROCM

    def forward(self, hidden_state: torch.Tensor, smooth_scale: Optional[torch.Tensor] = None):
        out, _, scale = _layernorm_quant(self, hidden_state, None, smooth_scale, "HIPLayerNormQuant")
        return out, scale


class HIPResidualAddLayerNormQuant(MojoResidualAddLayerNormQuant):
    """Both ``norm_pos`` return ``hidden_state + residual`` in the input dtype (the reference's ``post`` does too)."""

    supported_platforms_list = _ROCM

    def forward(self, hidden_state: torch.Tensor, residual: torch.Tensor, smooth_scale: Optional[torch.Tensor] = None):
        return _layernorm_quant(self, hidden_state, residual, smooth_scale, "HIPResidualAddLayerNormQuant")


class HIPStaticQuant(MojoStaticQuant):
    supported_platforms_list = _ROCM

    def forward(self, input: torch.Tensor):
        # (the reference's own shape checks, spelled out so the body also binds to the reference's class)
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
        _check_float_input(input, "HIPStaticQuant")
        L.require_cuda(input, self.scale)
        x = _dense(input)
        scale = _as_fp32(self.scale)
        out = torch.empty(x.shape, dtype=self.quant_dtype, device=x.device)
        L.check(L.load().mojo_hip_static_quant(L.ptr(x), L.ptr(scale), L.ptr(out), x.numel(), scale.numel(), L.dtype_code(x.dtype),
                                               L.dtype_code(self.quant_dtype), L.stream_of(x)), "HIPStaticQuant")
        return out, self.scale


def dequant_scale_form(input_shape, scale_shape):
    """How ``scale`` meets ``input`` in `HIPDequant`: ``("trailing", scale elements)`` for a tensor of the input's trailing
    dimensions (leading ones aside; a single element too), ``("token", row length)`` for ``input.shape[:-1] + (1,)``; any other
    broadcast raises NotImplementedError."""
    input_shape, scale_shape = tuple(input_shape), tuple(scale_shape)
    numel = 1
    for d in scale_shape:
        numel *= d
    if len(input_shape) >= 1 and scale_shape == input_shape[:-1] + (1,):
        return "token", input_shape[-1]
    if numel == 1 and len(scale_shape) <= max(len(input_shape), 1):
        return "trailing", 1
    stripped = scale_shape
    while len(stripped) > 1 and stripped[0] == 1:
        stripped = stripped[1:]
    if len(stripped) <= len(input_shape) and input_shape[len(input_shape) - len(stripped):] == stripped:
        return "trailing", numel
    raise NotImplementedError(
        f"HIPDequant: scale of shape {scale_shape} against input of shape {input_shape}: only a scale of the input's trailing "
        f"dimensions or a per-token scale input.shape[:-1] + (1,) is supported")


class HIPDequant(MojoDequant):
    """``scale`` is a tensor of the input's trailing dimensions or a per-token ``input.shape[:-1] + (1,)`` tensor (what the
    dynamic quantisers return); another broadcast raises NotImplementedError."""

    supported_platforms_list = _ROCM

    def forward(self, input: torch.Tensor, scale: torch.Tensor):
        if input.dtype not in (torch.int8, torch.float8_e4m3fn):
            raise NotImplementedError(f"HIPDequant: input dtype {input.dtype} (int8 or float8_e4m3fn)")
        form, length = dequant_scale_form(input.shape, scale.shape)
        L.require_cuda(input, scale)
        x = _dense(input)
        s = _as_fp32(scale)
        out = torch.empty(x.shape, dtype=self.output_dtype, device=x.device)
        token_dim = length if form == "token" else 0
        L.check(L.load().mojo_hip_dequant(L.ptr(x), L.ptr(s), L.ptr(out), x.numel(), s.numel(), token_dim, L.dtype_code(x.dtype),
                                          L.dtype_code(self.output_dtype), L.stream_of(x)), "HIPDequant")
        return out


class HIPDequantSwiGLUQuant(MojoDequantSwiGLUQuant):
    """The expert of a row is found on the device from ``token_count``; nothing synchronises with the host.  The reference
    checks on the host that ``token_count`` sums to the row count and raises otherwise; this class does NOT (`HIPMoEDynamicQuant`'s
    convention): negative counts read as zero, and rows at or past ``sum(token_count)`` come back as int8 zeros with scale 1.
    With ``token_count=None`` the single expert owns every row (``expert_num`` must be 1)."""

    supported_platforms_list = _ROCM

    def forward(self, x: torch.Tensor, activation_scale: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                quant_offset: Optional[torch.Tensor] = None, token_count: Optional[torch.Tensor] = None):
        if x.dim() != 2:
            raise ValueError(f"x must be 2D with shape (tokens, 2H), but got {tuple(x.shape)}")
        if x.shape[-1] % 2 != 0:
            raise ValueError(f"x last dimension must be even for SwiGLU split, but got {x.shape[-1]}")
        if quant_offset is not None:
            raise NotImplementedError("quant_offset is not supported by the hip backend (nor by the torch reference).")
        if x.dtype not in (torch.int32, torch.float32, torch.float16, torch.bfloat16):
            raise NotImplementedError(f"HIPDequantSwiGLUQuant: x dtype {x.dtype} (int32, float32, float16 or bfloat16)")
        tokens, hidden = x.shape[0], x.shape[1] // 2
        experts = self.weight_scale.shape[0]
        if tuple(self.weight_scale.shape) != (experts, 2 * hidden) or tuple(self.quant_scale.shape) != (experts, hidden):
            raise ValueError(f"x of shape {tuple(x.shape)} does not match weight_scale {tuple(self.weight_scale.shape)} / "
                             f"quant_scale {tuple(self.quant_scale.shape)}")
        if token_count is None:
            if experts != 1:
                raise ValueError(f"token_count is required with expert_num={experts} (only a single expert can own every row).")
        else:
            if token_count.dim() != 1 or token_count.numel() != experts:
                raise ValueError(f"token_count must be 1D with {experts} entries, got shape {tuple(token_count.shape)}.")
            if token_count.dtype not in (torch.int32, torch.int64):
                raise TypeError(f"token_count must be int32 or int64, got {token_count.dtype}.")
        if activation_scale is not None and activation_scale.numel() != tokens:
            raise ValueError(f"activation_scale must hold one value per token ({tokens}), got shape {tuple(activation_scale.shape)}.")
        grouped = bias is not None and bias.dim() == 2
        if bias is not None and tuple(bias.shape) not in ((2 * hidden,), (experts, 2 * hidden)):
            raise ValueError(f"bias must have shape ({2 * hidden},) or ({experts}, {2 * hidden}), got {tuple(bias.shape)}.")
        L.require_cuda(x, activation_scale, bias, self.weight_scale, self.quant_scale)
        xd = _dense(x)
        counts = None if token_count is None else _dense(token_count.to(xd.device, non_blocking=True))
        out = torch.empty(tokens, hidden, dtype=torch.int8, device=xd.device)
        scale = torch.empty(tokens, 1, dtype=torch.float32, device=xd.device)
        if tokens == 0 or hidden == 0:
            return out, scale
        act = None if activation_scale is None else _as_fp32(activation_scale).reshape(-1)
        ws, qs, b = _as_fp32(self.weight_scale), _as_fp32(self.quant_scale), _as_fp32(bias)
        L.check(L.load().mojo_hip_dequant_swiglu_quant(
            L.ptr(xd), L.ptr(ws), L.ptr(act), L.ptr(b), 1 if grouped else 0, L.ptr(qs), L.ptr(counts),
            1 if counts is not None and counts.dtype == torch.int64 else 0, L.ptr(out), L.ptr(scale), tokens, hidden, experts,
            1 if self.activate_left else 0, L.dtype_code(xd.dtype), L.stream_of(xd)), "HIPDequantSwiGLUQuant")
        return out, scale


__all__ = ["HIPDynamicQuant", "HIPMoEDynamicQuant", "HIPResidualAddRMSNormQuant", "HIPRMSNormQuant", "HIPLayerNormQuant",
           "HIPResidualAddLayerNormQuant", "HIPStaticQuant", "HIPDequant", "HIPDequantSwiGLUQuant"]
