"""HIP<Op> classes of the gated-delta-rule ops (`LINEAR_ATTN_OPS`): `MojoGatedDeltaRule` and `MojoGatedDeltaRuleUpdateState` on
csrc/gated_delta_rule.hip.  The prefill op is one launch of the chunked kernel on the matrix cores, the update
op one launch of the streaming kernel.  Everything outside the envelope raises ``NotImplementedError`` on the host, before any
device work."""
from typing import Optional

import torch

from ....core.operators.linear_attention import (MojoGatedDeltaRule, MojoGatedDeltaRuleUpdateState, check_prefill_call,
                                                 check_update_call)
from .. import lib as L

__all__ = ["HIPGatedDeltaRule", "HIPGatedDeltaRuleUpdateState"]

_ENVELOPE = """Envelope: ``Dk``, ``Dv`` 64 / 128 (independently), ``Hv % Hk == 0``; ``q`` / ``k`` / ``v`` / ``out`` share bf16 (the update op:
    bf16 or fp16), ``g`` / ``beta`` fp32 or that dtype; states fp32 and contiguous.  ``q`` / ``k`` / ``v`` are read in place
    when dense in the head dimension with batch, token and head strides that are multiples of 16 bytes (the three column
    slices of one fused ``[B, T, 2 Hk Dk + Hv Dv]`` convolution output), anything else raises.  No host sync (``cu_seqlens``
    is read on the device), capture-safe, no atomics: two calls give the same bits.  `mojo_hip_last_launch()` names the
    form taken."""


def _strides(t: torch.Tensor):
    return tuple(t.stride(i) if t.shape[i] > 1 else 0 for i in range(3))   # (a dimension of one element has no step)


def _gates(what, g, beta):
    if g.dtype != beta.dtype:
        raise NotImplementedError(f"{what}: g is {g.dtype}, beta {beta.dtype}: the two must share a dtype")
    return g.contiguous(), beta.contiguous()


def dv_slice_plan(sequences: int, value_heads: int, dv: int, dv_slice: Optional[int] = None) -> int:
    """State columns per workgroup of the prefill kernel: what `HIPGatedDeltaRule` takes for ``dv_slice`` (None = planned)."""
    return int(L.load().mojo_hip_gated_delta_rule_dv_slice(sequences, value_heads, dv, 0 if dv_slice is None else int(dv_slice)))


class HIPGatedDeltaRule(MojoGatedDeltaRule):
    __doc__ = f"""The gated delta rule over whole sequences, batched or packed by ``cu_seqlens``: the chunked (WY) form, 64 tokens a
    chunk, one workgroup per (sequence, value head, slice of ``dv_slice`` state columns) with the state slice in registers.
    ``dv_slice``: ``None`` = planned from the shapes (64 once the slices of 64 alone fill the CUs, else 32), 32 or 64 forces.
    ``final_state`` is a fresh tensor.  Packed rows outside every sequence are zeros.

    {_ENVELOPE}"""
    supported_platforms_list = ["rocm"]

    def forward(self, q, k, v, g, beta, scale: Optional[float] = None, initial_state: Optional[torch.Tensor] = None,
                output_final_state: bool = False, cu_seqlens: Optional[torch.Tensor] = None, *, dv_slice: Optional[int] = None):
        what = "HIPGatedDeltaRule"
        batch, tokens, hk, hv, dk, dv, sequences = check_prefill_call(what, q, k, v, g, beta, initial_state, cu_seqlens)
        if dv_slice not in (None, 32, 64):
            raise ValueError(f"{what}: dv_slice must be None, 32 or 64, got {dv_slice}")
        g, beta = _gates(what, g, beta)
        L.require_cuda(q, k, v, g, beta, initial_state, cu_seqlens)
        out = (torch.empty if cu_seqlens is None else torch.zeros)((batch, tokens, hv, dv), dtype=v.dtype, device=v.device)
        final_state = None
        if output_final_state:
            final_state = torch.empty((sequences, hv, dk, dv), dtype=torch.float32, device=v.device)
        if sequences == 0 or (tokens == 0 and final_state is None):
            return out, final_state
        cu = None if cu_seqlens is None else cu_seqlens.contiguous()
        L.check(L.load().mojo_hip_gated_delta_rule(
            L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(g), L.ptr(beta), L.ptr(initial_state), L.ptr(final_state), L.ptr(out), L.ptr(cu),
            1 if cu is not None and cu.dtype == torch.int64 else 0, sequences, tokens, hk, hv, dk, dv, *_strides(q), *_strides(k),
            *_strides(v), dk ** -0.5 if scale is None else float(scale), 1 if self.use_qk_l2norm else 0, L.dtype_code(g.dtype),
            L.dtype_code(q.dtype), 0 if dv_slice is None else dv_slice, L.stream_of(q)), what)
        return out, final_state


class HIPGatedDeltaRuleUpdateState(MojoGatedDeltaRuleUpdateState):
    __doc__ = f"""The gated delta rule for 1 to 8 tokens per sequence (decode, the verify step of multi-token prediction): one streaming
    launch, a workgroup per (sequence, value head, 32 state columns) with its state rows in registers; ``state`` is read once
    and rewritten in place with the state after the last token.  One fixed order: ``S^T k`` and ``d`` in fp64 (``d`` is a difference
    of nearly equal numbers once the state has learned the key), every state element rounded once per token, ``S^T q`` in
    fp32, one rounding of the output.

    {_ENVELOPE}"""
    supported_platforms_list = ["rocm"]

    def forward(self, q, k, v, g, beta, state, scale: Optional[float] = None):
        what = "HIPGatedDeltaRuleUpdateState"
        batch, tokens, hk, hv, dk, dv = check_update_call(what, q, k, v, g, beta, state)
        g, beta = _gates(what, g, beta)
        L.require_cuda(q, k, v, g, beta, state)
        out = torch.empty((batch, tokens, hv, dv), dtype=v.dtype, device=v.device)
        if batch == 0:
            return out
        L.check(L.load().mojo_hip_gated_delta_rule_update(
            L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(g), L.ptr(beta), L.ptr(state), L.ptr(out), batch, tokens, hk, hv, dk, dv,
            *_strides(q), *_strides(k), *_strides(v), dk ** -0.5 if scale is None else float(scale),
            1 if self.use_qk_l2norm else 0, L.dtype_code(g.dtype), L.dtype_code(q.dtype), L.stream_of(q)), what)
        return out
