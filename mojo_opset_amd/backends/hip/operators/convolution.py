"""HIP<Op> classes of the short-convolution ops (`SHORT_CONV_OPS`): `MojoCausalConv1dUpdateState` and `MojoCausalConv1d`
(csrc/causal_conv1d.hip).  Both are one launch of `mojo_hip_causal_conv1d`; the kernel follows the layout of the
input, not the op called: channel-contiguous (``stride(D) == 1``: `MojoCausalConv1d`'s natural ``[B, T, D]``, and the update-state
op on ``y.transpose(1, 2)`` of a projection output) or time-contiguous (``stride(T) == 1``: the reference's literal ``[B, D, T]``).
Any other stride pattern is made dense once.  ``cu_seqlens`` is read on the device: no forward synchronises with the host, and
both ops can be captured in a graph."""
from typing import Optional

import torch

from ....core.operators.convolution import (MojoCausalConv1d, MojoCausalConv1dUpdateState, check_conv1d_call,
                                            check_update_state_call, use_silu)
from .. import lib as L

_ROCM = ["rocm"]


def run_tokens() -> int:
    """Tokens a thread of the channel-contiguous kernel walks."""
    return int(L.load().mojo_hip_causal_conv1d_run_tokens())


def row_thread_max_t() -> int:
    """The longest time-contiguous row that takes one thread; longer rows are walked in vectors."""
    return int(L.load().mojo_hip_causal_conv1d_row_thread_max_t())


def _state_rows(state: torch.Tensor) -> bool:
    """Whether the kernel can address ``[N, D, S]`` in place: columns dense and no two rows overlapping - the rows of one
    dimension at least a row apart and the other dimension's step at least the whole extent of the first (either nesting).  One
    thread owns one row of the in-place update, so a view whose rows share memory (``as_strided`` with equal strides) is copied."""
    n, d, s = state.shape
    if not (s == 1 or state.stride(2) == 1):
        return False
    sn, sd = (state.stride(0) if n > 1 else None), (state.stride(1) if d > 1 else None)
    if sn is None or sd is None:
        return (sn is None or sn >= s) and (sd is None or sd >= s)
    return (sd >= s and sn >= d * sd) or (sn >= s and sd >= n * sn)


def _launch(what, x, x_strides, batch, seq_len, dim, weight, bias, residual, res_strides, state_in, state_out, out, out_strides,
            cu_seqlens, silu):
    """``x``, ``out`` and ``residual`` with their (batch, time, dim) strides; the states are ``[N, D, S]`` with dense columns."""
    L.require_cuda(x, weight, bias, residual, state_in, state_out, out, cu_seqlens)
    state = state_out if state_out is not None else state_in
    state_len = state.shape[2] if state is not None else weight.shape[1] - 1
    si = (state_in.stride(0), state_in.stride(1)) if state_in is not None else (0, 0)
    so = (state_out.stride(0), state_out.stride(1)) if state_out is not None else (0, 0)
    L.check(L.load().mojo_hip_causal_conv1d(
        L.ptr(x), L.ptr(weight), L.ptr(bias), L.ptr(residual), L.ptr(state_in), L.ptr(state_out), L.ptr(out), L.ptr(cu_seqlens),
        1 if cu_seqlens is not None and cu_seqlens.dtype == torch.int64 else 0, batch, seq_len, dim, weight.shape[1], state_len,
        *x_strides, *out_strides, *(res_strides if residual is not None else (0, 0, 0)), *si, *so, 1 if silu else 0,
        L.dtype_code(weight.dtype), L.stream_of(weight)), what)


class HIPCausalConv1dUpdateState(MojoCausalConv1dUpdateState):
    """One launch computes the outputs and rewrites ``conv_state`` in place: the one thread that reads a row of the old state
    is the one that writes its new state, after its reads.  ``hidden_states`` is read in place when its time or its channel
    stride is 1 (a column slice of a fused projection included) and made dense once otherwise; a channel-contiguous view
    (``y.transpose(1, 2)`` of a ``[B, T, D]`` tensor) gets its output with the same strides, a transposed view of a fresh
    ``[B, T, D]`` buffer.  The ``T = 1`` decode call makes no host synchronisation and can be captured in a graph."""
    supported_platforms_list = _ROCM

    def forward(self, hidden_states: torch.Tensor, conv_state: torch.Tensor, weight: torch.Tensor,
                bias: Optional[torch.Tensor] = None, activation: Optional[str] = None) -> torch.Tensor:
        what = "HIPCausalConv1dUpdateState"
        silu = use_silu(what, activation)
        check_update_state_call(what, hidden_states, conv_state, weight, bias)
        batch, dim, seq_len = hidden_states.shape
        x = hidden_states
        if x.stride(2) != 1 and not (dim == 1 or x.stride(1) == 1):
            x = x.contiguous()
        if x.stride(2) == 1:                                            # time-contiguous (a dense [B, D, 1] decode column too)
            out = torch.empty((batch, dim, seq_len), dtype=x.dtype, device=x.device)
            x_strides, out_strides = (x.stride(0), 1, x.stride(1)), (out.stride(0), 1, out.stride(1))
        else:                                                           # channel-contiguous: the output keeps the view's strides
            out = torch.empty((batch, seq_len, dim), dtype=x.dtype, device=x.device).transpose(1, 2)
            x_strides, out_strides = (x.stride(0), x.stride(2), 1), (out.stride(0), out.stride(2), 1)
        if out.numel() == 0 and seq_len > 0:
            return out
        state = conv_state if _state_rows(conv_state) else conv_state.contiguous()
        if seq_len > 0:
            _launch(what, x, x_strides, batch, seq_len, dim, weight.contiguous(), None if bias is None else bias.contiguous(),
                    None, None, state, state, out, out_strides, None, silu)
        if state is not conv_state:
            conv_state.copy_(state)
        return out


class HIPCausalConv1d(MojoCausalConv1d):
    """One launch: outputs, the residual add and every sequence's final state.  ``x`` is read in place when its channel stride
    is 1 (rows by a stride: a column slice of a fused projection buffer) or, batched, when its time stride is 1; anything else is
    made dense once.  ``cu_seqlens`` stays on the device: a run of tokens finds its sequence there, and a token within ``W - 1``
    of its sequence's start takes its missing inputs from ``initial_state`` or zero, never from the previous sequence.  A token
    outside every sequence of ``cu_seqlens`` gets zeros.  ``final_state`` is a fresh tensor, so it never aliases
    ``initial_state``.  Forward only."""
    supported_platforms_list = _ROCM

    def forward(self, x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
                residual: Optional[torch.Tensor] = None, initial_state: Optional[torch.Tensor] = None,
                output_final_state: bool = False, activation: Optional[str] = None,
                cu_seqlens: Optional[torch.Tensor] = None):
        what = "HIPCausalConv1d"
        silu = use_silu(what, activation)
        width, sequences = check_conv1d_call(what, x, weight, bias, residual, initial_state, cu_seqlens)
        batch, seq_len, dim = x.shape
        time_form = cu_seqlens is None and x.stride(1) == 1
        if not time_form and not (dim == 1 or x.stride(2) == 1):
            x = x.contiguous()
            time_form = cu_seqlens is None and x.stride(1) == 1
        if time_form:
            out = torch.empty((batch, dim, seq_len), dtype=x.dtype, device=x.device).transpose(1, 2)
            if residual is not None and residual.stride(1) != 1:
                residual = residual.transpose(1, 2).contiguous().transpose(1, 2)
            strides = lambda t: (t.stride(0), 1, t.stride(2))           # noqa: E731  [B, T, D]: (batch, time, dim)
        else:
            out = torch.empty((batch, seq_len, dim), dtype=x.dtype, device=x.device)
            if residual is not None and not (dim == 1 or residual.stride(2) == 1):
                residual = residual.contiguous()
            strides = lambda t: (t.stride(0), t.stride(1), 1)           # noqa: E731
        final_state = None
        if output_final_state:
            final_state = torch.empty((sequences, dim, width - 1), dtype=x.dtype, device=x.device)
        if initial_state is not None and not _state_rows(initial_state):
            initial_state = initial_state.contiguous()
        if dim == 0 or (cu_seqlens is None and x.numel() == 0):
            if final_state is not None:
                final_state.copy_(initial_state) if initial_state is not None else final_state.zero_()
            return out, final_state
        _launch(what, x, strides(x), sequences if cu_seqlens is not None else batch, seq_len, dim, weight.contiguous(),
                None if bias is None else bias.contiguous(), residual, None if residual is None else strides(residual),
                initial_state, final_state, out, strides(out), None if cu_seqlens is None else cu_seqlens.contiguous(), silu)
        return out, final_state
