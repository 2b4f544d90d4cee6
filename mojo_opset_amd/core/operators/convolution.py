"""API classes of the short-convolution ops (`SHORT_CONV_OPS`): the depthwise causal convolution of width 2..4 with an optional
SiLU that stands in front of every linear-attention or state-space mixer (GatedDeltaNet, Mamba-2, the FLA family).
`MojoCausalConv1dUpdateState` is the reference's class (`mojo_opset/core/operators/convolution.py`); `MojoCausalConv1d` is the
FORWARD of the reference's `MojoCausalConv1dFunction` (`core/functions/convolution.py`) as an inference operator - the reference
has no operator class of this name, and the backward pass is out of scope.  The torch goldens live in
``tests/short_conv_golden.py``.

Arithmetic (both ops, every backend): fp32, ``acc = bias`` (or ``+0.0``), then ``acc = acc + w[k] * x[oldest + k]`` for
``k = 0 .. W - 1`` with the product and the sum rounded on their own, SiLU on the fp32 accumulator, ONE rounding to storage; the
residual of `MojoCausalConv1d` is added to the rounded value (a second rounding).  The reference's update-state op rounds the
16-bit convolution before SiLU; one rounding is more accurate and stays inside the bound tests/test_short_conv_golden.py holds
the recordings to."""
from typing import Optional, Tuple

import torch

from ..operator import MojoOperator

WIDTHS = (2, 3, 4)
MAX_STATE_LEN = 8
_FLOATS = (torch.float32, torch.bfloat16, torch.float16)


def use_silu(what: str, activation: Optional[str]) -> bool:
    if activation is None:
        return False
    if activation in ("silu", "swish"):
        return True
    raise NotImplementedError(f"{what}: activation {activation!r}; None, 'silu' and 'swish' are supported")


def check_conv_contract(what: str, dim: int, weight: torch.Tensor, state_len: Optional[int], **same_dtype) -> int:
    """The checks both ops share; returns the width.  ``same_dtype``: name -> tensor or None, each of ``weight``'s dtype."""
    if weight.dim() != 2 or weight.shape[0] != dim:
        raise ValueError(f"{what}: weight must be [dim, width] = [{dim}, W], got {tuple(weight.shape)}")
    width = weight.shape[1]
    if width not in WIDTHS:
        raise NotImplementedError(f"{what}: width {width}; {WIDTHS} are supported")
    if weight.dtype not in _FLOATS:
        raise NotImplementedError(f"{what}: dtype {weight.dtype}; float32, bfloat16 and float16 are supported")
    for name, t in same_dtype.items():
        if t is not None and t.dtype != weight.dtype:
            raise NotImplementedError(f"{what}: {name} is {t.dtype}, weight {weight.dtype}: x, weight, bias, states and residual "
                                      f"must share one dtype")
    if state_len is not None:
        if state_len < width - 1:
            raise NotImplementedError(f"{what}: a state of {state_len} columns is shorter than width - 1 = {width - 1}")
        if state_len > MAX_STATE_LEN:
            raise NotImplementedError(f"{what}: a state of {state_len} columns; up to {MAX_STATE_LEN} are supported")
    return width


class MojoCausalConv1dUpdateState(MojoOperator):
    """forward(hidden_states [B, D, T], conv_state [B, D, S], weight [D, W], bias [D] | None, activation None | 'silu' | 'swish')
    -> [B, D, T] (reference `core/operators/convolution.py:9-42`).  With ``xcat = cat(conv_state, hidden_states)`` along time,
    output ``t`` is the dot product of the ``W`` taps with ``xcat[.., S + t - W + 1 .. S + t]``, and ``conv_state`` is
    overwritten IN PLACE with the last ``S`` columns of ``xcat``.  ``S >= W - 1``; W in {2, 3, 4}, ``S <= 8``, one dtype of
    float32 / bfloat16 / float16 for every tensor: anything else raises `NotImplementedError`."""


class MojoCausalConv1d(MojoOperator):
    """forward(x, weight [D, W], bias=None, residual=None, initial_state=None, output_final_state=False, activation=None,
    cu_seqlens=None) -> (out, final_state | None): the forward of the reference's `MojoCausalConv1dFunction`
    (`core/functions/convolution.py:137-208`).  ``x`` is ``[B, T, D]``, or with ``cu_seqlens`` (int32 / int64 ``[N + 1]``)
    packed ``[1, total_T, D]``; ``initial_state`` and ``final_state`` are ``[B or N, D, W - 1]``; ``residual`` has ``x``'s shape
    and is added after the output has been rounded to storage.  Forward only: the backward pass is out of scope.

    Deviation: with ``initial_state`` given and a sequence shorter than ``W - 1`` (length 0 included) the reference pads the
    final state with zeros and drops the initial state, which is wrong for chunked prefill; here ``final_state`` is the last
    ``W - 1`` columns of ``cat(initial_state, x_seq)``.  Without ``initial_state`` the two agree."""


def check_conv1d_call(what: str, x: torch.Tensor, weight: torch.Tensor, bias, residual, initial_state,
                      cu_seqlens) -> Tuple[int, int]:
    """Shape and dtype contract of `MojoCausalConv1d.forward`; returns ``(width, sequences)``."""
    if x.dim() != 3:
        raise ValueError(f"{what}: x must be [B, T, D], got {tuple(x.shape)}")
    width = check_conv_contract(what, x.shape[2], weight, None, x=x, bias=bias, residual=residual, initial_state=initial_state)
    if bias is not None and tuple(bias.shape) != (x.shape[2],):
        raise ValueError(f"{what}: bias must be [{x.shape[2]}], got {tuple(bias.shape)}")
    if residual is not None and residual.shape != x.shape:
        raise ValueError(f"{what}: residual {tuple(residual.shape)} must have x's shape {tuple(x.shape)}")
    if cu_seqlens is not None:
        if cu_seqlens.dtype not in (torch.int32, torch.int64):
            raise NotImplementedError(f"{what}: cu_seqlens must be int32 or int64, got {cu_seqlens.dtype}")
        if x.shape[0] != 1 or cu_seqlens.dim() != 1 or cu_seqlens.numel() < 1:
            raise ValueError(f"{what}: with cu_seqlens [N + 1], x must be packed [1, total_T, D]; got x {tuple(x.shape)}, "
                             f"cu_seqlens {tuple(cu_seqlens.shape)}")
        sequences = cu_seqlens.numel() - 1
    else:
        sequences = x.shape[0]
    if initial_state is not None and tuple(initial_state.shape) != (sequences, x.shape[2], width - 1):
        raise ValueError(f"{what}: initial_state must be [{sequences}, {x.shape[2]}, {width - 1}], got {tuple(initial_state.shape)}")
    return width, sequences


def check_update_state_call(what: str, hidden_states: torch.Tensor, conv_state: torch.Tensor, weight: torch.Tensor, bias) -> int:
    """Shape and dtype contract of `MojoCausalConv1dUpdateState.forward`; returns the width."""
    if hidden_states.dim() != 3 or conv_state.dim() != 3 or conv_state.shape[:2] != hidden_states.shape[:2]:
        raise ValueError(f"{what}: hidden_states [B, D, T] and conv_state [B, D, S] expected, got {tuple(hidden_states.shape)} and "
                         f"{tuple(conv_state.shape)}")
    width = check_conv_contract(what, hidden_states.shape[1], weight, conv_state.shape[2], hidden_states=hidden_states,
                                conv_state=conv_state, bias=bias)
    if bias is not None and tuple(bias.shape) != (hidden_states.shape[1],):
        raise ValueError(f"{what}: bias must be [{hidden_states.shape[1]}], got {tuple(bias.shape)}")
    return width
