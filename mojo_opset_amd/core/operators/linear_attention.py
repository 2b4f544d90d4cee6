"""API classes of the gated-delta-rule ops (`LINEAR_ATTN_OPS`): the linear recurrence that is the mixer of a GatedDeltaNet layer
(Qwen3-Next, the FLA family), as a prefill operator and a decode / short-verify state update.  The reference has no class for
either; semantics follow the published gated delta rule (FLA's ``chunk_gated_delta_rule`` / ``fused_recurrent_gated_delta_rule``).

Per sequence and value head ``h`` there is an fp32 state ``S [Dk, Dv]``; the key head is ``h // (Hv / Hk)``.  With
``use_qk_l2norm``, ``q^ = q * rsqrt(sum q^2 + 1e-6)`` and ``k^`` likewise, else ``q^ = q``, ``k^ = k``.  For each token in order::

    S  = exp(g_t) * S
    d  = beta_t * (v_t - S^T k^_t)
    S  = S + outer(k^_t, d)
    o_t = scale * S^T q^_t                    # scale defaults to Dk ** -0.5

``forward`` of the two classes is the golden: this loop in fp32, one rounding of ``o`` to storage."""
from typing import Optional, Tuple

import torch

from ..operator import MojoOperator

HEAD_DIMS = (64, 128)
MAX_UPDATE_TOKENS = 8
L2_EPS = 1e-6


def check_gated_delta_contract(what: str, q, k, v, g, beta, dtypes) -> Tuple[int, int, int, int, int, int]:
    """The checks both ops share; returns ``(B, T, Hk, Hv, Dk, Dv)``.  ``dtypes``: the storage dtypes of q / k / v."""
    if q.dim() != 4 or k.shape != q.shape or v.dim() != 4 or v.shape[:2] != q.shape[:2]:
        raise ValueError(f"{what}: q / k [B, T, Hk, Dk] and v [B, T, Hv, Dv] expected, got {tuple(q.shape)}, {tuple(k.shape)}, "
                         f"{tuple(v.shape)}")
    (batch, tokens, hk, dk), (hv, dv) = q.shape, v.shape[2:]
    if tuple(g.shape) != (batch, tokens, hv) or tuple(beta.shape) != (batch, tokens, hv):
        raise ValueError(f"{what}: g and beta must be [{batch}, {tokens}, {hv}], got {tuple(g.shape)} and {tuple(beta.shape)}")
    if dk not in HEAD_DIMS or dv not in HEAD_DIMS:
        raise NotImplementedError(f"{what}: Dk {dk} / Dv {dv}; {HEAD_DIMS} are supported")
    if hk <= 0 or hv % hk != 0:
        raise NotImplementedError(f"{what}: {hv} value heads are no multiple of {hk} key heads")
    if q.dtype not in dtypes or k.dtype != q.dtype or v.dtype != q.dtype:
        raise NotImplementedError(f"{what}: q, k and v must share one of {dtypes}, got {q.dtype} / {k.dtype} / {v.dtype}")
    for name, t in (("g", g), ("beta", beta)):
        if t.dtype not in (torch.float32, q.dtype):
            raise NotImplementedError(f"{what}: {name} is {t.dtype}; float32 or {q.dtype} are supported")
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.stride(3) != 1 or any(t.stride(i) * t.element_size() % 16 for i in range(3) if t.shape[i] > 1):
            raise NotImplementedError(f"{what}: {name} must be dense in the head dimension with batch, token and head strides "
                                      f"that are multiples of 16 bytes, got strides {t.stride()}")
    return batch, tokens, hk, hv, dk, dv


def check_state(what: str, name: str, state: torch.Tensor, shape) -> None:
    if tuple(state.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} must be {tuple(shape)}, got {tuple(state.shape)}")
    if state.dtype != torch.float32 or not state.is_contiguous():
        raise NotImplementedError(f"{what}: {name} must be contiguous float32, got {state.dtype}, strides {state.stride()}")


def check_prefill_call(what: str, q, k, v, g, beta, initial_state, cu_seqlens) -> Tuple[int, ...]:
    """Contract of `MojoGatedDeltaRule.forward`; returns ``(B, T, Hk, Hv, Dk, Dv, sequences)``."""
    dims = check_gated_delta_contract(what, q, k, v, g, beta, (torch.bfloat16,))
    sequences = dims[0]
    if cu_seqlens is not None:
        if cu_seqlens.dtype not in (torch.int32, torch.int64):
            raise NotImplementedError(f"{what}: cu_seqlens must be int32 or int64, got {cu_seqlens.dtype}")
        if dims[0] != 1 or cu_seqlens.dim() != 1 or cu_seqlens.numel() < 1:
            raise ValueError(f"{what}: with cu_seqlens [N + 1] the batch is packed [1, total_T, ...]; got q {tuple(q.shape)}, "
                             f"cu_seqlens {tuple(cu_seqlens.shape)}")
        sequences = cu_seqlens.numel() - 1
    if initial_state is not None:
        check_state(what, "initial_state", initial_state, (sequences, dims[3], dims[4], dims[5]))
    return (*dims, sequences)


def check_update_call(what: str, q, k, v, g, beta, state) -> Tuple[int, ...]:
    """Contract of `MojoGatedDeltaRuleUpdateState.forward`; returns ``(B, T, Hk, Hv, Dk, Dv)``."""
    dims = check_gated_delta_contract(what, q, k, v, g, beta, (torch.bfloat16, torch.float16))
    if not 1 <= dims[1] <= MAX_UPDATE_TOKENS:
        raise NotImplementedError(f"{what}: {dims[1]} tokens; 1 to {MAX_UPDATE_TOKENS} are supported (longer runs: MojoGatedDeltaRule)")
    check_state(what, "state", state, (dims[0], dims[3], dims[4], dims[5]))
    return dims


def recurrent_gated_delta_rule(q, k, v, g, beta, state, scale, use_qk_l2norm):
    """The token loop in fp32 on ``[T, Hk, Dk]`` / ``[T, Hv, Dv]`` / ``[T, Hv]`` of one sequence; ``state [Hv, Dk, Dv]`` fp32 is
    updated in place.  Returns ``o [T, Hv, Dv]`` in fp32."""
    group = v.shape[1] // q.shape[1]
    q, k, v, g, beta = (t.float() for t in (q, k, v, g, beta))
    if use_qk_l2norm:
        q = q * torch.rsqrt((q * q).sum(-1, keepdim=True) + L2_EPS)
        k = k * torch.rsqrt((k * k).sum(-1, keepdim=True) + L2_EPS)
    q, k = q.repeat_interleave(group, dim=1), k.repeat_interleave(group, dim=1)
    out = torch.empty_like(v)
    for t in range(q.shape[0]):
        state *= torch.exp(g[t])[:, None, None]
        d = beta[t][:, None] * (v[t] - torch.einsum("hkv,hk->hv", state, k[t]))
        state += k[t][:, :, None] * d[:, None, :]
        out[t] = scale * torch.einsum("hkv,hk->hv", state, q[t])
    return out


class MojoGatedDeltaRule(MojoOperator):
    """forward(q, k, v, g, beta, scale=None, initial_state=None, output_final_state=False, cu_seqlens=None)
    -> (out, final_state | None).  ``q`` / ``k`` ``[B, T, Hk, Dk]``, ``v`` ``[B, T, Hv, Dv]``, ``g`` (log decay, <= 0) and ``beta``
    ``[B, T, Hv]``; with ``cu_seqlens`` (int32 / int64 ``[N + 1]``) the batch is packed ``[1, total_T, ...]``.  ``initial_state``
    and ``final_state`` are fp32 ``[B or N, Hv, Dk, Dv]``; ``final_state`` is a new tensor.  A sequence of length 0 writes no
    output row and its final state is its initial state, or zeros.  A packed token outside every sequence gets zeros."""

    def __init__(self, use_qk_l2norm: bool = True, **kwargs):
        super().__init__(**kwargs)
        self.use_qk_l2norm = use_qk_l2norm

    def extra_repr(self) -> str:
        return f"use_qk_l2norm={self.use_qk_l2norm}"

    def forward(self, q, k, v, g, beta, scale: Optional[float] = None, initial_state: Optional[torch.Tensor] = None,
                output_final_state: bool = False, cu_seqlens: Optional[torch.Tensor] = None):
        batch, tokens, _, hv, dk, dv, sequences = check_prefill_call("MojoGatedDeltaRule", q, k, v, g, beta, initial_state,
                                                                     cu_seqlens)
        scale = dk ** -0.5 if scale is None else float(scale)
        out = torch.zeros_like(v)
        state = (torch.zeros(sequences, hv, dk, dv, dtype=torch.float32, device=q.device) if initial_state is None
                 else initial_state.clone())
        bounds = None if cu_seqlens is None else [min(max(int(c), 0), tokens) for c in cu_seqlens.tolist()]
        for s in range(sequences):
            b, t0, t1 = (s, 0, tokens) if bounds is None else (0, bounds[s], bounds[s + 1])
            if t1 > t0:
                out[b, t0:t1] = recurrent_gated_delta_rule(q[b, t0:t1], k[b, t0:t1], v[b, t0:t1], g[b, t0:t1], beta[b, t0:t1],
                                                           state[s], scale, self.use_qk_l2norm).to(out.dtype)
        return out, (state if output_final_state else None)


class MojoGatedDeltaRuleUpdateState(MojoOperator):
    """forward(q, k, v, g, beta, state, scale=None) -> out: the same shapes with ``1 <= T <= 8`` (the decode step and the short
    verify step of multi-token prediction); ``state`` fp32 ``[B, Hv, Dk, Dv]`` is rewritten IN PLACE with the state after the
    last token."""

    def __init__(self, use_qk_l2norm: bool = True, **kwargs):
        super().__init__(**kwargs)
        self.use_qk_l2norm = use_qk_l2norm

    def extra_repr(self) -> str:
        return f"use_qk_l2norm={self.use_qk_l2norm}"

    def forward(self, q, k, v, g, beta, state, scale: Optional[float] = None):
        batch, _, _, _, dk, _ = check_update_call("MojoGatedDeltaRuleUpdateState", q, k, v, g, beta, state)
        scale = dk ** -0.5 if scale is None else float(scale)
        out = torch.empty_like(v)
        for b in range(batch):
            out[b] = recurrent_gated_delta_rule(q[b], k[b], v[b], g[b], beta[b], state[b], scale, self.use_qk_l2norm).to(out.dtype)
        return out
