"""HIP<Op> classes of the sampling step (`SAMPLING_OPS`; kernels in csrc/sampling.hip).

The top-k stage, the nucleus mask and the draw run as two launches per call: a per-slice exact radix select, then one
workgroup per row that merges, sorts and finishes.  ``K`` is at most `MAX_K` on this path (``NotImplementedError`` above);
``-inf`` logits are legal, NaN and ``+inf`` are not supported.

Module-level functions, for callers that bring their own random numbers and for graph capture:

* `top_p_filter`: `HIPTopPFilter.forward` with the filter value as an argument;
* `sample_with_uniforms`: the selection of both samplers with one given fp32 uniform per row;
* `reject_with_uniforms`: both acceptance steps with given uniforms.

`top_p_filter` and `sample_with_uniforms` do not synchronise with the host and allocate by shape only, so they can be
captured in a graph.  ``slices`` (0: the library chooses) is the number of workgroups per row of the first launch; every
value gives the same bits.
"""
from typing import List, Optional, Union

import numpy as np
import torch

from ....core.operators.sampling import (MojoApplyPenaltiesTempurate, MojoJoinProbRejectSampling, MojoRejectSampling,
                                         MojoTopKSampling, MojoTopPFilter, MojoTopPSampling)
from .. import lib as L

_ROCM = ["rocm"]
MAX_K = 1024            # == mojo_hip_sampling_max_k()
_LOGIT_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_FREQ_KIND = {torch.int32: 0, torch.int64: 1, torch.float32: 2}
_ROW = np.dtype([("frequency", "<f4"), ("presence", "<f4"), ("repetition", "<f4"), ("temperature", "<f4"),
                 ("flags", "<i4"), ("pad", "<i4"), ("freq", "<u8")])      # the 32-byte row of mojo_hip_apply_penalties


def _dense(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous() else t.contiguous()


def _checked_k(k: int, vocab: int, what: str) -> int:
    k = min(int(k), vocab)
    if k < 1:
        raise ValueError(f"{what}: K must be at least 1, got {k}")
    if k > MAX_K:
        raise NotImplementedError(f"{what}: K = {k} is above the cap of {MAX_K} of the fused hip path")
    return k


def _rows_of(logits: torch.Tensor, what: str):
    if logits.dim() < 1 or logits.shape[-1] < 1:
        raise ValueError(f"{what}: logits must be [..., V] with V >= 1, got shape {tuple(logits.shape)}")
    if logits.dtype not in _LOGIT_DTYPES:
        raise NotImplementedError(f"{what}: logits dtype {logits.dtype}")
    vocab = logits.shape[-1]
    return logits.numel() // vocab, vocab


def workspace_bytes(rows: int, vocab: int, k: int, slices: int = 0) -> int:
    """Bytes of the candidate workspace of one call (answers without a GPU)."""
    return int(L.load().mojo_hip_sampling_workspace_bytes(rows, vocab, k, slices))


def _workspace(rows, vocab, k, slices, device):
    n = workspace_bytes(rows, vocab, k, slices)
    return torch.empty(max(n // 8, 1), dtype=torch.int64, device=device), n


def top_p_filter(logits: torch.Tensor, top_p: float, min_tokens_to_keep: int, rand_top_k: int,
                 filter_value: float = -float("inf"), slices: int = 0):
    """(final_probs_dist [..., K] in the input dtype, indices int64 [..., K]), ``K = min(rand_top_k, V)``."""
    rows, vocab = _rows_of(logits, "top_p_filter")
    k = _checked_k(rand_top_k, vocab, "top_p_filter")
    L.require_cuda(logits)
    x = _dense(logits)
    lead = tuple(x.shape[:-1])
    probs = torch.empty(lead + (k,), dtype=x.dtype, device=x.device)
    indices = torch.empty(lead + (k,), dtype=torch.int64, device=x.device)
    if rows == 0:
        return probs, indices
    ws, ws_bytes = _workspace(rows, vocab, k, slices, x.device)
    L.check(L.load().mojo_hip_top_p_filter(L.ptr(x), L.ptr(probs), L.ptr(indices), rows, vocab, k, float(top_p),
                                           int(min_tokens_to_keep), float(filter_value), int(slices), L.dtype_code(x.dtype),
                                           L.ptr(ws), ws_bytes, L.stream_of(x)), "top_p_filter")
    return probs, indices


def sample_with_uniforms(logits: torch.Tensor, uniforms: torch.Tensor, k: int, top_p: Optional[float] = None,
                         min_tokens_to_keep: int = 1, filter_value: float = -float("inf"), slices: int = 0):
    """(next_probs fp32 [..., 1], next_tokens int64 [..., 1]): per row the first of the top ``min(k, V)`` positions whose
    running sum of ``final_probs_dist`` exceeds ``uniforms[row] * total``, held to the last position of non-zero probability.
    ``top_p=None``: the distribution is the plain softmax of the top-k values.  ``uniforms``: fp32 in [0, 1), one per row."""
    rows, vocab = _rows_of(logits, "sample_with_uniforms")
    k = _checked_k(k, vocab, "sample_with_uniforms")
    L.require_cuda(logits, uniforms)
    if uniforms.dtype != torch.float32 or uniforms.numel() != rows:
        raise ValueError(f"sample_with_uniforms: uniforms must be fp32 with one value per row ({rows}), got {uniforms.dtype} "
                         f"{tuple(uniforms.shape)}")
    x, u = _dense(logits), _dense(uniforms)
    lead = tuple(x.shape[:-1])
    next_probs = torch.empty(lead + (1,), dtype=torch.float32, device=x.device)
    next_tokens = torch.empty(lead + (1,), dtype=torch.int64, device=x.device)
    if rows == 0:
        return next_probs, next_tokens
    ws, ws_bytes = _workspace(rows, vocab, k, slices, x.device)
    L.check(L.load().mojo_hip_sample_with_uniforms(
        L.ptr(x), L.ptr(u), L.ptr(next_probs), L.ptr(next_tokens), rows, vocab, k, 0 if top_p is None else 1,
        float(top_p if top_p is not None else 1.0), int(min_tokens_to_keep), float(filter_value), int(slices),
        L.dtype_code(x.dtype), L.ptr(ws), ws_bytes, L.stream_of(x)), "sample_with_uniforms")
    return next_probs, next_tokens


def _draw(logits: torch.Tensor) -> torch.Tensor:
    """One fp32 uniform per row from torch's default generator of the logits' device (``torch.manual_seed`` reproduces it)."""
    return torch.rand(logits.shape[:-1], dtype=torch.float32, device=logits.device)


class HIPTopKSampling(MojoTopKSampling):
    supported_platforms_list = _ROCM

    def forward(self, logits: torch.Tensor):
        rows, vocab = _rows_of(logits, "HIPTopKSampling")
        k = _checked_k(max(min(self.top_k, vocab), self.min_tokens_to_keep), vocab, "HIPTopKSampling")
        L.require_cuda(logits)
        return sample_with_uniforms(logits, _draw(logits), k)


class HIPTopPSampling(MojoTopPSampling):
    supported_platforms_list = _ROCM

    def forward(self, logits: torch.Tensor):
        rows, vocab = _rows_of(logits, "HIPTopPSampling")
        k = _checked_k(self.rand_top_k, vocab, "HIPTopPSampling")
        L.require_cuda(logits)
        return sample_with_uniforms(logits, _draw(logits), k, top_p=self.top_p, min_tokens_to_keep=self.min_tokens_to_keep,
                                    filter_value=self.filter_value)


class HIPTopPFilter(MojoTopPFilter):
    supported_platforms_list = _ROCM

    def forward(self, logits: torch.Tensor, top_p: float, min_tokens_to_keep: int, rand_top_k: int):
        return top_p_filter(logits, top_p, min_tokens_to_keep, rand_top_k, self.filter_value)


def reject_with_uniforms(target_probs: torch.Tensor, draft_tokens: torch.Tensor, draft_probs: torch.Tensor,
                         uniforms: torch.Tensor, joint: bool):
    """One launch of ``mojo_hip_reject_sampling``: ``uniforms`` fp32 ``[B, 1]`` (``joint=False``: `MojoRejectSampling`, int64
    lengths) or ``[B, S]`` (``joint=True``: `MojoJoinProbRejectSampling`, int32 lengths)."""
    what = "HIPJoinProbRejectSampling" if joint else "HIPRejectSampling"
    if target_probs.dim() != 3 or draft_tokens.dim() != 2 or draft_probs.shape != draft_tokens.shape:
        raise ValueError(f"{what}: target_probs [B, S+1, V], draft_tokens and draft_probs [B, S] expected, got "
                         f"{tuple(target_probs.shape)}, {tuple(draft_tokens.shape)}, {tuple(draft_probs.shape)}")
    batch, steps = draft_tokens.shape
    if target_probs.shape[0] != batch or target_probs.shape[1] < steps + 1:
        raise ValueError(f"{what}: target_probs {tuple(target_probs.shape)} does not hold {batch} x {steps + 1} positions")
    if draft_tokens.dtype != torch.int64:
        raise TypeError(f"{what}: draft_tokens must be int64, got {draft_tokens.dtype}")
    if target_probs.dtype not in _LOGIT_DTYPES or draft_probs.dtype != target_probs.dtype:
        raise NotImplementedError(f"{what}: probabilities {target_probs.dtype} / {draft_probs.dtype} (one of fp32, fp16, bf16 for both)")
    L.require_cuda(target_probs, draft_tokens, draft_probs, uniforms)
    if uniforms.dtype != torch.float32 or uniforms.numel() != batch * (steps if joint else 1):
        raise ValueError(f"{what}: uniforms must be fp32 with {'S' if joint else 'one'} per row, got {uniforms.dtype} {tuple(uniforms.shape)}")
    dev = target_probs.device
    target = _dense(target_probs[:, :steps + 1])
    next_tokens = torch.empty(batch, steps + 1, dtype=torch.int64, device=dev)
    accepted = torch.empty(batch, dtype=torch.int32 if joint else torch.int64, device=dev)
    if batch == 0:
        return next_tokens, accepted
    L.check(L.load().mojo_hip_reject_sampling(
        L.ptr(target), L.ptr(_dense(draft_tokens)), L.ptr(_dense(draft_probs)), L.ptr(_dense(uniforms)), L.ptr(next_tokens),
        L.ptr(accepted), batch, steps, target.shape[-1], 1 if joint else 0, L.dtype_code(target.dtype), L.stream_of(target)), what)
    return next_tokens, accepted


class HIPRejectSampling(MojoRejectSampling):
    supported_platforms_list = _ROCM

    def forward(self, target_probs, draft_tokens, draft_probs, random_seed: int = None):
        L.require_cuda(target_probs)
        if random_seed is not None:
            torch.manual_seed(random_seed)
        u = torch.rand(target_probs.shape[0], 1, device=target_probs.device)
        return reject_with_uniforms(target_probs, draft_tokens, draft_probs, u, False)


class HIPJoinProbRejectSampling(MojoJoinProbRejectSampling):
    supported_platforms_list = _ROCM

    def forward(self, target_probs, draft_tokens, draft_probs, random_seed: int = None):
        L.require_cuda(target_probs)
        if random_seed is not None:
            torch.manual_seed(random_seed)
        u = torch.rand(target_probs.shape[0], draft_probs.shape[1], device=target_probs.device)
        return reject_with_uniforms(target_probs, draft_tokens, draft_probs, u, True)


class HIPApplyPenaltiesTempurate(MojoApplyPenaltiesTempurate):
    """One elementwise launch over ``[B, V]``, driven by a per-row table that is built on the host from the Python lists (four
    fp32 parameters, which steps run, the address of the row's frequency vector) and copied to the device: the lists make
    this operator host-driven by its API, so it is NOT captured in a graph.  Frequency rows that arrive on the CPU are moved
    to the device; all of them must share one dtype among int32, int64 and fp32."""

    supported_platforms_list = _ROCM

    def forward(self, logits: torch.Tensor, token_freqs: List[Union[None, torch.Tensor]], presence_penalties: List[float],
                frequency_penalties: List[float], repetition_penalties: List[float],
                temps: Optional[List[Optional[float]]] = None) -> torch.Tensor:
        MojoApplyPenaltiesTempurate.check_call_contract(logits, token_freqs, presence_penalties, frequency_penalties,
                                                        repetition_penalties, temps)
        if logits.dtype not in _LOGIT_DTYPES:
            raise NotImplementedError(f"HIPApplyPenaltiesTempurate: logits dtype {logits.dtype}")
        kinds = {f.dtype for f in token_freqs if f is not None}
        if len(kinds) > 1 or not kinds <= set(_FREQ_KIND):
            raise NotImplementedError(f"HIPApplyPenaltiesTempurate: the frequency rows must share one dtype among int32, int64 "
                                      f"and float32, got {sorted(str(d) for d in kinds)}")
        L.require_cuda(logits)
        rows, vocab = logits.shape
        x = _dense(logits)
        out = x if x.dtype == torch.float32 else torch.empty_like(x)
        if rows == 0 or vocab == 0:
            return logits if logits.dtype == torch.float32 else out
        table = np.zeros(rows, dtype=_ROW)
        held = []                                                # device copies stay alive until the launch is queued
        for i, freq in enumerate(token_freqs):
            flags = 0
            if freq is not None:
                f = _dense(freq.to(x.device, non_blocking=True))
                held.append(f)
                table["freq"][i] = f.data_ptr()
                flags |= (1 if frequency_penalties[i] != 0.0 else 0) | (2 if presence_penalties[i] != 0.0 else 0) | \
                         (4 if repetition_penalties[i] != 1.0 else 0)
                table["frequency"][i], table["presence"][i] = frequency_penalties[i], presence_penalties[i]
                table["repetition"][i] = repetition_penalties[i]
            if temps is not None and temps[i] is not None:
                flags |= 8
                table["temperature"][i] = temps[i]
            table["flags"][i] = flags
        dev_table = torch.from_numpy(table.view(np.uint8).reshape(rows, _ROW.itemsize)).to(x.device)
        L.check(L.load().mojo_hip_apply_penalties(L.ptr(x), L.ptr(out), L.ptr(dev_table), rows, vocab, L.dtype_code(x.dtype),
                                                  _FREQ_KIND[next(iter(kinds))] if kinds else 0, L.stream_of(x)),
                "HIPApplyPenaltiesTempurate")
        if logits.dtype == torch.float32:
            if x is not logits:                                  # a strided fp32 input is still updated in place
                logits.copy_(x)
            return logits
        return out


__all__ = ["HIPTopKSampling", "HIPTopPSampling", "HIPTopPFilter", "HIPRejectSampling", "HIPJoinProbRejectSampling",
           "HIPApplyPenaltiesTempurate", "MAX_K", "top_p_filter", "sample_with_uniforms", "reject_with_uniforms", "workspace_bytes"]
