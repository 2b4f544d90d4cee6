"""Torch goldens of the sliding-window pair (`MojoPagedDecodeSWA`, `MojoPagedPrefillSWA`).

Importing this module registers ``TorchPagedDecodeSWA`` / ``TorchPagedPrefillSWA`` as the ``torch`` backends of the two
API classes.

Semantics and rounding points restate `mojo_opset/core/operators/attention.py:507-531` (the window mask), :561-650
(prefill) and :683-741 (decode): scores are a 16-bit ``bmm`` upcast to fp32 and scaled, masked with -inf outside the
visible set, softmax statistics in fp32, the unnormalised probabilities rounded to the storage type, a 16-bit ``bmm``
against V, upcast and divided by the fp32 row sum.  Pages are gathered by plain indexing of the table
(`paged.index_pages`).  `tests/golden/paged_swa.pt` pins these classes bit for bit.
"""
import math
from typing import Optional

import torch

from mojo_opset_amd.core.operators import attention as _attn

from .paged import expand_kv_heads, index_pages, window_mask

_CPU = ["rocm", "cpu"]


def _attend(op, q_i, k_i, v_i, kv_len, scale):
    """q_i [Hq, q_len, D], k_i / v_i [Hkv, kv_len, D] -> [Hq, q_len, D] fp32 (before the final cast)."""
    group = q_i.shape[0] // k_i.shape[0]
    k_t = expand_kv_heads(k_i.permute(0, 2, 1), group, op.gqa_layout)
    s = torch.bmm(q_i, k_t).float() * scale
    if op.is_causal:
        s = torch.where(window_mask(q_i.shape[1], kv_len, op.local_window_size, op.global_window_size).to(s.device),
                        s, float("-inf"))
    s = s - torch.max(s, dim=-1, keepdim=True).values
    p = torch.exp(s)
    denom = torch.sum(p, dim=-1, keepdim=True)
    return torch.bmm(p.to(q_i.dtype), expand_kv_heads(v_i, group, op.gqa_layout)).float() / denom


class TorchPagedDecodeSWA(_attn.MojoPagedDecodeSWA):
    """Reference :683-741: one query per sequence at position ``kv_len - 1``; rows with ``kv_len <= 0`` are zeros."""

    supported_platforms_list = _CPU

    def forward(self, query, key_cache, value_cache, total_seq_lens, block_table, softmax_scale: Optional[float] = None,
                *, max_total_seq_len: Optional[int] = None):
        _attn.assert_paged_decode_contract(block_table, total_seq_lens)
        dim = query.shape[2]
        scale = 1.0 / math.sqrt(dim) if softmax_scale is None else softmax_scale
        out = torch.zeros_like(query)
        for b, kv_len in enumerate(total_seq_lens.tolist()):
            if kv_len <= 0:
                continue
            if int(block_table[b, 0]) < 0:
                raise ValueError("Paged decode requires a valid block table for rows with kv lens > 0.")
            o = _attend(self, query[b].unsqueeze(1), index_pages(key_cache, block_table[b], kv_len),
                        index_pages(value_cache, block_table[b], kv_len), kv_len, scale)
            out[b] = o.squeeze(1).to(out.dtype)
        return out


class TorchPagedPrefillSWA(_attn.MojoPagedPrefillSWA):
    """Reference :561-650: packed queries, row i of a sequence at position ``kv_len - q_len + i``.  Rows of padding
    tokens and of sequences without keys are zeros (the reference leaves them uninitialised)."""

    supported_platforms_list = _CPU

    def forward(self, query, key_cache, value_cache, cu_q_lens, block_table, softmax_scale: Optional[float] = None,
                cu_total_seq_lens: Optional[torch.Tensor] = None, *, max_q_len: Optional[int] = None,
                max_total_seq_len: Optional[int] = None):
        _attn.assert_paged_prefill_contract(cu_q_lens, block_table, cu_total_seq_lens)
        dim = query.shape[2]
        scale = 1.0 / math.sqrt(dim) if softmax_scale is None else softmax_scale
        cu_q = cu_q_lens.tolist()
        cu_kv = cu_q if cu_total_seq_lens is None else cu_total_seq_lens.tolist()
        out = torch.zeros_like(query)
        for b in range(len(cu_q) - 1):
            lo, hi = cu_q[b], cu_q[b + 1]
            kv_len = cu_kv[b + 1] - cu_kv[b]
            if hi == lo or kv_len <= 0:
                continue
            if int(block_table[b, 0]) < 0:
                raise ValueError("Paged prefill requires a valid block table for rows with kv lens > 0.")
            o = _attend(self, query[lo:hi].permute(1, 0, 2), index_pages(key_cache, block_table[b], kv_len),
                        index_pages(value_cache, block_table[b], kv_len), kv_len, scale)
            out[lo:hi] = o.permute(1, 0, 2).to(out.dtype)
        return out
