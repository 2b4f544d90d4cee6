"""Torch goldens of the sliding-window pair (`MojoPagedDecodeSWA`, `MojoPagedPrefillSWA`).

Ops beyond the SURVEY §8 set carry their goldens here, in the tests, not in the repo-level `oracle/` package.  Importing
this module registers ``TorchPagedDecodeSWA`` / ``TorchPagedPrefillSWA`` as the ``torch`` backends of the two API classes.

Semantics and rounding points restate `mojo_opset/core/operators/attention.py:507-531` (the window mask), :561-650
(prefill) and :683-741 (decode): scores are a 16-bit ``bmm`` upcast to fp32 and scaled, masked with -inf outside the
visible set, softmax statistics in fp32, the unnormalised probabilities rounded to the storage type, a 16-bit ``bmm``
against V, upcast and divided by the fp32 row sum.  Pages are gathered by plain indexing of the table (a negative id
indexes from the end of the cache, as in the reference).  `tests/golden/paged_swa.pt` pins these classes bit for bit.
"""
import math
from typing import Optional

import torch

from mojo_opset_amd.core.operators import attention as _attn

_CPU = ["rocm", "cpu"]


def window_mask(q_len: int, kv_len: int, local: Optional[int], glob: Optional[int]) -> torch.Tensor:
    """``[q_len, kv_len]`` bool: row i (position ``p = kv_len - q_len + i``) sees key j iff ``j <= p`` and, when a window
    is set, ``j >= p - local`` or ``j < glob`` (reference :507-531)."""
    pos = torch.arange(q_len)[:, None] + (kv_len - q_len)
    key = torch.arange(kv_len)[None, :]
    mask = key <= pos
    if local is not None or glob is not None:
        win = torch.zeros(q_len, kv_len, dtype=torch.bool)
        if local is not None:
            win |= pos <= key + local
        if glob is not None:
            win |= key < glob
        mask &= win
    return mask


def _pages(cache, table_row, kv_len):
    """``[Hkv, kv_len, D]`` of one sequence: its first ceil(kv_len / page) pages, token-major."""
    n_kv, page, dim = cache.shape[1], cache.shape[2], cache.shape[3]
    blocks = (kv_len + page - 1) // page
    x = cache[table_row[:blocks].long()]                             # [blocks, Hkv, page, D]
    return x.permute(1, 0, 2, 3).reshape(n_kv, blocks * page, dim)[:, :kv_len]


def _expand(x, group, interleave):
    """``[Hkv, S, D] -> [Hq, S, D]``: ABAB tiles the kv heads, AABB repeats each one."""
    if group == 1:
        return x
    return x.repeat((group, 1, 1)) if interleave else x.repeat_interleave(group, dim=0)


def _attend(op, q_i, k_i, v_i, kv_len, scale):
    """q_i [Hq, q_len, D], k_i / v_i [Hkv, kv_len, D] -> [Hq, q_len, D] fp32 (before the final cast)."""
    group = q_i.shape[0] // k_i.shape[0]
    interleave = op.gqa_layout == "ABAB"
    k_t = _expand(k_i.permute(0, 2, 1), group, interleave)
    s = torch.bmm(q_i, k_t).float() * scale
    if op.is_causal:
        s = torch.where(window_mask(q_i.shape[1], kv_len, op.local_window_size, op.global_window_size).to(s.device),
                        s, float("-inf"))
    s = s - torch.max(s, dim=-1, keepdim=True).values
    p = torch.exp(s)
    denom = torch.sum(p, dim=-1, keepdim=True)
    return torch.bmm(p.to(q_i.dtype), _expand(v_i, group, interleave)).float() / denom


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
            o = _attend(self, query[b].unsqueeze(1), _pages(key_cache, block_table[b], kv_len),
                        _pages(value_cache, block_table[b], kv_len), kv_len, scale)
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
            o = _attend(self, query[lo:hi].permute(1, 0, 2), _pages(key_cache, block_table[b], kv_len),
                        _pages(value_cache, block_table[b], kv_len), kv_len, scale)
            out[lo:hi] = o.permute(1, 0, 2).to(out.dtype)
        return out
