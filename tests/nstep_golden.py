"""Torch golden of the n-step paged decode (`MojoPagedDecodeNstepSWA`, `NSTEP_OPS`).

Importing this module registers ``TorchPagedDecodeNstepSWA`` as the ``torch`` backend of the API class.

Semantics and rounding points restate `mojo_opset/experimental/operators/attention.py:1185-1259` with the window mask of
`mojo_opset/core/operators/attention.py:507-531`: per sequence, the ``S`` query rows against its first ``kv_len`` keys (pages
gathered by plain indexing of the table), scores a 16-bit ``bmm`` upcast to fp32 and scaled, -inf outside the visible set,
softmax statistics in fp32, the unnormalised probabilities rounded to the storage type, a 16-bit ``bmm`` against V, upcast
and divided by the fp32 row sum.  Rows with ``kv_len <= 0`` are zeros.  `tests/golden/paged_nstep_swa.pt` pins this class
bit for bit (tests/make_nstep_golden.py records it from the reference).
"""
import math
from typing import Optional

import torch

from mojo_opset_amd.core.operators import attention as _attn
from oracle.paged import expand_kv_heads, index_pages, window_mask


class TorchPagedDecodeNstepSWA(_attn.MojoPagedDecodeNstepSWA):
    supported_platforms_list = ["rocm", "cpu"]

    def forward(self, query, key_cache, value_cache, total_seq_lens, block_table, softmax_scale: Optional[float] = None,
                *, max_total_seq_len: Optional[int] = None):
        _attn.assert_paged_decode_contract(block_table, total_seq_lens)
        _attn.assert_nstep_query(query)
        steps, hq, dim = query.shape[1:]
        group = hq // key_cache.shape[1]
        scale = 1.0 / math.sqrt(dim) if softmax_scale is None else softmax_scale
        out = torch.zeros_like(query)
        for b, kv_len in enumerate(total_seq_lens.tolist()):
            if kv_len <= 0:
                continue
            if int(block_table[b, 0]) < 0:
                raise ValueError("Paged decode requires a valid block table for rows with kv lens > 0.")
            q_b = query[b].permute(1, 0, 2)                                           # [Hq, S, D]
            k_t = index_pages(key_cache, block_table[b], kv_len).permute(0, 2, 1)     # [Hkv, D, kv_len]
            s = torch.bmm(q_b, expand_kv_heads(k_t, group, self.gqa_layout)).float() * scale
            if self.is_causal:
                mask = window_mask(steps, kv_len, self.local_window_size, self.global_window_size)
                s = torch.where(mask.to(s.device), s, float("-inf"))
            s = s - torch.max(s, dim=-1, keepdim=True).values
            p = torch.exp(s)
            denom = torch.sum(p, dim=-1, keepdim=True)
            v_b = expand_kv_heads(index_pages(value_cache, block_table[b], kv_len), group, self.gqa_layout)
            o = torch.bmm(p.to(query.dtype), v_b).float() / denom
            out[b] = o.permute(1, 0, 2).to(out.dtype)
        return out
