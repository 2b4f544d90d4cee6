"""Torch golden of the n-step paged decode over the int8 KV cache (`MojoPagedDecodeNstepSWAWithKVDequant`,
`NSTEP_KV_INT8_OPS`).

Importing this module registers ``TorchPagedDecodeNstepSWAWithKVDequant`` as the ``torch`` backend of the API class.

The reference has no class of this name.  The arithmetic is that of its `MojoPagedPrefillSWAWithKVDequant`
(`oracle/kv_int8_swa.py`, ``_attend`` with ``compute_dtype=bfloat16``) applied to the ``S`` query rows of each sequence, with
the shapes and the ``total_seq_lens`` convention of `MojoPagedDecodeNstepSWA` (`tests/nstep_golden.py`): per sequence, the
``S`` rows against its first ``kv_len`` keys (pages gathered by plain indexing of the table), keys and values dequantised in
fp32 (``K8 * key_scale``), fp32 scores masked with -inf outside the visible set, ``p = exp(s - max)`` kept fp32 into the value
product, the result divided by the fp32 row sum, then cast.  Rows with ``kv_len <= 0`` are zeros.
`tests/test_nstep_kv_int8_golden.py` pins this class bit for bit to the prefill golden.
"""
import math
from typing import Optional

import torch

from mojo_opset_amd.core.operators import attention as _attn
from oracle.paged import expand_kv_heads, index_pages, window_mask


class TorchPagedDecodeNstepSWAWithKVDequant(_attn.MojoPagedDecodeNstepSWAWithKVDequant):
    supported_platforms_list = ["rocm", "cpu"]

    def forward(self, query, query_scale, key_cache, key_scale, value_cache, value_scale, total_seq_lens, block_table,
                softmax_scale: Optional[float] = None, *, max_total_seq_len: Optional[int] = None):
        _attn.assert_paged_decode_contract(block_table, total_seq_lens)
        _attn.assert_nstep_query(query)
        assert query_scale is None and query.dtype == self.query_dtype, "query_scale must be None for non-quantized query"
        if self.compute_dtype == torch.int8:
            raise NotImplementedError("compute_dtype=torch.int8 (quantised query and probabilities) has no n-step golden")
        steps, hq, dim = query.shape[1:]
        group, layout = hq // key_cache.shape[1], self.gqa_layout
        scale = 1.0 / math.sqrt(dim) if softmax_scale is None else softmax_scale
        ks, vs = expand_kv_heads(key_scale, group, layout), expand_kv_heads(value_scale, group, layout)
        out = torch.zeros_like(query)
        for b, kv_len in enumerate(total_seq_lens.tolist()):
            if kv_len <= 0:
                continue
            q_b = query[b].permute(1, 0, 2)                                           # [Hq, S, D]
            k8 = expand_kv_heads(index_pages(key_cache, block_table[b], kv_len), group, layout)
            v8 = expand_kv_heads(index_pages(value_cache, block_table[b], kv_len), group, layout)
            k_t = k8.permute(0, 2, 1)                                                 # [Hq, D, kv_len]
            s = torch.bmm(q_b.float(), (k_t.float() * ks.unsqueeze(-1).float()).float()) * scale
            if self.is_causal:
                mask = window_mask(steps, kv_len, self.local_window_size, self.global_window_size).to(s.device)
                s = torch.where(mask, s, float("-inf"))
            s = s - torch.max(s, dim=-1, keepdim=True).values
            p = torch.exp(s)
            denom = torch.sum(p, dim=-1, keepdim=True)
            o = torch.bmm(p.float(), (v8.float() * vs.unsqueeze(1).float()).float()) / denom
            out[b] = o.permute(1, 0, 2).to(out.dtype)
        return out
