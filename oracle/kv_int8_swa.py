"""Torch goldens of sliding-window attention over the int8 paged KV cache (`MojoPagedDecodeSWAWithKVDequant`,
`MojoPagedPrefillSWAWithKVDequant`).

Importing this module registers ``TorchPagedDecodeSWAWithKVDequant`` / ``TorchPagedPrefillSWAWithKVDequant`` as the
``torch`` backends of the two API classes.

Semantics and rounding points restate `mojo_opset/experimental/operators/attention.py:850-980` (prefill) and :1032-1148
(decode).  They differ from the GQA-dequant golden (`oracle/kv_int8.py`: softmax, then the probabilities rounded to
the query dtype): here the scores are fp32 and masked with -inf by `paged.window_mask`,
``p = exp(s - max)`` stays fp32 into the value product, and the result is divided by the fp32 row sum, then cast.  With
``compute_dtype=bfloat16`` keys and values are dequantised in fp32 (``K8 * key_scale``); with ``compute_dtype=int8`` the
scaled query and the unnormalised probabilities are quantised per row (`row_quantize`) and both products are
integer-valued fp32 matmuls.  With ``is_causal=False`` no mask is applied at all.  Pages are gathered by plain indexing of
the table.  `tests/golden/paged_kv_int8_swa_*.pt` pin these classes bit for bit.
"""
import math
from typing import Optional

import torch

from mojo_opset_amd.core.operators import attention as _attn

from .kv_int8 import check_query, row_quantize
from .paged import expand_kv_heads, index_pages, window_mask

_CPU = ["rocm", "cpu"]


def _attend(op, q, k8, v8, key_scale, value_scale, softmax_scale, kv_len):
    """q [Hq, Lq, D], k8 / v8 [Hq, kv_len, D] int8 (already expanded), scales [Hq, D] -> [Hq, Lq, D] fp32."""
    k_t = k8.permute(0, 2, 1)
    if op.compute_dtype == torch.int8:
        q_quant, q_scale = row_quantize(q * key_scale.unsqueeze(1), op.qmax, op.qmin)
        s = torch.bmm(q_quant.float(), k_t.float()) * q_scale * softmax_scale
    else:
        s = torch.bmm(q.float(), (k_t.float() * key_scale.unsqueeze(-1).float()).float()) * softmax_scale
    if op.is_causal:
        mask = window_mask(q.shape[1], kv_len, op.local_window_size, op.global_window_size).to(s.device)
        s = torch.where(mask, s, float("-inf"))
    s = s - torch.max(s, dim=-1, keepdim=True).values
    p = torch.exp(s)
    denom = torch.sum(p, dim=-1, keepdim=True)
    if op.compute_dtype == torch.int8:
        p_quant, p_scale = row_quantize(p, op.qmax, op.qmin)
        o = torch.bmm(p_quant.float(), v8.float()) * p_scale * value_scale.unsqueeze(1)
    else:
        o = torch.bmm(p.float(), (v8.float() * value_scale.unsqueeze(1).float()).float())
    return o / denom


class TorchPagedDecodeSWAWithKVDequant(_attn.MojoPagedDecodeSWAWithKVDequant):
    """Reference :1032-1148: one query per sequence at position ``kv_len - 1``; rows with ``kv_len == 0`` are zeros."""

    supported_platforms_list = _CPU

    def forward(self, query, query_scale, key_cache, key_scale, value_cache, value_scale, total_seq_lens, block_table,
                softmax_scale: Optional[float] = None, *, max_total_seq_len: Optional[int] = None):
        _attn.assert_paged_decode_contract(block_table, total_seq_lens)
        check_query(self, query, query_scale)
        batch, hq, dim = query.shape
        group, layout = hq // key_cache.shape[1], self.gqa_layout
        scale = 1.0 / math.sqrt(dim) if softmax_scale is None else softmax_scale
        ks, vs = expand_kv_heads(key_scale, group, layout), expand_kv_heads(value_scale, group, layout)
        out = torch.zeros_like(query)
        for b, kv_len in enumerate(total_seq_lens.tolist()):
            if kv_len == 0:
                continue
            k8 = expand_kv_heads(index_pages(key_cache, block_table[b], kv_len), group, layout)
            v8 = expand_kv_heads(index_pages(value_cache, block_table[b], kv_len), group, layout)
            out[b] = _attend(self, query[b].unsqueeze(1), k8, v8, ks, vs, scale, kv_len).squeeze(1).to(out.dtype)
        return out


class TorchPagedPrefillSWAWithKVDequant(_attn.MojoPagedPrefillSWAWithKVDequant):
    """Reference :850-980: packed queries, row i of a sequence at position ``kv_len - q_len + i``.  Rows of sequences
    without queries are zeros (the reference leaves them uninitialised)."""

    supported_platforms_list = _CPU

    def forward(self, query, query_scale, key_cache, key_scale, value_cache, value_scale, cu_q_lens, block_table,
                softmax_scale: Optional[float] = None, cu_total_seq_lens: Optional[torch.Tensor] = None,
                max_q_len: Optional[int] = None, max_total_seq_len: Optional[int] = None):
        _attn.assert_paged_prefill_contract(cu_q_lens, block_table, cu_total_seq_lens)
        check_query(self, query, query_scale)
        tokens, hq, dim = query.shape
        group, layout = hq // key_cache.shape[1], self.gqa_layout
        scale = 1.0 / math.sqrt(dim) if softmax_scale is None else softmax_scale
        ks, vs = expand_kv_heads(key_scale, group, layout), expand_kv_heads(value_scale, group, layout)
        cu_q = cu_q_lens.tolist()
        cu_kv = cu_q if cu_total_seq_lens is None else cu_total_seq_lens.tolist()
        out = torch.zeros_like(query)
        for b in range(len(cu_q) - 1):
            lo, hi = cu_q[b], cu_q[b + 1]
            if hi == lo:
                continue
            kv_len = cu_kv[b + 1] - cu_kv[b]
            k8 = expand_kv_heads(index_pages(key_cache, block_table[b], kv_len), group, layout)
            v8 = expand_kv_heads(index_pages(value_cache, block_table[b], kv_len), group, layout)
            o = _attend(self, query[lo:hi].permute(1, 0, 2), k8, v8, ks, vs, scale, kv_len)
            out[lo:hi] = o.permute(1, 0, 2).to(out.dtype)
        return out
