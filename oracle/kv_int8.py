"""Torch goldens of the int8 paged KV cache ops (`MojoStorePagedKVCacheC8`, `MojoPagedDecodeGQAWithKVDequant`,
`MojoPagedPrefillGQAWithKVDequant`).

Importing this module registers ``TorchStorePagedKVCacheC8`` / ``TorchPagedDecodeGQAWithKVDequant`` /
``TorchPagedPrefillGQAWithKVDequant`` as the ``torch`` backends of the three API classes.

Semantics and rounding points restate `mojo_opset/experimental/operators/kv_cache.py:109-184` (store: the quotient
``state / scale`` under torch's type promotion, ``round``, clamp to [-128, 127], int8; plan rows written page by page)
and `mojo_opset/experimental/operators/attention.py:461-632` (prefill), :635-800 (decode).  With
``compute_dtype=bfloat16`` keys and values are dequantised in fp32 (``K8 * key_scale``), scores are an fp32 matmul times
the softmax scale, the softmax runs in fp32 and its probabilities are rounded to the query dtype before the fp32 product
with the values.  With ``compute_dtype=int8`` the scaled query and the probabilities are quantised per row (amax / 127,
clamped to 1e-5) and both products are integer-valued fp32 matmuls.  Pages are gathered by plain indexing of the table
(`paged.index_pages`).  `tests/golden/paged_kv_int8_*.pt` pin these classes bit for bit.
"""
import math
from typing import Optional

import torch

from mojo_opset_amd.core.operators import attention as _attn
from mojo_opset_amd.core.operators import kv_cache as _kv

from .paged import expand_kv_heads, index_pages

_CPU = ["rocm", "cpu"]


def quantize_kv_cache(cache: torch.Tensor):
    """The recipe of the reference's tests for a float cache ``[N, Hkv, page, D]``: per (head, channel) ``amax / 127``
    clamped to 1e-5, the cache divided by the fp32 scale, the scale stored as bf16 -> (int8 cache, scale [Hkv, D])."""
    cache_f = cache.float()
    scale = (cache_f.abs().amax(dim=(0, 2)) / 127).clamp(min=1e-5)
    quant = torch.round(cache_f / scale.unsqueeze(0).unsqueeze(2)).clamp(-128, 127).to(torch.int8)
    return quant, scale.to(torch.bfloat16)


def row_quantize(x: torch.Tensor, qmax: int, qmin: int):
    """Dynamic per-row symmetric quantisation (reference :450-459), in the dtype of ``x`` (bf16 for a bf16 query times a
    bf16 scale and for the probabilities): scale = amax / qmax with amax clamped to 1e-12, a scale below 1e-6 becomes 1."""
    scale = x.abs().amax(dim=-1, keepdim=True).clamp(min=1e-12) / qmax
    scale = torch.where(scale < 1e-6, 1.0, scale)
    q = (x / scale).round().clamp(qmin, qmax).to(torch.int8)
    return q, scale.view(*x.shape[:-1], 1)


def _attend(op, q, k8, v8, key_scale, value_scale, softmax_scale, mask_rows):
    """q [Hq, Lq, D], k8 / v8 [Hq, Lk, D] int8 (already expanded), scales [Hq, D] -> [Hq, Lq, D] fp32."""
    if op.compute_dtype == torch.int8:
        q_quant, q_scale = row_quantize(q * key_scale.unsqueeze(1), op.qmax, op.qmin)
        scores = torch.matmul(q_quant.float(), k8.mT.float()) * q_scale * softmax_scale
    else:
        scores = torch.matmul(q.float(), (k8.float() * key_scale.unsqueeze(1).float()).mT) * softmax_scale
    if mask_rows is not None:
        scores = torch.where(mask_rows, scores, float("-inf"))
    probs = torch.softmax(scores, dim=-1, dtype=torch.float32).to(q.dtype)
    if op.compute_dtype == torch.int8:
        p_quant, p_scale = row_quantize(probs, op.qmax, op.qmin)
        return torch.matmul(p_quant.float(), v8.float()) * p_scale * value_scale.unsqueeze(1)
    return torch.matmul(probs.float(), v8.float() * value_scale.unsqueeze(1).float())


def check_query(op, query, query_scale):
    if op.query_dtype == torch.int8:
        assert query_scale is not None and query.dtype == op.query_dtype, "query_scale must be provided for quantized query"
    else:
        assert query_scale is None and query.dtype == op.query_dtype, "query_scale must be None for non-quantized query"


class TorchStorePagedKVCacheC8(_kv.MojoStorePagedKVCacheC8):
    supported_platforms_list = _CPU

    def forward(self, key_states, value_states, key_cache, value_cache, key_scale, value_scale,
                block_table: Optional[torch.Tensor] = None, cu_q_lens: Optional[torch.Tensor] = None,
                context_kv_lens: Optional[torch.Tensor] = None, *, chunk_metadata: Optional[torch.Tensor] = None):
        self.check_call_contract(key_states, value_states, block_table, cu_q_lens, context_kv_lens, chunk_metadata)
        if chunk_metadata is None:
            chunk_metadata = _kv.build_paged_kv_chunk_metadata(block_table, cu_q_lens, context_kv_lens, key_cache.shape[2])
        assert key_scale is not None and value_scale is not None
        _kv.assert_paged_kv_store_contract(chunk_metadata)
        if chunk_metadata.shape[0] == 0:
            return key_cache, value_cache
        k8 = torch.round(key_states / key_scale).clamp(-128, 127).to(torch.int8)
        v8 = torch.round(value_states / value_scale).clamp(-128, 127).to(torch.int8)
        for src, blk, off, n in chunk_metadata.tolist():
            key_cache[blk, :, off:off + n, :] = k8[src:src + n].permute(1, 0, 2)
            value_cache[blk, :, off:off + n, :] = v8[src:src + n].permute(1, 0, 2)
        return key_cache, value_cache


class TorchPagedDecodeGQAWithKVDequant(_attn.MojoPagedDecodeGQAWithKVDequant):
    supported_platforms_list = _CPU

    def forward(self, query, query_scale, key_cache, key_scale, value_cache, value_scale, total_seq_lens, block_tables,
                softmax_scale: Optional[float] = None, mask: Optional[torch.Tensor] = None, *,
                max_total_seq_len: Optional[int] = None):
        _attn.assert_paged_decode_contract(block_tables, total_seq_lens)
        check_query(self, query, query_scale)
        batch, hq, dim = query.shape
        hkv = key_cache.shape[1]
        group, layout = hq // hkv, self.gqa_layout
        scale = 1.0 / math.sqrt(dim) if softmax_scale is None else softmax_scale
        ks, vs = expand_kv_heads(key_scale, group, layout), expand_kv_heads(value_scale, group, layout)
        out = torch.zeros(batch, hq, dim, dtype=query.dtype, device=query.device)
        for b, kv_len in enumerate(total_seq_lens.tolist()):
            if kv_len == 0:
                continue
            k8 = expand_kv_heads(index_pages(key_cache, block_tables[b], kv_len), group, layout)
            v8 = expand_kv_heads(index_pages(value_cache, block_tables[b], kv_len), group, layout)
            rows = None
            if not self.is_causal and mask is not None:
                rows = (mask if mask.dim() == 2 else mask[b])[kv_len, :kv_len]
            out[b] = _attend(self, query[b].unsqueeze(1), k8, v8, ks, vs, scale, rows).squeeze(1)
        return out


class TorchPagedPrefillGQAWithKVDequant(_attn.MojoPagedPrefillGQAWithKVDequant):
    supported_platforms_list = _CPU

    def forward(self, query, query_scale, key_cache, key_scale, value_cache, value_scale, cu_q_lens, block_tables,
                softmax_scale: Optional[float] = None, cu_total_seq_lens: Optional[torch.Tensor] = None,
                mask: Optional[torch.Tensor] = None, max_q_len: Optional[int] = None,
                max_total_seq_len: Optional[int] = None):
        _attn.assert_paged_prefill_contract(cu_q_lens, block_tables, cu_total_seq_lens)
        check_query(self, query, query_scale)
        tokens, hq, dim = query.shape
        hkv = key_cache.shape[1]
        group, layout = hq // hkv, self.gqa_layout
        scale = 1.0 / math.sqrt(dim) if softmax_scale is None else softmax_scale
        ks, vs = expand_kv_heads(key_scale, group, layout), expand_kv_heads(value_scale, group, layout)
        cu_q = cu_q_lens.tolist()
        cu_kv = cu_q if cu_total_seq_lens is None else cu_total_seq_lens.tolist()
        out = torch.zeros(tokens, hq, dim, dtype=query.dtype, device=query.device)
        for b in range(len(cu_q) - 1):
            lo, hi = cu_q[b], cu_q[b + 1]
            q_len, kv_len = hi - lo, cu_kv[b + 1] - cu_kv[b]
            k8 = expand_kv_heads(index_pages(key_cache, block_tables[b], kv_len), group, layout)
            v8 = expand_kv_heads(index_pages(value_cache, block_tables[b], kv_len), group, layout)
            rows = None
            if self.is_causal:
                rows = torch.ones(q_len, kv_len, dtype=torch.bool, device=query.device).tril(kv_len - q_len)
            elif mask is not None:
                rows = (mask if mask.dim() == 2 else mask[b])[kv_len - q_len:kv_len, :kv_len]
            out[lo:hi] = _attend(self, query[lo:hi].permute(1, 0, 2), k8, v8, ks, vs, scale, rows).permute(1, 0, 2)
        return out
