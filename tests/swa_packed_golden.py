"""Torch golden of the packed var-len attention over contiguous K/V (`MojoSWA`, `PACKED_ATTN_OPS`).

Importing this module registers ``TorchSWA`` as the ``torch`` backend of the API class.

Semantics and rounding points restate `mojo_opset/core/operators/attention.py:774-835` with the window mask of :507-531: per
sequence, the query rows ``[cu_q_lens[b], cu_q_lens[b+1])`` against the K/V rows ``[cu_total_seq_lens[b],
cu_total_seq_lens[b+1])`` — `oracle.swa._attend`, the arithmetic of the paged prefill golden, on plain slices.  Defined beyond
the reference: rows of a sequence with ``kv_len <= 0`` are zeros, and so are rows at or past ``cu_q_lens[-1]`` (the reference
raises an ``IndexError`` on an empty key set and leaves the output uninitialised).  `tests/golden/swa_packed.pt` pins this
class bit for bit (tests/make_swa_packed_golden.py records it from the reference).
"""
import math
from typing import Optional

import torch

from mojo_opset_amd.core.operators import attention as _attn
from oracle.swa import _attend


class TorchSWA(_attn.MojoSWA):
    supported_platforms_list = ["rocm", "cpu"]

    def forward(self, query, key, value, cu_q_lens, cu_total_seq_lens, softmax_scale: Optional[float] = None, *,
                max_q_len: Optional[int] = None, max_total_seq_len: Optional[int] = None):
        _attn.assert_swa_packed_contract(query, key, value, cu_q_lens, cu_total_seq_lens)
        scale = 1.0 / math.sqrt(query.shape[2]) if softmax_scale is None else softmax_scale
        cu_q, cu_kv = cu_q_lens.tolist(), cu_total_seq_lens.tolist()
        out = torch.zeros_like(query)
        for b in range(len(cu_q) - 1):
            lo, hi = cu_q[b], cu_q[b + 1]
            k_lo, kv_len = cu_kv[b], cu_kv[b + 1] - cu_kv[b]
            if hi <= lo or kv_len <= 0:
                continue
            o = _attend(self, query[lo:hi].permute(1, 0, 2), key[k_lo:k_lo + kv_len].permute(1, 0, 2),
                        value[k_lo:k_lo + kv_len].permute(1, 0, 2), kv_len, scale)
            out[lo:hi] = o.permute(1, 0, 2).to(out.dtype)
        return out
