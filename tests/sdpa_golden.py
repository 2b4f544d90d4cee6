"""Torch golden of the bidirectional attention with an optional mask (`MojoSdpa`, `FULL_ATTN_OPS`).

Importing this module registers ``TorchSdpa`` as the ``torch`` backend of the API class.

The reference's class (`mojo_opset/core/operators/attention.py:456-504`) is torch's fused scaled-dot-product attention with no
dropout and no causal edge, so the golden is the same library call on the same arguments: that is the only way to the same
bits (the library's CPU kernel blocks and rounds in its own order).  `tests/golden/sdpa.pt` pins this class bit for bit
(tests/make_sdpa_golden.py records it from the reference).

A row whose mask hides every key is NaN or unspecified in the library; the hip backend defines it as zeros (beyond the
reference), so no recorded case has such a row.
"""
from typing import Optional

import torch
import torch.nn.functional as F

from mojo_opset_amd.core.operators import attention as _attn


class TorchSdpa(_attn.MojoSdpa):
    supported_platforms_list = ["rocm", "cpu"]

    def forward(self, query, key, value, attn_mask: Optional[torch.Tensor] = None):
        return F.scaled_dot_product_attention(query, key, value, attn_mask=attn_mask, scale=self.scale,
                                              enable_gqa=self.enable_gqa)


def reference_fp32(query, key, value, attn_mask=None, scale=None, enable_gqa=False):
    """The same attention in fp32, step by step (what the tolerance of the GPU tests is about): scores scaled, bias added or
    hidden keys set to -inf, softmax, rows with no visible key as zeros."""
    q, k, v = query.float(), key.float(), value.float()
    if enable_gqa and q.shape[-3] != k.shape[-3]:
        g = q.shape[-3] // k.shape[-3]
        k, v = k.repeat_interleave(g, dim=-3), v.repeat_interleave(g, dim=-3)
    s = (q @ k.transpose(-1, -2)) * (q.shape[-1] ** -0.5 if scale is None else scale)
    if attn_mask is not None:
        s = s.masked_fill(~attn_mask, float("-inf")) if attn_mask.dtype == torch.bool else s + attn_mask.float()
    dead = torch.isneginf(s).all(dim=-1, keepdim=True)
    p = torch.softmax(s.masked_fill(dead, 0.0), dim=-1).masked_fill(dead, 0.0)
    return p @ v
