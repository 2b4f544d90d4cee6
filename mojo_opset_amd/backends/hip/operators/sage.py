"""HIP<Op> class of the int8-compute paged prefill (`SAGE_ATTN_OPS`): `MojoPagedPrefillSageGQA` on the int8 matrix cores
(csrc/sage_prefill.hip).  One launch of `mojo_hip_paged_prefill_sage_gqa`: no dequantising gather, no 16-bit
scratch, no workspace.  Everything outside the envelope raises ``NotImplementedError`` on the host, before any device work."""
import math
from typing import Optional

import torch

from ....core.operators.attention import MojoPagedPrefillSageGQA, assert_paged_prefill_contract
from .. import lib as L
from .attention import _validate_tables

__all__ = ["HIPPagedPrefillSageGQA"]

_DIMS, _GROUPS, _MAX_PAGE = (64, 128), (1, 2, 4, 8), 256
MAX_KV_LEN = 132104            # 127 * 128 * kv_len < 2^31: the int32 P.V accumulator bounds the row length


class HIPPagedPrefillSageGQA(MojoPagedPrefillSageGQA):
    """Causal paged prefill with both contractions on ``v_mfma_i32_16x16x64_i8`` and int32 accumulators.  Two passes over the
    keys (row maxima, then probabilities quantised against the final maximum), so the integers are the golden's.

    Envelope: ``head_dim`` 64 / 128, pages of a multiple of 16 tokens up to 256, ``Hq / Hkv`` 1 / 2 / 4 / 8, both GQA layouts,
    int32 tables, caches dense in ``head_dim`` with shared strides that are multiples of 16 bytes, fp32 scales, at most
    132 104 keys a sequence — ``min(max_total_seq_len, page * table width)`` is what is checked, so a wide table needs the hint.
    ``mask`` and ``is_causal=False`` are not built.  ``max_q_len`` / ``max_total_seq_len`` are upper-bound hints: a length above
    its hint is cut to it.  Every key from the first negative or out-of-pool page id on is a zero K / V row (score 0, counted in
    the row sum), as in `HIPPagedPrefillGQA`.  Rows of a sequence without keys, rows that see no key (``kv_len < q_len``:
    `HIPPagedPrefillGQA` leaves them without a defined value) and rows at or past ``cu_q_lens[-1]`` are zeros.
    ``MOJO_HIP_VALIDATE=1`` (a host sync) raises ``ValueError`` for a negative first page id of a sequence with keys and for a
    length above its hint.  No host sync otherwise, capture-safe, and two calls give the same bits."""
    supported_platforms_list = ["rocm"]

    def forward(self, query, query_scale, key_cache, key_scale, value_cache, value_scale, cu_q_lens, block_tables,
                softmax_scale: Optional[float] = None, cu_total_seq_lens: Optional[torch.Tensor] = None,
                mask: Optional[torch.Tensor] = None, max_q_len: Optional[int] = None,
                max_total_seq_len: Optional[int] = None):
        what = "HIPPagedPrefillSageGQA"
        assert_paged_prefill_contract(cu_q_lens, block_tables, cu_total_seq_lens)
        if not self.is_causal or mask is not None:
            raise NotImplementedError(f"{what} supports causal attention without an explicit mask only")
        if query.dtype != torch.int8 or key_cache.dtype != torch.int8 or value_cache.dtype != torch.int8:
            raise NotImplementedError(f"{what}: query and caches must be int8, got {query.dtype} / {key_cache.dtype} / "
                                      f"{value_cache.dtype} (16-bit queries: MojoPagedPrefillGQAWithKVDequant)")
        tokens, hq, dim = query.shape
        n_blocks, hkv, page, dim_c = key_cache.shape
        assert dim_c == dim and hq % hkv == 0 and value_cache.shape == key_cache.shape
        assert query_scale is not None and tuple(query_scale.shape) == (hq, tokens), f"{what}: query_scale must be [Hq, T]"
        assert tuple(key_scale.shape) == (n_blocks, hkv, page), f"{what}: key_scale must be [N, Hkv, page]"
        assert tuple(value_scale.shape) == (hkv, dim), f"{what}: value_scale must be [Hkv, head_dim]"
        if dim not in _DIMS or page % 16 != 0 or page > _MAX_PAGE or hq // hkv not in _GROUPS:
            raise NotImplementedError(f"{what}: head_dim {dim} / page {page} / group {hq // hkv} outside the envelope "
                                      f"(head_dim {_DIMS}, pages of a multiple of 16 tokens up to {_MAX_PAGE}, groups {_GROUPS})")
        if any(t.dtype != torch.float32 for t in (query_scale, key_scale, value_scale)):
            raise NotImplementedError(f"{what}: query_scale, key_scale and value_scale must be float32")
        if key_cache.stride() != value_cache.stride() or key_cache.stride(-1) != 1 or any(s % 16 for s in key_cache.stride()[:3]):
            raise NotImplementedError(f"{what}: key/value caches must share strides that are multiples of 16 bytes and be dense "
                                      f"in head_dim")
        hint_q = int(max_q_len) if max_q_len else 0
        hint_kv = int(max_total_seq_len) if max_total_seq_len else 0
        capacity = page * block_tables.shape[1]
        if (min(hint_kv, capacity) if hint_kv else capacity) > MAX_KV_LEN:
            raise NotImplementedError(f"{what}: up to {MAX_KV_LEN} keys a sequence (int32 accumulators); the table holds "
                                      f"{capacity} and max_total_seq_len is {max_total_seq_len}")
        L.require_cuda(query, query_scale, key_cache, key_scale, value_cache, value_scale, cu_q_lens, block_tables,
                       cu_total_seq_lens)
        batch = cu_q_lens.shape[0] - 1
        if _validate_tables() and batch > 0 and block_tables.shape[1] > 0:
            q_lens = cu_q_lens[1:] - cu_q_lens[:-1]
            kv_lens = q_lens if cu_total_seq_lens is None else cu_total_seq_lens[1:] - cu_total_seq_lens[:-1]
            if bool(((q_lens > 0) & (kv_lens > 0) & (block_tables[:, 0] < 0)).any()):
                raise ValueError("Paged prefill requires a valid block table for rows with kv lens > 0.")
            if (hint_kv and int(kv_lens.max()) > hint_kv) or (hint_q and int(q_lens.max()) > hint_q):
                raise ValueError(f"{what}: a sequence's length exceeds its max_q_len / max_total_seq_len hint")
        q = query if query.is_contiguous() else query.contiguous()
        out = torch.empty(q.shape, dtype=torch.bfloat16, device=q.device)
        if tokens == 0 or batch == 0:
            return out.zero_() if batch == 0 else out
        dense = [t if t.is_contiguous() else t.contiguous() for t in (query_scale, key_scale, value_scale, cu_q_lens)]
        tables = block_tables if block_tables.stride(1) == 1 else block_tables.contiguous()
        cu_kv = None if cu_total_seq_lens is None else cu_total_seq_lens.contiguous()
        scale = 1.0 / math.sqrt(dim) if softmax_scale is None else float(softmax_scale)
        L.check(L.load().mojo_hip_paged_prefill_sage_gqa(
            L.ptr(q), L.ptr(dense[0]), L.ptr(key_cache), L.ptr(dense[1]), L.ptr(value_cache), L.ptr(dense[2]), L.ptr(dense[3]),
            L.ptr(cu_kv), L.ptr(tables), L.ptr(out), tokens, batch, hq, hkv, dim, n_blocks, page, tables.shape[1],
            tables.stride(0), key_cache.stride(0), key_cache.stride(1), key_cache.stride(2), hint_q, hint_kv, scale,
            1 if self.gqa_layout == "ABAB" else 0, L.stream_of(q)), what)
        return out
