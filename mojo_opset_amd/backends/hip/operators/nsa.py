"""HIP<Op> classes of the native-sparse-attention decode pair (`NSA_ATTN_OPS`): `MojoDecodeNSA` and `MojoPagedDecodeNSA` on
csrc/nsa_decode.hip, and of its prefill pair (`NSA_PREFILL_OPS`): `MojoPrefillNSA` and `MojoPagedPrefillNSA` on
csrc/nsa_prefill.hip.  Each pair ends in one entry point: the contiguous op is its computed-row-address
instance, the paged op the table lookup.  Everything outside the envelope raises ``NotImplementedError`` on the host, before
any device work."""
import math
from typing import Optional

import torch

from ....core.operators.attention import (MojoDecodeNSA, MojoPagedDecodeNSA, MojoPagedPrefillNSA, MojoPrefillNSA,
                                          assert_paged_decode_contract, assert_paged_prefill_contract)
from .. import lib as L
from .attention import _validate_tables

__all__ = ["HIPDecodeNSA", "HIPPagedDecodeNSA", "HIPPrefillNSA", "HIPPagedPrefillNSA"]

_DIMS, _MAX_PAGE, _MAX_SELECTED, _MAX_BLOCKS = (64, 128), 256, 64, 8192
_ENVELOPE = """Envelope: bf16 / fp16, ``head_dim`` 64 / 128, ``block_size % compress_ratio == 0``, ``num_selected_blocks <= 64``, at most
    8192 selection blocks in a row's capacity, K/V dense in ``head_dim`` with shared strides that are multiples of 16 bytes,
    ``gate_proj`` on the device in the query's dtype or fp32.  Scores, probabilities and the weighted sum stay in fp32 and
    the output is rounded once, where the golden rounds at every step; where two block scores are closer than the golden's
    rounding noise the two may select different blocks.  Among equal block scores the LOWER block index is taken (the
    reference's ``torch.topk`` leaves ties unspecified).  ``num_splits``: ``None`` = the launch form is planned from the
    shapes, ``1`` = the fused form (one launch, the score row in LDS; refused when the row does not fit), ``> 1`` = the
    split form with that many key slices; `mojo_hip_last_launch()` names the form taken.  No host sync, capture-safe, and two
    calls of one form give the same bits."""


def _nsa_envelope(op, what, query, key, value, tables, page, max_pages, strides, max_blocks=_MAX_BLOCKS):
    """What decode and prefill refuse alike, on the host and before any device work; answers (cr, bs, nsel)."""
    heads, dim = query.shape[1:]
    if query.dtype not in (torch.bfloat16, torch.float16) or key.dtype != query.dtype or value.dtype != query.dtype:
        raise NotImplementedError(f"{what}: query, key and value must share bf16 or fp16, got {query.dtype} / {key.dtype} / "
                                  f"{value.dtype}")
    cr, bs, nsel = int(op.compress_ratio), int(op.block_size), int(op.num_selected_blocks)
    if dim not in _DIMS or cr <= 0 or bs <= 0 or bs % cr != 0 or not 0 <= nsel <= _MAX_SELECTED or int(op.window_size) < 0:
        raise NotImplementedError(f"{what}: head_dim {dim} / compress_ratio {cr} / block_size {bs} / num_selected_blocks {nsel} "
                                  f"outside the envelope (head_dim {_DIMS}, block_size a multiple of compress_ratio, at most "
                                  f"{_MAX_SELECTED} selected blocks)")
    if tables is not None and (page % 16 != 0 or page > _MAX_PAGE):
        raise NotImplementedError(f"{what}: page {page} (pages of a multiple of 16 tokens up to {_MAX_PAGE})")
    if -(-page * max_pages // bs) > max_blocks:
        raise NotImplementedError(f"{what}: {page * max_pages} keys of capacity are more than {max_blocks} selection blocks")
    if key.stride() != value.stride() or key.stride(-1) != 1 or any(s % 8 for s in strides):
        raise NotImplementedError(f"{what}: key / value must share strides that are multiples of 16 bytes and be dense in head_dim")
    gate = op.gate_proj
    if gate.dtype not in (query.dtype, torch.float32) or tuple(gate.shape) != (heads, dim, 3) or heads != op.num_heads:
        raise NotImplementedError(f"{what}: gate_proj must be [{heads}, {dim}, 3] in {query.dtype} or float32, got "
                                  f"{tuple(gate.shape)} {gate.dtype}")
    return cr, bs, nsel


def _nsa_launch(op, what, query, key, value, lens, tables, page, max_pages, n_blocks, strides, softmax_scale, num_splits):
    """The shared host path: envelope, workspace, launch.  ``strides``: (block or batch, head, token) of K/V in elements."""
    batch, heads, dim = query.shape
    cr, bs, nsel = _nsa_envelope(op, what, query, key, value, tables, page, max_pages, strides)
    gate = op.gate_proj
    if num_splits is not None and int(num_splits) < 1:
        raise ValueError(f"{what}: num_splits must be None or >= 1, got {num_splits}")
    L.require_cuda(query, key, value, lens, tables, gate)
    q = query if query.is_contiguous() else query.contiguous()
    out = torch.empty_like(q)
    if batch == 0 or page * max_pages == 0:
        return out.zero_()
    gate = gate.detach()
    gate = gate if gate.is_contiguous() else gate.contiguous()
    splits = 0 if num_splits is None else int(num_splits)
    lib = L.load()
    ws_bytes = lib.mojo_hip_nsa_decode_workspace_bytes(batch, heads, dim, page * max_pages, cr, bs, splits)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=q.device)
    scale = 1.0 / math.sqrt(dim) if softmax_scale is None else float(softmax_scale)
    L.check(lib.mojo_hip_nsa_decode(
        L.ptr(q), L.ptr(key), L.ptr(value), L.ptr(gate), L.ptr(lens), L.ptr(tables), L.ptr(out), L.ptr(ws), ws.numel(), batch,
        heads, dim, n_blocks, page, max_pages, 0 if tables is None else tables.stride(0), *strides, cr, bs, nsel,
        int(op.window_size), scale, L.dtype_code(q.dtype), L.dtype_code(gate.dtype), splits, L.stream_of(q)), what)
    return out


class HIPDecodeNSA(MojoDecodeNSA):
    __doc__ = f"""Native sparse attention decode over contiguous K/V ``[B, S, H, D]``: one walk over K for every score the three
    branches need, one weight per key, one walk over V.

    {_ENVELOPE}"""
    supported_platforms_list = ["rocm"]

    def forward(self, query, key, value, total_seq_lens: Optional[torch.Tensor] = None, softmax_scale: Optional[float] = None,
                *, num_splits: Optional[int] = None):
        what = "HIPDecodeNSA"
        assert key.shape == value.shape and key.shape[0] == query.shape[0] and key.shape[2:] == query.shape[1:]
        if total_seq_lens is not None and total_seq_lens.dtype != torch.int32:
            raise NotImplementedError(f"{what}: total_seq_lens must be int32, got {total_seq_lens.dtype}")
        lens = None if total_seq_lens is None else total_seq_lens.contiguous()
        return _nsa_launch(self, what, query, key, value, lens, None, key.shape[1], 1, 0,
                           (key.stride(0), key.stride(2), key.stride(1)), softmax_scale, num_splits)


class HIPPagedDecodeNSA(MojoPagedDecodeNSA):
    __doc__ = f"""Native sparse attention decode over a paged cache ``[N, H, page, D]``, pages of a multiple of 16 tokens up to 256,
    int32 lengths and tables; the page and the selection block are independent.  Every key from the first negative or
    out-of-pool page id on is a zero K / V row (score 0, counted by the three softmaxes), as in `HIPPagedDecodeGQA`; a length
    above ``page * table width`` is cut to it.  ``MOJO_HIP_VALIDATE=1`` (a host sync) raises ``ValueError`` for a negative
    first page id of a sequence with keys.

    {_ENVELOPE}"""
    supported_platforms_list = ["rocm"]

    def forward(self, query, key_cache, value_cache, total_seq_lens, block_tables, softmax_scale: Optional[float] = None,
                *, num_splits: Optional[int] = None):
        what = "HIPPagedDecodeNSA"
        if any(isinstance(t, torch.Tensor) and t.dtype != torch.int32 for t in (total_seq_lens, block_tables)):
            raise NotImplementedError(f"{what}: total_seq_lens and block_tables must be int32")
        assert_paged_decode_contract(block_tables, total_seq_lens)
        n_blocks, heads, page, dim = key_cache.shape
        assert value_cache.shape == key_cache.shape and (heads, dim) == tuple(query.shape[1:])
        tables = block_tables if block_tables.stride(1) == 1 else block_tables.contiguous()
        if (_validate_tables() and query.is_cuda and query.shape[0] > 0 and tables.shape[1] > 0 and
                bool(((total_seq_lens > 0) & (tables[:, 0] < 0)).any())):
            raise ValueError("Paged decode requires a valid block table for rows with kv lens > 0.")
        return _nsa_launch(self, what, query, key_cache, value_cache, total_seq_lens.contiguous(), tables, page, tables.shape[1],
                           n_blocks, (key_cache.stride(0), key_cache.stride(1), key_cache.stride(2)), softmax_scale, num_splits)


_PREFILL_MAX_BLOCKS = 959
_PREFILL_ENVELOPE = f"""Envelope: bf16 / fp16, ``head_dim`` 64 / 128, ``block_size % compress_ratio == 0`` with ``compress_ratio`` a divisor of
    16 (a group of keys never leaves a 16-key piece of a tile), ``num_selected_blocks <= 64``, at most {_PREFILL_MAX_BLOCKS}
    selection blocks in a sequence's capacity (two fp32 statistics per (row, block) live in LDS; the capacity is ``page *
    table width``, or ``T`` for contiguous K/V), K/V dense in ``head_dim`` with shared strides that are multiples of 16 bytes,
    ``gate_proj`` on the device in the query's dtype or fp32, int32 ``cu_*`` and tables.  Scores, statistics and the weighted
    sum stay in fp32; the weight of a (row, key) is rounded ONCE to the storage type in front of the second matrix product
    (the residual of that rounding takes a second product on steps with a weight of 2^-4 or more) and the output once.  Among equal block scores the LOWER block index is taken.  A row with ``0 < t_kv < compress_ratio`` is not
    compressed (groups of one key), unlike decode.  No host sync, capture-safe, two calls give the same bits;
    `mojo_hip_last_launch()` answers ``nsa_prefill:w<waves>:d<dim>``."""


def _nsa_prefill_launch(op, what, query, key, value, cu_q, cu_kv, tables, page, max_pages, n_blocks, strides, softmax_scale):
    """The prefill pair's host path: the decode pair's envelope, then its own plan and launch."""
    total, heads, dim = query.shape
    cr, bs, nsel = _nsa_envelope(op, what, query, key, value, tables, page, max_pages, strides, _PREFILL_MAX_BLOCKS)
    if 16 % cr != 0:
        raise NotImplementedError(f"{what}: compress_ratio {cr} must divide 16")
    if any(t is not None and t.dtype != torch.int32 for t in (cu_q, cu_kv, tables)):
        raise NotImplementedError(f"{what}: cu_q_lens, cu_total_seq_lens and block_tables must be int32")
    gate = op.gate_proj
    L.require_cuda(query, key, value, cu_q, cu_kv, tables, gate)
    q = query if query.is_contiguous() else query.contiguous()
    out = torch.zeros_like(q)                          # (rows behind the last sequence read as zeros)
    batch = cu_q.shape[0] - 1
    if total == 0 or batch <= 0 or page * max_pages == 0:
        return out
    gate = gate.detach()
    gate = gate if gate.is_contiguous() else gate.contiguous()
    lib = L.load()
    if lib.mojo_hip_nsa_prefill_workspace_bytes(total, batch, heads, dim, page * max_pages, cr, bs) < 0:
        raise NotImplementedError(f"{what}: the launch plan refuses these shapes")
    scale = 1.0 / math.sqrt(dim) if softmax_scale is None else float(softmax_scale)
    L.check(lib.mojo_hip_nsa_prefill(
        L.ptr(q), L.ptr(key), L.ptr(value), L.ptr(gate), L.ptr(cu_q), L.ptr(cu_kv), L.ptr(tables), L.ptr(out), None, 0, total,
        batch, heads, dim, n_blocks, page, max_pages, 0 if tables is None else tables.stride(0), *strides, cr, bs, nsel,
        int(op.window_size), int(bool(op.is_causal)), scale, L.dtype_code(q.dtype), L.dtype_code(gate.dtype), L.stream_of(q)), what)
    return out


class HIPPrefillNSA(MojoPrefillNSA):
    __doc__ = f"""Native sparse attention prefill over contiguous K/V ``[T, H, D]``: scores on the matrix cores, one weight per
    (row, key), the weighted sum on the matrix cores (csrc/nsa_prefill.hip).

    {_PREFILL_ENVELOPE}"""
    supported_platforms_list = ["rocm"]

    def forward(self, query, key, value, cu_q_lens, softmax_scale: Optional[float] = None):
        assert key.shape == value.shape == query.shape and cu_q_lens.dim() == 1
        return _nsa_prefill_launch(self, "HIPPrefillNSA", query, key, value, cu_q_lens.contiguous(), None, None, key.shape[0], 1, 0,
                                   (0, key.stride(1), key.stride(0)), softmax_scale)


class HIPPagedPrefillNSA(MojoPagedPrefillNSA):
    __doc__ = f"""Native sparse attention prefill over a paged cache ``[N, H, page, D]``, pages of a multiple of 16 tokens up to
    256.  Every key from the first negative or out-of-pool page id on is a zero K / V row (score 0, counted by the three
    softmaxes); a length above ``page * table width`` is cut to it.  ``MOJO_HIP_VALIDATE=1`` (a host sync) raises
    ``ValueError`` for a negative first page id of a sequence with keys.

    {_PREFILL_ENVELOPE}"""
    supported_platforms_list = ["rocm"]

    def forward(self, query, key_cache, value_cache, cu_q_lens, block_tables, softmax_scale: Optional[float] = None,
                cu_total_seq_lens: Optional[torch.Tensor] = None):
        what = "HIPPagedPrefillNSA"
        if any(isinstance(t, torch.Tensor) and t.dtype != torch.int32 for t in (cu_q_lens, block_tables, cu_total_seq_lens)):
            raise NotImplementedError(f"{what}: cu_q_lens, cu_total_seq_lens and block_tables must be int32")
        assert_paged_prefill_contract(cu_q_lens, block_tables, cu_total_seq_lens)
        n_blocks, heads, page, dim = key_cache.shape
        assert value_cache.shape == key_cache.shape and (heads, dim) == tuple(query.shape[1:])
        tables = block_tables if block_tables.stride(1) == 1 else block_tables.contiguous()
        cu_kv = None if cu_total_seq_lens is None else cu_total_seq_lens.contiguous()
        if _validate_tables() and query.is_cuda and tables.shape[0] > 0 and tables.shape[1] > 0:
            kv_lens = (cu_q_lens if cu_kv is None else cu_kv).diff()
            if bool(((kv_lens > 0) & (cu_q_lens.diff() > 0) & (tables[:, 0] < 0)).any()):
                raise ValueError("Paged decode requires a valid block table for rows with kv lens > 0.")
        return _nsa_prefill_launch(self, what, query, key_cache, value_cache, cu_q_lens.contiguous(), cu_kv, tables, page,
                                   tables.shape[1], n_blocks, (key_cache.stride(0), key_cache.stride(1), key_cache.stride(2)),
                                   softmax_scale)
