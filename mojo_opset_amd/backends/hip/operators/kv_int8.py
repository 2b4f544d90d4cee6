"""HIP<Op> classes of the int8 paged KV cache with per-channel scales: the quantising store, the decode / prefill
GQA that read it, their sliding-window forms and the n-step decode.  Everything that is not built raises ``NotImplementedError`` on the host, before any
device work."""
from typing import Optional

import torch

from ....core.operators.attention import (MojoPagedDecodeGQAWithKVDequant, MojoPagedDecodeNstepSWAWithKVDequant,
                                          MojoPagedDecodeSWAWithKVDequant, MojoPagedPrefillGQAWithKVDequant,
                                          MojoPagedPrefillSWAWithKVDequant, assert_nstep_query,
                                          assert_paged_decode_contract, assert_paged_prefill_contract)
from ....core.operators.kv_cache import MojoStorePagedKVCacheC8, assert_paged_kv_layout_contract
from .. import lib as L
from .attention import _nstep_composed, _paged_decode, _paged_prefill, _swa_windows, _validate_tables

__all__ = ["HIPStorePagedKVCacheC8", "HIPPagedDecodeGQAWithKVDequant", "HIPPagedPrefillGQAWithKVDequant",
           "HIPPagedDecodeSWAWithKVDequant", "HIPPagedPrefillSWAWithKVDequant", "HIPPagedDecodeNstepSWAWithKVDequant"]

_ROCM = ["rocm"]
_SCALE_DTYPES = (torch.bfloat16, torch.float16, torch.float32)
_DECODE_DIMS = (64, 80, 96, 128)
_PREFILL_DIMS = (64, 96, 128)
_DECODE_KV8 = ("mojo_hip_paged_decode_gqa_kv8_workspace_bytes", "mojo_hip_paged_decode_gqa_kv8")
_PREFILL_KV8 = ("mojo_hip_paged_prefill_gqa_kv8_workspace_bytes", "mojo_hip_paged_prefill_gqa_kv8")
_DECODE_SWA_KV8 = ("mojo_hip_paged_decode_swa_kv8_workspace_bytes", "mojo_hip_paged_decode_swa_kv8")
_PREFILL_SWA_KV8 = ("mojo_hip_paged_prefill_swa_kv8_workspace_bytes", "mojo_hip_paged_prefill_swa_kv8")
_DECODE_NSTEP_KV8 = ("mojo_hip_paged_decode_nstep_kv8_workspace_bytes", "mojo_hip_paged_decode_nstep_kv8")


def _dense(t):
    return t if t.is_contiguous() else t.contiguous()


def _refuse_unbuilt(op, what, query, query_scale, mask):
    """The host-side refusals shared by decode and prefill (no tensor is touched)."""
    if op.compute_dtype == torch.int8:
        raise NotImplementedError(f"{what}: compute_dtype=torch.int8 (quantised query and probabilities) is not built")
    if not op.is_causal or mask is not None:
        raise NotImplementedError(f"{what} supports causal attention without an explicit mask only")
    if query_scale is not None or query.dtype == torch.int8:
        raise NotImplementedError(f"{what}: quantised queries (query_scale) are not built")
    if query.dtype not in (torch.bfloat16, torch.float16):
        raise NotImplementedError(f"{what}: query dtype {query.dtype} (bf16 / fp16 only)")


def _check_int8_caches(what, key_cache, value_cache, key_scale, value_scale, hkv, dim):
    assert key_cache.dtype == torch.int8 and value_cache.dtype == torch.int8, f"{what}: the caches must be int8"
    assert value_cache.shape == key_cache.shape
    assert tuple(key_scale.shape) == (hkv, dim) and tuple(value_scale.shape) == (hkv, dim), \
        f"{what}: key_scale / value_scale must be [kv_heads, head_dim]"
    if key_cache.stride() != value_cache.stride() or key_cache.stride(-1) != 1:
        raise NotImplementedError(f"{what}: key/value caches must share strides and be dense in head_dim")
    if key_scale.dtype != value_scale.dtype or key_scale.dtype not in _SCALE_DTYPES:
        raise NotImplementedError(f"{what}: key_scale and value_scale must share one of the dtypes bf16 / fp16 / fp32")


class HIPStorePagedKVCacheC8(MojoStorePagedKVCacheC8):
    supported_platforms_list = _ROCM

    def forward(self, key_states, value_states, key_cache, value_cache, key_scale, value_scale,
                block_table: Optional[torch.Tensor] = None, cu_q_lens: Optional[torch.Tensor] = None,
                context_kv_lens: Optional[torch.Tensor] = None, *, chunk_metadata: Optional[torch.Tensor] = None):
        self.check_call_contract(key_states, value_states, block_table, cu_q_lens, context_kv_lens, chunk_metadata)
        assert key_scale is not None and value_scale is not None
        assert key_cache.dim() == 4
        n_blocks, heads, page, dim = key_cache.shape
        tokens = key_states.shape[0]
        assert key_states.shape[1:] == (heads, dim), "key/value states do not match the cache's (heads, head_dim)"
        assert key_states.dtype == value_states.dtype
        _check_int8_caches("HIPStorePagedKVCacheC8", key_cache, value_cache, key_scale, value_scale, heads, dim)
        if key_states.dtype not in (torch.bfloat16, torch.float16):
            raise NotImplementedError(f"HIPStorePagedKVCacheC8: state dtype {key_states.dtype} (bf16 / fp16 only)")
        if dim % 8 != 0:
            raise NotImplementedError(f"HIPStorePagedKVCacheC8: head_dim {dim} must be a multiple of 8")
        L.require_cuda(key_states, value_states, key_cache, value_cache, key_scale, value_scale, block_table, cu_q_lens,
                       context_kv_lens, chunk_metadata)
        if key_states.stride(-1) != 1 or key_states.stride() != value_states.stride():
            key_states, value_states = key_states.contiguous(), value_states.contiguous()
        key_scale, value_scale = _dense(key_scale), _dense(value_scale)
        common = (tokens, heads, dim, n_blocks, page, L.dtype_code(key_states.dtype), L.dtype_code(key_scale.dtype),
                  key_states.stride(0), key_states.stride(1), key_cache.stride(0), key_cache.stride(1),
                  key_cache.stride(2), L.stream_of(key_cache))
        lib = L.load()
        if chunk_metadata is not None:
            plan = _dense(chunk_metadata)
            L.check(lib.mojo_hip_store_paged_kv_c8_plan(
                L.ptr(key_states), L.ptr(value_states), L.ptr(key_cache), L.ptr(value_cache), L.ptr(key_scale),
                L.ptr(value_scale), L.ptr(plan), plan.shape[0], *common), "HIPStorePagedKVCacheC8")
        else:
            assert_paged_kv_layout_contract(block_table, cu_q_lens, context_kv_lens)
            batch = context_kv_lens.shape[0]
            if cu_q_lens is not None:
                assert cu_q_lens.shape[0] == batch + 1
            table = block_table if block_table.stride(1) == 1 else block_table.contiguous()
            L.check(lib.mojo_hip_store_paged_kv_c8_layout(
                L.ptr(key_states), L.ptr(value_states), L.ptr(key_cache), L.ptr(value_cache), L.ptr(key_scale),
                L.ptr(value_scale), L.ptr(table), table.stride(0), table.shape[1],
                L.ptr(None if cu_q_lens is None else _dense(cu_q_lens)), L.ptr(_dense(context_kv_lens)), batch, *common),
                "HIPStorePagedKVCacheC8")
        return key_cache, value_cache


class HIPPagedDecodeGQAWithKVDequant(MojoPagedDecodeGQAWithKVDequant):
    """Paged decode over the int8 cache: the scales are folded into the query (``q * key_scale``) and into the epilogue
    (``value_scale``), both contractions run on the matrix cores in fp16."""
    supported_platforms_list = _ROCM

    def forward(self, query, query_scale, key_cache, key_scale, value_cache, value_scale, total_seq_lens, block_tables,
                softmax_scale: Optional[float] = None, mask: Optional[torch.Tensor] = None, *,
                max_total_seq_len: Optional[int] = None, leave_empty_rows: Optional[bool] = None):
        what = "HIPPagedDecodeGQAWithKVDequant"
        assert_paged_decode_contract(block_tables, total_seq_lens)
        _refuse_unbuilt(self, what, query, query_scale, mask)
        batch, hq, dim = query.shape
        n_blocks, hkv, page, dim_c = key_cache.shape
        assert dim_c == dim and hq % hkv == 0
        _check_int8_caches(what, key_cache, value_cache, key_scale, value_scale, hkv, dim)
        if dim not in _DECODE_DIMS or page % 16 != 0 or not 1 <= hq // hkv <= 16:
            raise NotImplementedError(f"{what}: head_dim {dim} / page {page} / group {hq // hkv} outside the envelope "
                                      f"(head_dim {_DECODE_DIMS}, pages of a multiple of 16 tokens, groups of 1..16)")
        if any(s % 16 for s in key_cache.stride()[:3]):
            raise NotImplementedError(f"{what}: cache strides must be multiples of 16 bytes")
        L.require_cuda(query, key_cache, value_cache, key_scale, value_scale, total_seq_lens, block_tables)
        return _paged_decode(self, what, _DECODE_KV8, query, key_cache, value_cache, total_seq_lens, block_tables,
                             softmax_scale, max_total_seq_len, leave_empty_rows, scales=(_dense(key_scale), _dense(value_scale)))


class HIPPagedPrefillGQAWithKVDequant(MojoPagedPrefillGQAWithKVDequant):
    """Paged prefill over the int8 cache, the simple route: one dequantising gather of the pages in use into 16-bit
    scratch pages, then `HIPPagedPrefillGQA`'s kernels on the scratch.  The scratch is sized without a
    host sync as ``batch * ceil(min(max_total_seq_len, page * table width) / page)`` pages of K and of V: a caller who
    omits ``max_total_seq_len`` on a wide table pays for the table's capacity.  ``max_total_seq_len``, when given, MUST be an
    upper bound of every sequence's kv length: unlike the 16-bit op, where the hint only steers planning, here it sizes the
    scratch, and keys past it are not gathered (they read as zero keys).  ``MOJO_HIP_VALIDATE=1`` checks it (one sync)."""
    supported_platforms_list = _ROCM

    def forward(self, query, query_scale, key_cache, key_scale, value_cache, value_scale, cu_q_lens, block_tables,
                softmax_scale: Optional[float] = None, cu_total_seq_lens: Optional[torch.Tensor] = None,
                mask: Optional[torch.Tensor] = None, max_q_len: Optional[int] = None,
                max_total_seq_len: Optional[int] = None):
        what = "HIPPagedPrefillGQAWithKVDequant"
        assert_paged_prefill_contract(cu_q_lens, block_tables, cu_total_seq_lens)
        _refuse_unbuilt(self, what, query, query_scale, mask)
        tokens, hq, dim = query.shape
        n_blocks, hkv, page, dim_c = key_cache.shape
        assert dim_c == dim and hq % hkv == 0
        _check_int8_caches(what, key_cache, value_cache, key_scale, value_scale, hkv, dim)
        if dim not in _PREFILL_DIMS or page % 4 != 0 or hq // hkv not in (1, 2, 4, 8):
            raise NotImplementedError(f"{what}: head_dim {dim} / page {page} / group {hq // hkv} outside the envelope "
                                      f"(head_dim {_PREFILL_DIMS}, pages of a multiple of 4 tokens, groups of 1, 2, 4, 8)")
        if any(s % 16 for s in key_cache.stride()[:3]):
            raise NotImplementedError(f"{what}: cache strides must be multiples of 16 bytes")
        L.require_cuda(query, key_cache, value_cache, key_scale, value_scale, cu_q_lens, block_tables, cu_total_seq_lens)
        return _paged_prefill(self, what, _PREFILL_KV8, query, key_cache, value_cache, cu_q_lens, block_tables, softmax_scale,
                              cu_total_seq_lens, max_q_len, max_total_seq_len, scales=(_dense(key_scale), _dense(value_scale)))


class HIPPagedDecodeSWAWithKVDequant(MojoPagedDecodeSWAWithKVDequant):
    """Sliding-window paged decode over the int8 cache: `HIPPagedDecodeGQAWithKVDequant`'s kernel walking only the
    16-token tiles of the global and local ranges.  Pages outside a row's visible set are never read: their
    table entries may be -1 or any valid id.  With no window its entry point runs the unwindowed op, bit for bit."""
    supported_platforms_list = _ROCM

    def forward(self, query, query_scale, key_cache, key_scale, value_cache, value_scale, total_seq_lens, block_table,
                softmax_scale: Optional[float] = None, *, max_total_seq_len: Optional[int] = None,
                leave_empty_rows: Optional[bool] = None):
        what = "HIPPagedDecodeSWAWithKVDequant"
        assert_paged_decode_contract(block_table, total_seq_lens)
        _refuse_unbuilt(self, what, query, query_scale, None)
        windows = _swa_windows(self, what)
        batch, hq, dim = query.shape
        n_blocks, hkv, page, dim_c = key_cache.shape
        assert dim_c == dim and hq % hkv == 0
        _check_int8_caches(what, key_cache, value_cache, key_scale, value_scale, hkv, dim)
        if dim not in _DECODE_DIMS or page % 16 != 0 or not 1 <= hq // hkv <= 16:
            raise NotImplementedError(f"{what}: head_dim {dim} / page {page} / group {hq // hkv} outside the envelope "
                                      f"(head_dim {_DECODE_DIMS}, pages of a multiple of 16 tokens, groups of 1..16)")
        if any(s % 16 for s in key_cache.stride()[:3]):
            raise NotImplementedError(f"{what}: cache strides must be multiples of 16 bytes")
        L.require_cuda(query, key_cache, value_cache, key_scale, value_scale, total_seq_lens, block_table)
        return _paged_decode(self, what, _DECODE_SWA_KV8, query, key_cache, value_cache, total_seq_lens, block_table,
                             softmax_scale, max_total_seq_len, leave_empty_rows,
                             scales=(_dense(key_scale), _dense(value_scale)), windows=windows)


class HIPPagedDecodeNstepSWAWithKVDequant(MojoPagedDecodeNstepSWAWithKVDequant):
    """``S`` query tokens per sequence in one pass over the int8 cache: `HIPPagedDecodeSWAWithKVDequant`'s
    kernel with (step, head) pairs in the 16 columns of its score product, so the K/V bytes are read once per block of
    ``16 // G`` steps.  ``S = 1`` is `HIPPagedDecodeSWAWithKVDequant`, bit for bit.

    Where the workspace query answers -1 — ``MOJO_HIP_DECODE_MFMA=0`` — the COMPOSED route runs: ``S`` single-step
    launches, step ``j`` on ``query[:, j]`` with the lengths ``len - (S - 1 - j)`` (computed on the device: no sync,
    capture-safe).  It is correct and costs ``S`` times the bytes.

    A row with ``0 < len < S`` stores zeros for the steps that see no key, and raises ``ValueError`` under
    ``MOJO_HIP_VALIDATE=1``; with no window negative page ids are holes as in the single-step op."""
    supported_platforms_list = _ROCM

    def forward(self, query, query_scale, key_cache, key_scale, value_cache, value_scale, total_seq_lens, block_table,
                softmax_scale: Optional[float] = None, *, max_total_seq_len: Optional[int] = None,
                leave_empty_rows: Optional[bool] = None):
        what = "HIPPagedDecodeNstepSWAWithKVDequant"
        assert_paged_decode_contract(block_table, total_seq_lens)
        assert_nstep_query(query)
        _refuse_unbuilt(self, what, query, query_scale, None)
        windows = _swa_windows(self, what)
        batch, steps, hq, dim = query.shape
        n_blocks, hkv, page, dim_c = key_cache.shape
        assert dim_c == dim and hq % hkv == 0
        _check_int8_caches(what, key_cache, value_cache, key_scale, value_scale, hkv, dim)
        if dim not in _DECODE_DIMS or page % 16 != 0 or not 1 <= hq // hkv <= 16:
            raise NotImplementedError(f"{what}: head_dim {dim} / page {page} / group {hq // hkv} outside the envelope "
                                      f"(head_dim {_DECODE_DIMS}, pages of a multiple of 16 tokens, groups of 1..16)")
        if any(s % 16 for s in key_cache.stride()[:3]):
            raise NotImplementedError(f"{what}: cache strides must be multiples of 16 bytes")
        L.require_cuda(query, key_cache, value_cache, key_scale, value_scale, total_seq_lens, block_table)
        if steps == 0:
            return torch.empty_like(query)
        if _validate_tables() and batch > 0 and bool(((total_seq_lens > 0) & (total_seq_lens < steps)).any()):
            raise ValueError(f"{what}: a row holds fewer keys than the {steps} query steps it counts")
        scales = (_dense(key_scale), _dense(value_scale))
        hint = int(max_total_seq_len) if max_total_seq_len is not None else 0
        fused = L.load().mojo_hip_paged_decode_nstep_kv8_workspace_bytes(
            batch, hq, hkv, dim, page, block_table.shape[1], hint, *windows, steps) >= 0
        if fused:
            return _paged_decode(self, what, _DECODE_NSTEP_KV8, query, key_cache, value_cache, total_seq_lens, block_table,
                                 softmax_scale, max_total_seq_len, leave_empty_rows, scales=scales, windows=(*windows, steps))
        return _nstep_composed(self, what, _DECODE_SWA_KV8, query, key_cache, value_cache, total_seq_lens, block_table,
                               softmax_scale, max_total_seq_len, leave_empty_rows, windows, scales=scales)


class HIPPagedPrefillSWAWithKVDequant(MojoPagedPrefillSWAWithKVDequant):
    """Sliding-window paged prefill over the int8 cache: the dequantising gather of the pages that intersect a sequence's
    visible union — ``[0, global)`` and ``[kv_len - q_len - local, kv_len)`` — into a compact 16-bit scratch, then
    `HIPPagedPrefillSWA`'s kernels on it.  The scratch holds ``ceil(global / page) + ceil((max_q_len +
    local + 1) / page) + 2`` pages per sequence whatever the context (``max_q_len`` omitted: the token count);
    ``max_q_len`` and ``max_total_seq_len``, when given, MUST be upper bounds (`HIPPagedPrefillGQAWithKVDequant`).  With a
    window the pages must be a multiple of 16 tokens.  With no window its entry point runs the unwindowed op."""
    supported_platforms_list = _ROCM

    def forward(self, query, query_scale, key_cache, key_scale, value_cache, value_scale, cu_q_lens, block_table,
                softmax_scale: Optional[float] = None, cu_total_seq_lens: Optional[torch.Tensor] = None,
                max_q_len: Optional[int] = None, max_total_seq_len: Optional[int] = None):
        what = "HIPPagedPrefillSWAWithKVDequant"
        assert_paged_prefill_contract(cu_q_lens, block_table, cu_total_seq_lens)
        _refuse_unbuilt(self, what, query, query_scale, None)
        windows = _swa_windows(self, what)
        tokens, hq, dim = query.shape
        n_blocks, hkv, page, dim_c = key_cache.shape
        assert dim_c == dim and hq % hkv == 0
        _check_int8_caches(what, key_cache, value_cache, key_scale, value_scale, hkv, dim)
        windowed = windows[0] >= 0 or windows[1] > 0
        if dim not in _PREFILL_DIMS or page % (16 if windowed else 4) != 0 or hq // hkv not in (1, 2, 4, 8):
            raise NotImplementedError(f"{what}: head_dim {dim} / page {page} / group {hq // hkv} outside the envelope "
                                      f"(head_dim {_PREFILL_DIMS}, pages of a multiple of 16 tokens — 4 without a window —, "
                                      f"groups of 1, 2, 4, 8)")
        if any(s % 16 for s in key_cache.stride()[:3]):
            raise NotImplementedError(f"{what}: cache strides must be multiples of 16 bytes")
        L.require_cuda(query, key_cache, value_cache, key_scale, value_scale, cu_q_lens, block_table, cu_total_seq_lens)
        return _paged_prefill(self, what, _PREFILL_SWA_KV8, query, key_cache, value_cache, cu_q_lens, block_table,
                              softmax_scale, cu_total_seq_lens, max_q_len, max_total_seq_len,
                              scales=(_dense(key_scale), _dense(value_scale)), windows=windows)
