"""API classes of the paged GQA attention pair and of its sliding-window pair.

Constructor arguments, contracts and `forward` signatures follow
`mojo_opset/core/operators/attention.py` (`MojoPagedDecodeGQA` :113-232,
`MojoPagedPrefillGQA` :315-451, contracts :12-37, `MojoPagedPrefillSWA` :533-650,
`MojoPagedDecodeSWA` :653-744, `MojoSWA` :747-838, `MojoSdpa` :456-504) and `mojo_opset/experimental/operators/attention.py` (`MojoPagedDecodeNstepSWA`
:1154-1262).  The classes are API-only; see `core/operator.py` for why the golden `forward` is not here.
"""
from typing import Optional

import torch

from ..operator import MojoOperator

_GQA_LAYOUTS = ("ABAB", "AABB")


def assert_paged_decode_contract(block_tables, total_seq_lens) -> None:
    """int32 `[B]` lengths and int32 `[B, max_blocks]` table (reference :31-37)."""
    assert isinstance(block_tables, torch.Tensor) and isinstance(total_seq_lens, torch.Tensor)
    assert total_seq_lens.dtype == torch.int32
    assert block_tables.dtype == torch.int32
    assert block_tables.dim() == 2
    assert block_tables.shape[0] == total_seq_lens.shape[0]


def assert_paged_prefill_contract(cu_q_lens, block_tables, cu_total_seq_lens) -> None:
    """int32 `[B+1]` cumulative lengths and int32 `[B, max_blocks]` table (reference :12-28)."""
    assert isinstance(cu_q_lens, torch.Tensor) and isinstance(block_tables, torch.Tensor)
    assert cu_q_lens.dtype == torch.int32
    assert block_tables.dtype == torch.int32
    assert block_tables.dim() == 2
    batch = cu_q_lens.shape[0] - 1
    if cu_total_seq_lens is not None:
        assert isinstance(cu_total_seq_lens, torch.Tensor)
        assert cu_total_seq_lens.dtype == torch.int32
        assert cu_total_seq_lens.dim() == 1
        assert cu_total_seq_lens.shape[0] == batch + 1
    assert block_tables.shape[0] == batch


class _PagedGQABase:
    def _init_gqa(self, is_causal: bool, gqa_layout: str) -> None:
        if gqa_layout not in _GQA_LAYOUTS:
            raise ValueError(f"gqa_layout must be one of ['ABAB', 'AABB'], got {gqa_layout}")
        self.is_causal = is_causal
        self.gqa_layout = gqa_layout

    def extra_repr(self) -> str:
        return f"is_causal={self.is_causal!r}, gqa_layout={self.gqa_layout!r}"


class MojoPagedDecodeGQA(_PagedGQABase, MojoOperator):
    """One query token per sequence against a paged KV cache.

    forward(query [B,Hq,D], key_cache/value_cache [N_blocks,Hkv,page,D], total_seq_lens [B] i32,
            block_tables [B,max_blocks] i32 (unused = -1), softmax_scale=None, mask=None, *,
            max_total_seq_len=None) -> [B,Hq,D]; rows with seq_len <= 0 are zeros.
    """

    def __init__(self, is_causal: bool = True, gqa_layout: str = "AABB"):
        super().__init__()
        self._init_gqa(is_causal, gqa_layout)


class MojoPagedPrefillGQA(_PagedGQABase, MojoOperator):
    """Packed var-len queries against a paged KV cache, causal offset ``kv_len - q_len``.

    forward(query [T,Hq,D], key_cache, value_cache, cu_q_lens [B+1] i32, block_tables [B,nb] i32,
            softmax_scale=None, cu_total_seq_lens=None, mask=None, max_q_len=None,
            max_total_seq_len=None) -> [T,Hq,D]
    """

    def __init__(self, is_causal: bool = True, gqa_layout: str = "AABB"):
        super().__init__()
        self._init_gqa(is_causal, gqa_layout)


class _PagedSWABase:
    """Constructor of the sliding-window pair (reference :533-560, :653-680): the attributes ``is_causal``,
    ``gqa_layout``, ``gqa_interleave``, ``global_window_size`` and ``local_window_size`` are all a backend may read
    (the plugin keeps the reference's constructor and grafts only ``forward``)."""

    def _init_swa(self, is_causal: bool, gqa_layout: str, global_window_size: Optional[int],
                  local_window_size: Optional[int]) -> None:
        if gqa_layout not in _GQA_LAYOUTS:
            raise ValueError(f"gqa_layout must be one of ['ABAB', 'AABB'], got {gqa_layout}")
        self.is_causal = is_causal
        self.gqa_layout = gqa_layout
        self.gqa_interleave = gqa_layout == "ABAB"
        self.global_window_size = global_window_size
        self.local_window_size = local_window_size

    def extra_repr(self) -> str:
        return (f"is_causal={self.is_causal}, gqa_layout={self.gqa_layout}, "
                f"global_window_size={self.global_window_size}, local_window_size={self.local_window_size}")


class MojoPagedDecodeSWA(_PagedSWABase, MojoOperator):
    """One query token per sequence against a paged KV cache, sliding window.

    The query sits at position ``p = kv_len - 1`` and sees key ``j`` iff ``j <= p`` and, when a window is set,
    ``j >= p - local_window_size`` (local window: ``local + 1`` keys) or ``j < global_window_size``.

    forward(query [B,Hq,D], key_cache/value_cache [N_blocks,Hkv,page,D], total_seq_lens [B] i32,
            block_table [B,max_blocks] i32, softmax_scale=None, *, max_total_seq_len=None) -> [B,Hq,D];
    rows with seq_len <= 0 are zeros.
    """

    def __init__(self, is_causal: bool = True, gqa_layout: str = "AABB", global_window_size: Optional[int] = None,
                 local_window_size: Optional[int] = None):
        super().__init__()
        self._init_swa(is_causal, gqa_layout, global_window_size, local_window_size)


def assert_nstep_query(query) -> None:
    """The n-step op's query is 4-D (reference experimental :1199-1201)."""
    assert query.ndim == 4, (
        f"MojoPagedDecodeNstepSWA expects 4D query [bsz, seq_len, n_q_heads, head_dim], got ndim={query.ndim}")


class MojoPagedDecodeNstepSWA(_PagedSWABase, MojoOperator):
    """``S`` query tokens per sequence (draft verification, multi-token prediction) against a paged KV cache, causal,
    with the optional windows of `MojoPagedDecodeSWA`; with no window it is the n-step form of `MojoPagedDecodeGQA`.

    ``total_seq_lens`` counts the ``S`` new tokens: step ``j`` of a row of ``kv_len`` keys sits at position
    ``p = kv_len - S + j`` and sees key ``t`` iff ``t <= p`` and, when a window is set, ``t >= p - local_window_size`` or
    ``t < global_window_size``.

    forward(query [B,S,Hq,D], key_cache/value_cache [N_blocks,Hkv,page,D], total_seq_lens [B] i32,
            block_table [B,max_blocks] i32, softmax_scale=None, *, max_total_seq_len=None) -> [B,S,Hq,D];
    rows with seq_len <= 0 are zeros.
    """

    def __init__(self, is_causal: bool = True, gqa_layout: str = "AABB", global_window_size: Optional[int] = None,
                 local_window_size: Optional[int] = None):
        super().__init__()
        self._init_swa(is_causal, gqa_layout, global_window_size, local_window_size)


class MojoPagedPrefillSWA(_PagedSWABase, MojoOperator):
    """Packed var-len queries against a paged KV cache, causal offset ``kv_len - q_len``, sliding window (the
    visibility rule of `MojoPagedDecodeSWA` for every query row).

    forward(query [T,Hq,D], key_cache, value_cache, cu_q_lens [B+1] i32, block_table [B,nb] i32,
            softmax_scale=None, cu_total_seq_lens=None, *, max_q_len=None, max_total_seq_len=None) -> [T,Hq,D]
    """

    def __init__(self, is_causal: bool = True, gqa_layout: str = "AABB", global_window_size: Optional[int] = None,
                 local_window_size: Optional[int] = None):
        super().__init__()
        self._init_swa(is_causal, gqa_layout, global_window_size, local_window_size)


def assert_swa_packed_contract(query, key, value, cu_q_lens, cu_total_seq_lens) -> None:
    """int32 `[B+1]` cumulative lengths (reference :785-786) and packed 3-D query / key / value of one head_dim and dtype."""
    assert isinstance(cu_q_lens, torch.Tensor) and isinstance(cu_total_seq_lens, torch.Tensor)
    assert cu_q_lens.dtype == torch.int32
    assert cu_total_seq_lens.dtype == torch.int32
    assert cu_q_lens.dim() == 1 and cu_q_lens.shape[0] >= 1 and cu_total_seq_lens.shape == cu_q_lens.shape
    assert query.dim() == 3 and key.dim() == 3 and value.shape == key.shape
    assert key.shape[2] == query.shape[2] and key.shape[1] > 0 and query.shape[1] % key.shape[1] == 0
    assert query.dtype == key.dtype == value.dtype


class MojoSWA(_PagedSWABase, MojoOperator):
    """Packed var-len queries against CONTIGUOUS packed keys and values (no cache, no table): the attention of a first
    prefill.  Sequence ``b`` owns query rows ``[cu_q_lens[b], cu_q_lens[b+1])`` and K/V rows
    ``[cu_total_seq_lens[b], cu_total_seq_lens[b+1])``; causal offset ``kv_len - q_len`` and the visibility rule of
    `MojoPagedDecodeSWA` for every query row.  With no window it is plain var-len flash attention.

    forward(query [Tq,Hq,D], key [Tk,Hkv,D], value [Tk,Hkv,D], cu_q_lens [B+1] i32, cu_total_seq_lens [B+1] i32,
            softmax_scale=None) -> [Tq,Hq,D]
    """

    def __init__(self, is_causal: bool = True, gqa_layout: str = "AABB", global_window_size: Optional[int] = None,
                 local_window_size: Optional[int] = None):
        super().__init__()
        self._init_swa(is_causal, gqa_layout, global_window_size, local_window_size)


class MojoSdpa(MojoOperator):
    """Bidirectional scaled-dot-product attention with an optional mask: every query row sees every key (no causal edge).

    forward(query [B,Hq,Sq,D], key [B,Hkv,Sk,D], value [B,Hkv,Sk,D], attn_mask=None) -> [B,Hq,Sq,D]; 3-D tensors are one
    batch entry.  ``scale=None`` is ``1 / sqrt(D)``.  ``enable_gqa=True`` lets ``Hq`` be a multiple of ``Hkv``: query head
    ``h`` reads kv head ``h // (Hq // Hkv)`` (the grouping of ``repeat_interleave``).  ``attn_mask`` is broadcastable to
    ``[B,Hq,Sq,Sk]``: boolean (``False`` hides the key) or floating (added to the scaled score, ``-inf`` allowed).
    """

    def __init__(self, scale: Optional[float] = None, enable_gqa: bool = False):
        super().__init__()
        self.scale = scale
        self.enable_gqa = enable_gqa

    def extra_repr(self) -> str:
        return f"scale={self.scale!r}, enable_gqa={self.enable_gqa!r}"


class _PagedGQAKVDequantBase:
    """Constructor of the int8-cache pair (`mojo_opset/experimental/operators/attention.py:464-499`, :638-681): the
    attributes ``is_causal``, ``gqa_layout``, ``query_dtype``, ``context_dtype``, ``compute_dtype`` (and ``qmax`` /
    ``qmin`` with ``compute_dtype=torch.int8``) are all a backend may read."""

    def _init_kv_dequant(self, is_causal, gqa_layout, query_dtype, context_dtype, compute_dtype) -> None:
        if gqa_layout not in _GQA_LAYOUTS:
            raise ValueError(f"gqa_layout must be one of ['ABAB', 'AABB'], got {gqa_layout}")
        self.is_causal = is_causal
        self.gqa_layout = gqa_layout
        self.query_dtype = query_dtype
        self.context_dtype = context_dtype
        self.compute_dtype = compute_dtype
        assert self.query_dtype in (torch.bfloat16, torch.int8), f"Unsupported query dtype {self.query_dtype}"
        if self.query_dtype == torch.int8:
            raise NotImplementedError("Quantized query is not implemented")
        assert self.context_dtype == torch.int8, f"Quant attention support int8 context only, but got {self.context_dtype}"
        assert self.compute_dtype in (torch.bfloat16, torch.int8), f"Unsupported compute dtype {self.compute_dtype}"
        if self.compute_dtype == torch.int8:
            self.qmax = 127
            self.qmin = -128

    def extra_repr(self) -> str:
        return (f"is_causal={self.is_causal!r}, gqa_layout={self.gqa_layout!r}, query_dtype={self.query_dtype!r}, "
                f"context_dtype={self.context_dtype!r}, compute_dtype={self.compute_dtype!r}")


class MojoPagedDecodeGQAWithKVDequant(_PagedGQAKVDequantBase, MojoOperator):
    """`MojoPagedDecodeGQA` over an int8 K/V cache with per-channel scales.

    forward(query [B,Hq,D], query_scale (None: the query is not quantised), key_cache [N,Hkv,page,D] int8,
            key_scale [Hkv,D], value_cache int8, value_scale [Hkv,D], total_seq_lens [B] i32, block_tables [B,nb] i32,
            softmax_scale=None, mask=None, *, max_total_seq_len=None) -> [B,Hq,D]; rows of length 0 are zeros.
    A key is ``K8 * key_scale``, a value ``V8 * value_scale``.
    """

    def __init__(self, is_causal: bool = True, gqa_layout: str = "AABB", query_dtype: torch.dtype = torch.bfloat16,
                 context_dtype: torch.dtype = torch.int8, compute_dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        self._init_kv_dequant(is_causal, gqa_layout, query_dtype, context_dtype, compute_dtype)


class MojoPagedPrefillGQAWithKVDequant(_PagedGQAKVDequantBase, MojoOperator):
    """`MojoPagedPrefillGQA` over an int8 K/V cache with per-channel scales.

    forward(query [T,Hq,D], query_scale (None), key_cache int8, key_scale [Hkv,D], value_cache int8, value_scale [Hkv,D],
            cu_q_lens [B+1] i32, block_tables [B,nb] i32, softmax_scale=None, cu_total_seq_lens=None, mask=None,
            max_q_len=None, max_total_seq_len=None) -> [T,Hq,D]
    """

    def __init__(self, is_causal: bool = True, gqa_layout: str = "AABB", query_dtype: torch.dtype = torch.bfloat16,
                 context_dtype: torch.dtype = torch.int8, compute_dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        self._init_kv_dequant(is_causal, gqa_layout, query_dtype, context_dtype, compute_dtype)


class _PagedSWAKVDequantBase:
    """Constructor of the windowed int8-cache pair (`mojo_opset/experimental/operators/attention.py:806-848`, :988-1030):
    the attributes of `_PagedSWABase` and of `_PagedGQAKVDequantBase` together — ``is_causal``, ``gqa_layout``,
    ``gqa_interleave``, ``global_window_size``, ``local_window_size``, ``query_dtype``, ``context_dtype``,
    ``compute_dtype`` (and ``qmax`` / ``qmin`` with ``compute_dtype=torch.int8``)."""

    def _init_swa_kv_dequant(self, is_causal, gqa_layout, global_window_size, local_window_size, query_dtype,
                             context_dtype, compute_dtype) -> None:
        _PagedSWABase._init_swa(self, is_causal, gqa_layout, global_window_size, local_window_size)
        _PagedGQAKVDequantBase._init_kv_dequant(self, is_causal, gqa_layout, query_dtype, context_dtype, compute_dtype)

    def extra_repr(self) -> str:
        return (f"is_causal={self.is_causal!r}, gqa_layout={self.gqa_layout!r}, "
                f"global_window_size={self.global_window_size!r}, local_window_size={self.local_window_size!r}, "
                f"query_dtype={self.query_dtype!r}, context_dtype={self.context_dtype!r}, "
                f"compute_dtype={self.compute_dtype!r}")


class MojoPagedDecodeSWAWithKVDequant(_PagedSWAKVDequantBase, MojoOperator):
    """`MojoPagedDecodeSWA` over an int8 K/V cache with per-channel scales (the visibility rule of `MojoPagedDecodeSWA`,
    the cache of `MojoPagedDecodeGQAWithKVDequant`).

    forward(query [B,Hq,D], query_scale (None: the query is not quantised), key_cache [N,Hkv,page,D] int8,
            key_scale [Hkv,D], value_cache int8, value_scale [Hkv,D], total_seq_lens [B] i32, block_table [B,nb] i32,
            softmax_scale=None, *, max_total_seq_len=None) -> [B,Hq,D]; rows of length 0 are zeros.
    """

    def __init__(self, is_causal: bool = True, gqa_layout: str = "AABB", global_window_size: Optional[int] = None,
                 local_window_size: Optional[int] = None, query_dtype: torch.dtype = torch.bfloat16,
                 context_dtype: torch.dtype = torch.int8, compute_dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        self._init_swa_kv_dequant(is_causal, gqa_layout, global_window_size, local_window_size, query_dtype,
                                  context_dtype, compute_dtype)


class MojoPagedDecodeNstepSWAWithKVDequant(_PagedSWAKVDequantBase, MojoOperator):
    """`MojoPagedDecodeNstepSWA` over an int8 K/V cache with per-channel scales: ``S`` query tokens per sequence, the
    arithmetic of `MojoPagedPrefillSWAWithKVDequant` applied to the ``S`` rows of each sequence.

    ``total_seq_lens`` counts the ``S`` new tokens: step ``j`` of a row of ``kv_len`` keys sits at position
    ``p = kv_len - S + j`` and sees key ``t`` iff ``t <= p`` and, when a window is set, ``t >= p - local_window_size`` or
    ``t < global_window_size``.

    forward(query [B,S,Hq,D], query_scale (None: the query is not quantised), key_cache [N,Hkv,page,D] int8,
            key_scale [Hkv,D], value_cache int8, value_scale [Hkv,D], total_seq_lens [B] i32, block_table [B,nb] i32,
            softmax_scale=None, *, max_total_seq_len=None) -> [B,S,Hq,D]; rows with seq_len <= 0 are zeros.
    """

    def __init__(self, is_causal: bool = True, gqa_layout: str = "AABB", global_window_size: Optional[int] = None,
                 local_window_size: Optional[int] = None, query_dtype: torch.dtype = torch.bfloat16,
                 context_dtype: torch.dtype = torch.int8, compute_dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        self._init_swa_kv_dequant(is_causal, gqa_layout, global_window_size, local_window_size, query_dtype,
                                  context_dtype, compute_dtype)


class MojoPagedPrefillSWAWithKVDequant(_PagedSWAKVDequantBase, MojoOperator):
    """`MojoPagedPrefillSWA` over an int8 K/V cache with per-channel scales.

    forward(query [T,Hq,D], query_scale (None), key_cache int8, key_scale [Hkv,D], value_cache int8, value_scale [Hkv,D],
            cu_q_lens [B+1] i32, block_table [B,nb] i32, softmax_scale=None, cu_total_seq_lens=None, max_q_len=None,
            max_total_seq_len=None) -> [T,Hq,D]
    """

    def __init__(self, is_causal: bool = True, gqa_layout: str = "AABB", global_window_size: Optional[int] = None,
                 local_window_size: Optional[int] = None, query_dtype: torch.dtype = torch.bfloat16,
                 context_dtype: torch.dtype = torch.int8, compute_dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        self._init_swa_kv_dequant(is_causal, gqa_layout, global_window_size, local_window_size, query_dtype,
                                  context_dtype, compute_dtype)


class MojoPackedSdpa(MojoOperator):
    """Packed var-len BIDIRECTIONAL attention over contiguous K/V: the attention of a vision tower, where every sequence is
    one image or one window.  The semantics of the reference's ``MojoSWA(is_causal=False, gqa_layout=...)`` (:747-835), under
    a name of its own: sequence ``b`` owns query rows ``[cu_q_lens[b], cu_q_lens[b+1])`` and K/V rows
    ``[cu_total_seq_lens[b], cu_total_seq_lens[b+1])``, and every query row of the sequence sees every key of it.  ``q_len``
    and ``kv_len`` are independent; ``kv_len < q_len`` is legal (there is no offset).

    forward(query [Tq,Hq,D], key [Tk,Hkv,D], value [Tk,Hkv,D], cu_q_lens [B+1] i32, cu_total_seq_lens [B+1] i32,
            softmax_scale=None, *, max_q_len=None, max_total_seq_len=None) -> [Tq,Hq,D]
    """

    def __init__(self, gqa_layout: str = "AABB"):
        super().__init__()
        if gqa_layout not in _GQA_LAYOUTS:
            raise ValueError(f"gqa_layout must be one of ['ABAB', 'AABB'], got {gqa_layout}")
        self.gqa_layout = gqa_layout
        self.gqa_interleave = gqa_layout == "ABAB"

    def extra_repr(self) -> str:
        return f"gqa_layout={self.gqa_layout}"
