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


class MojoPagedPrefillSageGQA(_PagedGQABase, MojoOperator):
    """Causal paged prefill with int8 COMPUTE (SageAttention style; `SAGE_ATTN_OPS`): an int8 query with per-token scales, an
    int8 K cache with per-token scales, an int8 V cache with per-channel scales, and probabilities quantised to ``[0, 127]``, so
    that Q.K^T and P.V are both int8 products with exact integer sums.

    forward(query [T,Hq,D] int8, query_scale [Hq,T] fp32, key_cache [N,Hkv,page,D] int8, key_scale [N,Hkv,page] fp32,
            value_cache [N,Hkv,page,D] int8, value_scale [Hkv,D] fp32, cu_q_lens [B+1] i32, block_tables [B,nb] i32,
            softmax_scale=None, cu_total_seq_lens=None, mask=None, max_q_len=None, max_total_seq_len=None) -> [T,Hq,D] bf16

    For query row ``(t, h)`` of a sequence of ``kv_len`` keys, ``kh`` the kv head of ``h``:

    1. ``dot[j] = sum_d q8[t,h,d] * k8[j,kh,d]`` (an exact integer);
    2. ``s[j] = ((float(dot[j]) * softmax_scale) * query_scale[h,t]) * key_scale[j,kh]``, every product fp32, in this order;
    3. key ``j`` is visible iff ``j <= kv_len - q_len + (t - seq_start)``; ``m = max s[j]`` over the visible keys;
    4. ``p[j] = round_half_even(exp(s[j] - m) * 127)`` for a visible key, 0 for a hidden one: quantised against the FINAL maximum;
    5. ``out[t,h,d] = bf16(value_scale[kh,d] * (sum_j p[j] * v8[j,kh,d]) / (sum_j p[j]))`` - the divisor is the sum of the
       QUANTISED probabilities (the ``1/127`` of both sums cancels).

    Rows of a sequence with ``q_len == 0`` or ``kv_len <= 0``, and rows that see no key (``kv_len < q_len``), are zeros.

    ``forward`` below is the golden.  The scores are fp32 as stated; ``exp``, the rounding and the final quotient are evaluated
    in fp64 so that the integers ``p`` do not depend on the host's vectorised fp32 ``exp``."""

    def __init__(self, is_causal: bool = True, gqa_layout: str = "AABB", query_dtype: torch.dtype = torch.int8,
                 context_dtype: torch.dtype = torch.int8, compute_dtype: torch.dtype = torch.int8):
        super().__init__()
        self._init_gqa(is_causal, gqa_layout)
        assert query_dtype == torch.int8, f"MojoPagedPrefillSageGQA: int8 query only, got {query_dtype}"
        assert context_dtype == torch.int8, f"MojoPagedPrefillSageGQA: int8 context only, got {context_dtype}"
        assert compute_dtype == torch.int8, f"MojoPagedPrefillSageGQA: int8 compute only, got {compute_dtype}"
        self.query_dtype, self.context_dtype, self.compute_dtype = query_dtype, context_dtype, compute_dtype

    def forward(self, query, query_scale, key_cache, key_scale, value_cache, value_scale, cu_q_lens, block_tables,
                softmax_scale: Optional[float] = None, cu_total_seq_lens: Optional[torch.Tensor] = None,
                mask: Optional[torch.Tensor] = None, max_q_len: Optional[int] = None,
                max_total_seq_len: Optional[int] = None):
        assert_paged_prefill_contract(cu_q_lens, block_tables, cu_total_seq_lens)
        assert mask is None and self.is_causal, "MojoPagedPrefillSageGQA: causal attention without an explicit mask only"
        tokens, hq, dim = query.shape
        hkv, page = key_cache.shape[1], key_cache.shape[2]
        group = hq // hkv
        scale = torch.tensor(dim ** -0.5 if softmax_scale is None else softmax_scale, dtype=torch.float32)
        heads = torch.arange(hq)
        kv_of = heads % hkv if self.gqa_layout == "ABAB" else heads // group
        out = torch.zeros(tokens, hq, dim, dtype=torch.bfloat16, device=query.device)
        cu_q = cu_q_lens.tolist()
        cu_kv = cu_q if cu_total_seq_lens is None else cu_total_seq_lens.tolist()
        for b in range(len(cu_q) - 1):
            q0, q_len, kv_len = cu_q[b], cu_q[b + 1] - cu_q[b], cu_kv[b + 1] - cu_kv[b]
            if q_len <= 0 or kv_len <= 0:
                continue
            pages = block_tables[b, :(kv_len + page - 1) // page].long()
            k8 = key_cache[pages].transpose(1, 2).reshape(-1, hkv, dim)[:kv_len]          # [kv, Hkv, D]
            v8 = value_cache[pages].transpose(1, 2).reshape(-1, hkv, dim)[:kv_len]
            ks = key_scale[pages].transpose(1, 2).reshape(-1, hkv)[:kv_len].float()       # [kv, Hkv]
            q8 = query[q0:q0 + q_len]                                                     # [q, Hq, D]
            dot = torch.einsum("qhd,khd->hqk", q8.double(), k8[:, kv_of].double())        # exact: |dot| < 2^53
            s = ((dot.float() * scale) * query_scale[:, q0:q0 + q_len].float()[:, :, None]) * ks[:, kv_of].T[:, None, :]
            visible = torch.arange(kv_len)[None, :] <= (kv_len - q_len + torch.arange(q_len))[:, None]
            m = s.masked_fill(~visible, float("-inf")).amax(dim=-1, keepdim=True)
            p = torch.where(visible, torch.round(torch.exp((s - m).double()) * 127), 0.0)  # [Hq, q, kv] integers
            num = torch.einsum("hqk,khd->qhd", p, v8[:, kv_of].double())                  # exact integer sums
            den = p.sum(dim=-1).T[:, :, None]                                             # [q, Hq, 1]
            o = value_scale.double()[kv_of][None] * num / den
            out[q0:q0 + q_len] = torch.where(den > 0, o, 0.0).to(torch.bfloat16)
        return out

    def extra_repr(self) -> str:
        return (f"is_causal={self.is_causal!r}, gqa_layout={self.gqa_layout!r}, query_dtype={self.query_dtype!r}, "
                f"context_dtype={self.context_dtype!r}, compute_dtype={self.compute_dtype!r}")


class _NSADecodeBase:
    """Constructor and per-sequence golden of the native-sparse-attention decode pair (`NSA_ATTN_OPS`;
    `mojo_opset/experimental/operators/attention.py:1266-1485`).  MHA: K/V have the query's ``H`` heads.  For one sequence of
    ``sl`` keys and one head, with ``scale = softmax_scale or 1/sqrt(D)``, ``cr = compress_ratio``, ``bs = block_size`` (the
    SELECTION block, not the cache page), ``nsel = num_selected_blocks``, ``ws = window_size``:

    * compressed: ``C = sl // cr`` groups of ``cr`` consecutive keys (the ``sl % cr`` tail keys are in no group), ``ck_j`` /
      ``cv_j`` the group means, ``pc = softmax_j(scale * q.ck_j)``, ``out_comp = sum_j pc_j cv_j``; zeros when ``C == 0``;
    * selection: block ``b`` of ``nb = ceil(sl / bs)`` scores the sum of ``pc_j`` over its ``bs // cr`` groups with
      ``j < C`` (0 without one); the ``min(nsel, nb)`` highest blocks are taken per head — AMONG EQUAL SCORES THE LOWER BLOCK
      INDEX FIRST (this project's rule: the reference's ``torch.topk`` leaves ties unspecified) — and ``out_sel`` is softmax
      attention over the keys of the taken blocks, the partial last block included;
    * window: ``out_win`` is softmax attention over the last ``min(ws, sl)`` keys;
    * ``g = sigmoid(q . gate_proj[h])`` (three values, parameter ``gate_proj [H, D, 3]``) and
      ``out = g0 out_comp + g1 out_sel + g2 out_win``.  A sequence with ``sl <= 0`` gives zeros; ``is_causal`` has no effect.

    ``forward`` of the two classes is the golden, with the reference's roundings: group means rounded to the storage dtype,
    score einsums in the storage dtype, probabilities cast to it before P.V, each branch and the gate in it.  A backend that
    keeps scores, probabilities and the weighted sum in fp32 and rounds once (the HIP one) stays inside the reference's
    ``atol = rtol = 1e-2``; where two block scores are closer than these roundings' noise the two may take different blocks."""

    def _init_nsa(self, num_heads, head_dim, compress_ratio, num_selected_blocks, block_size, window_size, is_causal):
        self.num_heads, self.head_dim = num_heads, head_dim
        self.compress_ratio, self.num_selected_blocks = compress_ratio, num_selected_blocks
        self.block_size, self.window_size, self.is_causal = block_size, window_size, is_causal
        self.gate_proj = torch.nn.Parameter(torch.empty(num_heads, head_dim, 3))

    def extra_repr(self) -> str:
        return (f"num_heads={self.num_heads}, head_dim={self.head_dim}, compress_ratio={self.compress_ratio}, "
                f"num_selected_blocks={self.num_selected_blocks}, block_size={self.block_size}, "
                f"window_size={self.window_size}, is_causal={self.is_causal}")

    @staticmethod
    def _attend(q, k, v, scale, mask=None):
        """q [H,D], k / v [S,H,D] -> [H,D]: fp32 softmax of the storage-dtype scores, probabilities back in the storage dtype."""
        scores = torch.einsum("hd,shd->hs", q, k).float() * scale
        if mask is not None:
            scores = scores.masked_fill(~mask, float("-inf"))
        probs = torch.nan_to_num(torch.softmax(scores, dim=-1, dtype=torch.float32).to(q.dtype), nan=0.0)
        return torch.einsum("hs,shd->hd", probs, v)

    def _decode_one(self, q, k, v, scale):
        sl, heads, dim = k.shape
        cr, bs = self.compress_ratio, self.block_size
        n_groups, nb = sl // cr, (sl + bs - 1) // bs
        ck = k[:n_groups * cr].reshape(n_groups, cr, heads, dim).mean(dim=1)
        cv = v[:n_groups * cr].reshape(n_groups, cr, heads, dim).mean(dim=1)
        pc = (torch.einsum("hd,chd->hc", q, ck) * scale).softmax(dim=-1, dtype=torch.float32)
        block_score = torch.zeros(heads, nb, dtype=torch.float32, device=q.device)
        for b in range(nb):
            if b * (bs // cr) < n_groups:
                block_score[:, b] = pc[:, b * (bs // cr):min((b + 1) * (bs // cr), n_groups)].sum(dim=-1)
        taken = torch.sort(block_score, dim=-1, descending=True, stable=True).indices[:, :min(self.num_selected_blocks, nb)]
        block_mask = torch.zeros(heads, nb, dtype=torch.bool, device=q.device).scatter_(1, taken, True)
        mask = block_mask.repeat_interleave(bs, dim=1)[:, :sl]
        start = max(0, sl - self.window_size)
        g = torch.sigmoid(torch.einsum("hd,hdc->hc", q, self.gate_proj.to(q.dtype)))
        return (g[:, 0:1] * self._attend(q, ck, cv, scale) + g[:, 1:2] * self._attend(q, k, v, scale, mask) +
                g[:, 2:3] * self._attend(q, k[start:], v[start:], scale))


class MojoDecodeNSA(_NSADecodeBase, MojoOperator):
    """Native sparse attention, one query token per sequence over contiguous K/V (see `_NSADecodeBase`).

    forward(query [B,H,D], key [B,S,H,D], value [B,S,H,D], total_seq_lens=None ([B] i32; None: S), softmax_scale=None)
    -> [B,H,D]"""

    def __init__(self, num_heads, head_dim, compress_ratio=4, num_selected_blocks=16, block_size=64, window_size=512,
                 is_causal=True, **kwargs):
        super().__init__(**kwargs)
        self._init_nsa(num_heads, head_dim, compress_ratio, num_selected_blocks, block_size, window_size, is_causal)

    def forward(self, query, key, value, total_seq_lens: Optional[torch.Tensor] = None, softmax_scale: Optional[float] = None):
        if total_seq_lens is not None:
            assert total_seq_lens.dtype == torch.int32
        scale = query.shape[-1] ** -0.5 if softmax_scale is None else softmax_scale
        out = torch.zeros_like(query)
        lens = [key.shape[1]] * query.shape[0] if total_seq_lens is None else total_seq_lens.tolist()
        for i, sl in enumerate(lens):
            if sl > 0:
                out[i] = self._decode_one(query[i], key[i, :sl], value[i, :sl], scale)
        return out


class MojoPagedDecodeNSA(_NSADecodeBase, MojoOperator):
    """Native sparse attention, one query token per sequence over a paged KV cache (see `_NSADecodeBase`).  The cache page
    and the selection block are independent.  Every key from the first negative or out-of-pool page id on is a zero K / V
    row; a negative FIRST page id of a sequence with keys raises ``ValueError``.

    forward(query [B,H,D], key_cache / value_cache [N,H,page,D], total_seq_lens [B] i32, block_tables [B,nb] i32,
            softmax_scale=None) -> [B,H,D]"""

    def __init__(self, num_heads, head_dim, compress_ratio=4, num_selected_blocks=16, block_size=64, window_size=512,
                 is_causal=True, **kwargs):
        super().__init__(**kwargs)
        self._init_nsa(num_heads, head_dim, compress_ratio, num_selected_blocks, block_size, window_size, is_causal)

    def forward(self, query, key_cache, value_cache, total_seq_lens, block_tables, softmax_scale: Optional[float] = None):
        assert_paged_decode_contract(block_tables, total_seq_lens)
        n_blocks, heads, page, dim = key_cache.shape
        scale = dim ** -0.5 if softmax_scale is None else softmax_scale
        out = torch.zeros_like(query)
        for i, sl in enumerate(total_seq_lens.tolist()):
            if sl <= 0:
                continue
            ids = block_tables[i, :(sl + page - 1) // page].tolist()
            if ids[0] < 0:
                raise ValueError("Paged decode requires a valid block table for rows with kv lens > 0.")
            bad = [j for j, n in enumerate(ids) if n < 0 or n >= n_blocks]
            ids = ids[:bad[0]] if bad else ids
            k = torch.zeros(len(ids) * page + sl, heads, dim, dtype=query.dtype, device=query.device)
            v = torch.zeros_like(k)
            if ids:
                k[:len(ids) * page] = key_cache[ids].transpose(1, 2).reshape(-1, heads, dim)
                v[:len(ids) * page] = value_cache[ids].transpose(1, 2).reshape(-1, heads, dim)
            out[i] = self._decode_one(query[i], k[:sl], v[:sl], scale)
        return out


class _NSAPrefillBase(_NSADecodeBase):
    """Per-row golden of the native-sparse-attention prefill pair (`NSA_PREFILL_OPS`;
    `mojo_opset/experimental/operators/attention.py:1488-1638`).  Row ``t`` of a sequence with ``q_len`` queries and ``kv_len``
    keys sees the first ``t_kv`` keys, ``t_kv = kv_len - q_len + t + 1`` when ``is_causal`` and ``kv_len`` otherwise (unlike
    decode, ``is_causal`` matters), and its result is the decode step of `_NSADecodeBase` on them.  Two exceptions: a row with
    ``t_kv <= 0`` gives zeros, and a row with ``0 < t_kv < compress_ratio`` IS NOT COMPRESSED (the reference's rule): its
    compressed branch is softmax attention over the ``t_kv`` raw keys, where decode gives that branch zeros at such a length.
    Roundings, ties and tolerances as in `_NSADecodeBase`."""

    def _prefill_seq(self, out, q, k, v, scale):
        """``out [q_len,H,D]`` (zeros) of one sequence: ``q [q_len,H,D]``, ``k`` / ``v [kv_len,H,D]``."""
        q_len, kv_len, cr = q.shape[0], k.shape[0], self.compress_ratio
        for t in range(q_len):
            t_kv = kv_len - q_len + t + 1 if self.is_causal else kv_len
            if t_kv >= cr:
                out[t] = self._decode_one(q[t], k[:t_kv], v[:t_kv], scale)
            elif t_kv > 0:         # one block, taken; the window is the context: three times the same attention unless ws < t_kv
                g = torch.sigmoid(torch.einsum("hd,hdc->hc", q[t], self.gate_proj.to(q.dtype)))
                full = self._attend(q[t], k[:t_kv], v[:t_kv], scale)
                start = max(0, t_kv - self.window_size)
                sel = full if self.num_selected_blocks > 0 else torch.zeros_like(full)
                out[t] = g[:, 0:1] * full + g[:, 1:2] * sel + g[:, 2:3] * self._attend(q[t], k[start:t_kv], v[start:t_kv], scale)


class MojoPrefillNSA(_NSAPrefillBase, MojoOperator):
    """Native sparse attention for packed var-len queries over contiguous K/V, ``kv_len = q_len`` (see `_NSAPrefillBase`).

    forward(query [T,H,D], key [T,H,D], value [T,H,D], cu_q_lens [B+1] i32, softmax_scale=None) -> [T,H,D]"""

    def __init__(self, num_heads, head_dim, compress_ratio=4, num_selected_blocks=16, block_size=64, window_size=512,
                 is_causal=True, **kwargs):
        super().__init__(**kwargs)
        self._init_nsa(num_heads, head_dim, compress_ratio, num_selected_blocks, block_size, window_size, is_causal)

    def forward(self, query, key, value, cu_q_lens, softmax_scale: Optional[float] = None):
        assert cu_q_lens.dtype == torch.int32
        scale = query.shape[-1] ** -0.5 if softmax_scale is None else softmax_scale
        out, cu = torch.zeros_like(query), cu_q_lens.tolist()
        for s, e in zip(cu[:-1], cu[1:]):
            self._prefill_seq(out[s:e], query[s:e], key[s:e], value[s:e], scale)
        return out


class MojoPagedPrefillNSA(_NSAPrefillBase, MojoOperator):
    """Native sparse attention for packed var-len queries over a paged KV cache (see `_NSAPrefillBase`).  The cache page and
    the selection block are independent.  Every key from the first negative or out-of-pool page id on is a zero K / V
    row; a negative FIRST page id of a sequence with keys raises ``ValueError``.

    forward(query [T,H,D], key_cache / value_cache [N,H,page,D], cu_q_lens [B+1] i32, block_tables [B,nb] i32,
            softmax_scale=None, cu_total_seq_lens=None ([B+1] i32; None: kv_len = q_len)) -> [T,H,D]"""

    def __init__(self, num_heads, head_dim, compress_ratio=4, num_selected_blocks=16, block_size=64, window_size=512,
                 is_causal=True, **kwargs):
        super().__init__(**kwargs)
        self._init_nsa(num_heads, head_dim, compress_ratio, num_selected_blocks, block_size, window_size, is_causal)

    def forward(self, query, key_cache, value_cache, cu_q_lens, block_tables, softmax_scale: Optional[float] = None,
                cu_total_seq_lens: Optional[torch.Tensor] = None):
        assert_paged_prefill_contract(cu_q_lens, block_tables, cu_total_seq_lens)
        n_blocks, heads, page, dim = key_cache.shape
        scale = dim ** -0.5 if softmax_scale is None else softmax_scale
        out, cu = torch.zeros_like(query), cu_q_lens.tolist()
        cu_kv = cu if cu_total_seq_lens is None else cu_total_seq_lens.tolist()
        for i, (s, e) in enumerate(zip(cu[:-1], cu[1:])):
            sl = min(cu_kv[i + 1] - cu_kv[i], page * block_tables.shape[1])
            if e <= s or sl <= 0:
                continue
            ids = block_tables[i, :(sl + page - 1) // page].tolist()
            if ids[0] < 0:
                raise ValueError("Paged decode requires a valid block table for rows with kv lens > 0.")
            bad = [j for j, n in enumerate(ids) if n < 0 or n >= n_blocks]
            ids = ids[:bad[0]] if bad else ids
            k = torch.zeros(len(ids) * page + sl, heads, dim, dtype=query.dtype, device=query.device)
            v = torch.zeros_like(k)
            if ids:
                k[:len(ids) * page] = key_cache[ids].transpose(1, 2).reshape(-1, heads, dim)
                v[:len(ids) * page] = value_cache[ids].transpose(1, 2).reshape(-1, heads, dim)
            self._prefill_seq(out[s:e], query[s:e], k[:sl], v[:sl], scale)
        return out


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
