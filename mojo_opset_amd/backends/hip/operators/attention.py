"""HIP<Op> classes of the paged attention family."""
import math
from typing import Optional

import torch

from ....core.operators.attention import (MojoPagedDecodeGQA, MojoPagedDecodeNstepSWA, MojoPagedDecodeSWA,
                                          MojoPackedSdpa, MojoPagedPrefillGQA, MojoPagedPrefillSWA, MojoSdpa, MojoSWA,
                                          assert_nstep_query,
                                          assert_paged_decode_contract, assert_paged_prefill_contract,
                                          assert_swa_packed_contract)
from .... import switches
from .. import lib as L

_ROCM = ["rocm"]


def _validate_tables() -> bool:
    """Opt-in host check that reproduces the golden's ValueError for a row whose first page id is
    negative although its length is positive (`core/operators/attention.py:186-187`).  Off by default
    because it costs a device->host sync per call and cannot run under graph capture; without it such
    a row is computed over zero K/V (the kernel's treatment of every negative page id).  The same switch checks the
    ``max_total_seq_len`` / ``max_q_len`` hints against the device-side lengths (a length above its hint is truncated
    to the hint by the kernels)."""
    return switches.get("MOJO_HIP_VALIDATE", "0") == "1"


def _capturing(t: torch.Tensor) -> bool:
    return t.is_cuda and torch.cuda.is_current_stream_capturing()


def _check_cache_layout(key_cache, value_cache, what):
    if key_cache.stride() != value_cache.stride() or key_cache.stride(-1) != 1:
        raise NotImplementedError(f"{what}: key/value caches must share strides and be dense in head_dim")


def _paged_decode(op, what, symbols, query, key_cache, value_cache, total_seq_lens, block_tables, softmax_scale,
                 max_total_seq_len, leave_empty_rows, scales=None, windows=()):
    """The host path of every paged decode op, from the opt-in table check to the launch.  ``what``: the class name in
    messages; ``symbols``: the C workspace query and entry point; ``scales``: (key_scale, value_scale) of the int8 cache,
    dense; ``windows``: (local, global) of the SWA ABI, (local, global, steps) of the n-step one, whose query is
    ``[B, S, Hq, D]``.  The caller has checked its own contract and envelope."""
    batch, (hq, dim) = query.shape[0], query.shape[-2:]
    hkv, page = key_cache.shape[1], key_cache.shape[2]
    if _validate_tables() and batch > 0 and block_tables.shape[1] > 0:
        if bool(((total_seq_lens > 0) & (block_tables[:, 0] < 0)).any()):
            raise ValueError("Paged decode requires a valid block table for rows with kv lens > 0.")
        if max_total_seq_len is not None and int(total_seq_lens.max()) > int(max_total_seq_len):
            raise ValueError(f"{what}: a total_seq_lens entry exceeds max_total_seq_len")
    q = query if query.is_contiguous() else query.contiguous()
    tables = block_tables if block_tables.stride(1) == 1 else block_tables.contiguous()
    lens = total_seq_lens if total_seq_lens.is_contiguous() else total_seq_lens.contiguous()
    scale = 1.0 / math.sqrt(dim) if softmax_scale is None else float(softmax_scale)
    hint = int(max_total_seq_len) if max_total_seq_len is not None else 0
    out = torch.empty_like(q)
    lib = L.load()
    ws_bytes = getattr(lib, symbols[0])(batch, hq, hkv, dim, page, tables.shape[1], hint, *windows)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=q.device)
    if scales is None:
        caches, extra = (L.ptr(key_cache), L.ptr(value_cache)), windows
    else:
        caches = (L.ptr(key_cache), L.ptr(scales[0]), L.ptr(value_cache), L.ptr(scales[1]))
        extra = (L.dtype_code(scales[0].dtype), *windows)
    L.check(getattr(lib, symbols[1])(
        L.ptr(q), *caches, L.ptr(lens), L.ptr(tables), L.ptr(out), L.ptr(ws),
        ws.numel(), batch, hq, hkv, dim, page, tables.shape[1], tables.stride(0), key_cache.stride(0),
        key_cache.stride(1), key_cache.stride(2), hint, scale, 1 if op.gqa_layout == "ABAB" else 0,
        # replay contract of padded rows (seq_len <= 0): untouched while a graph is being captured, zeros eagerly
        1 if (_capturing(q) if leave_empty_rows is None else leave_empty_rows) else 0,
        L.dtype_code(q.dtype), *extra, L.stream_of(q)), what)
    return out


def _paged_prefill(op, what, symbols, query, key_cache, value_cache, cu_q_lens, block_tables, softmax_scale,
                  cu_total_seq_lens, max_q_len, max_total_seq_len, scales=None, windows=()):
    """The host path of every paged prefill op (arguments as `_paged_decode`).  The int8 op's workspace holds its scratch
    pages, so it is never absent, and its hint is checked as the upper bound it must be there."""
    tokens, hq, dim = query.shape
    n_blocks, hkv, page = key_cache.shape[:3]
    batch = cu_q_lens.shape[0] - 1
    if _validate_tables() and batch > 0 and block_tables.shape[1] > 0:
        q_lens = cu_q_lens[1:] - cu_q_lens[:-1]
        kv_lens = q_lens if cu_total_seq_lens is None else cu_total_seq_lens[1:] - cu_total_seq_lens[:-1]
        if bool(((q_lens > 0) & (kv_lens > 0) & (block_tables[:, 0] < 0)).any()):
            raise ValueError("Paged prefill requires a valid block table for rows with kv lens > 0.")
        if scales is not None and max_total_seq_len and int(kv_lens.max()) > int(max_total_seq_len):
            raise ValueError(f"{what}: a sequence's kv length exceeds max_total_seq_len (the hint sizes the scratch "
                             f"pages: it must be an upper bound)")
    q = query if query.is_contiguous() else query.contiguous()
    tables = block_tables if block_tables.stride(1) == 1 else block_tables.contiguous()
    cu_q = cu_q_lens.contiguous()
    cu_kv = None if cu_total_seq_lens is None else cu_total_seq_lens.contiguous()
    scale = 1.0 / math.sqrt(dim) if softmax_scale is None else float(softmax_scale)
    out = torch.empty_like(q)
    lib = L.load()
    hint_q = int(max_q_len) if max_q_len else 0
    hint_kv = int(max_total_seq_len) if max_total_seq_len else 0
    # few, long blocks (a chunked prefill against a long cache) are cut along the keys: fp32 partials + a merge launch
    ws_bytes = getattr(lib, symbols[0])(tokens, batch, hq, hkv, dim, page, tables.shape[1], hint_q, hint_kv, *windows)
    if scales is None:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device) if ws_bytes > 0 else None
        caches, pool, extra = (L.ptr(key_cache), L.ptr(value_cache)), (), ()
    else:
        ws_bytes = max(ws_bytes, 256)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device)   # (the allocator aligns to >= 256 bytes)
        caches = (L.ptr(key_cache), L.ptr(scales[0]), L.ptr(value_cache), L.ptr(scales[1]))
        pool, extra = (n_blocks,), (L.dtype_code(scales[0].dtype),)
    L.check(getattr(lib, symbols[1])(
        L.ptr(q), *caches, L.ptr(cu_q), L.ptr(cu_kv), L.ptr(tables), L.ptr(out),
        tokens, batch, hq, hkv, dim, *pool, page, tables.shape[1], tables.stride(0), key_cache.stride(0),
        key_cache.stride(1), key_cache.stride(2), hint_q, hint_kv, scale,
        1 if op.gqa_layout == "ABAB" else 0, L.dtype_code(q.dtype), *extra, L.ptr(ws), ws_bytes, *windows, L.stream_of(q)), what)
    return out


def _check_16bit_caches(what, query, key_cache, value_cache):
    hq, dim = query.shape[-2:]
    n_blocks, hkv, page, dim_c = key_cache.shape
    assert dim_c == dim and value_cache.shape == key_cache.shape and hq % hkv == 0
    assert query.dtype == key_cache.dtype == value_cache.dtype
    _check_cache_layout(key_cache, value_cache, what)


_DECODE_GQA = ("mojo_hip_paged_decode_gqa_workspace_bytes", "mojo_hip_paged_decode_gqa")
_DECODE_SWA = ("mojo_hip_paged_decode_swa_workspace_bytes", "mojo_hip_paged_decode_swa")
_DECODE_NSTEP = ("mojo_hip_paged_decode_nstep_workspace_bytes", "mojo_hip_paged_decode_nstep")
_PREFILL_GQA = ("mojo_hip_paged_prefill_gqa_workspace_bytes", "mojo_hip_paged_prefill_gqa")
_PREFILL_SWA = ("mojo_hip_paged_prefill_swa_workspace_bytes", "mojo_hip_paged_prefill_swa")
_SWA_PACKED = ("mojo_hip_swa_packed_workspace_bytes", "mojo_hip_swa_packed")
_SDPA = ("mojo_hip_sdpa_workspace_bytes", "mojo_hip_sdpa")
_PACKED_SDPA = ("mojo_hip_packed_sdpa_workspace_bytes", "mojo_hip_packed_sdpa")


class HIPPagedDecodeGQA(MojoPagedDecodeGQA):
    supported_platforms_list = _ROCM

    def forward(self, query, key_cache, value_cache, total_seq_lens, block_tables,
                softmax_scale: Optional[float] = None, mask: Optional[torch.Tensor] = None, *,
                max_total_seq_len: Optional[int] = None, leave_empty_rows: Optional[bool] = None):
        assert_paged_decode_contract(block_tables, total_seq_lens)
        if not self.is_causal or mask is not None:
            raise NotImplementedError("HIPPagedDecodeGQA supports causal attention without an explicit mask only")
        L.require_cuda(query, key_cache, value_cache, total_seq_lens, block_tables)
        _check_16bit_caches("HIPPagedDecodeGQA", query, key_cache, value_cache)
        return _paged_decode(self, "HIPPagedDecodeGQA", _DECODE_GQA, query, key_cache, value_cache, total_seq_lens,
                             block_tables, softmax_scale, max_total_seq_len, leave_empty_rows)


class HIPPagedPrefillGQA(MojoPagedPrefillGQA):
    supported_platforms_list = _ROCM

    def forward(self, query, key_cache, value_cache, cu_q_lens, block_tables, softmax_scale: Optional[float] = None,
                cu_total_seq_lens: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                max_q_len: Optional[int] = None, max_total_seq_len: Optional[int] = None):
        assert_paged_prefill_contract(cu_q_lens, block_tables, cu_total_seq_lens)
        if not self.is_causal or mask is not None:
            raise NotImplementedError("HIPPagedPrefillGQA supports causal attention without an explicit mask only")
        L.require_cuda(query, key_cache, value_cache, cu_q_lens, block_tables, cu_total_seq_lens)
        _check_16bit_caches("HIPPagedPrefillGQA", query, key_cache, value_cache)
        return _paged_prefill(self, "HIPPagedPrefillGQA", _PREFILL_GQA, query, key_cache, value_cache, cu_q_lens,
                              block_tables, softmax_scale, cu_total_seq_lens, max_q_len, max_total_seq_len)


def _swa_windows(op, what):
    """(local, global) of the C ABI from the reference's attributes: local < 0 = none, global <= 0 = none.  Host-side
    Python ints only (no sync, capture-safe).  Raises the ValueError of the windows that leave a row without any
    visible key — where the golden's softmax returns NaN: a negative size, or ``global_window_size=0`` alone."""
    local, glob = op.local_window_size, op.global_window_size
    for name, v in (("local_window_size", local), ("global_window_size", glob)):
        if v is not None and int(v) < 0:
            raise ValueError(f"{what}: {name} must be None or >= 0, got {v}")
    if local is None and glob is not None and int(glob) == 0:
        raise ValueError(f"{what}: global_window_size=0 without a local window leaves no key visible")
    return (-1 if local is None else int(local)), (0 if glob is None else int(glob))


class HIPPagedDecodeSWA(MojoPagedDecodeSWA):
    """Sliding-window paged decode: the GQA decode kernels walking only the tiles of the global and local ranges (DESIGN
    §4.10).  With no window, or ``is_causal=False`` (no mask at all), its entry point runs the GQA op itself, bit for bit."""
    supported_platforms_list = _ROCM

    def forward(self, query, key_cache, value_cache, total_seq_lens, block_table, softmax_scale: Optional[float] = None,
                *, max_total_seq_len: Optional[int] = None, leave_empty_rows: Optional[bool] = None):
        assert_paged_decode_contract(block_table, total_seq_lens)
        windows = _swa_windows(self, "HIPPagedDecodeSWA")
        if not self.is_causal:
            windows = (-1, 0)
        L.require_cuda(query, key_cache, value_cache, total_seq_lens, block_table)
        _check_16bit_caches("HIPPagedDecodeSWA", query, key_cache, value_cache)
        return _paged_decode(self, "HIPPagedDecodeSWA", _DECODE_SWA, query, key_cache, value_cache, total_seq_lens,
                             block_table, softmax_scale, max_total_seq_len, leave_empty_rows, windows=windows)


def _nstep_composed(op, what, symbols, query, key_cache, value_cache, total_seq_lens, block_table, softmax_scale,
                    max_total_seq_len, leave_empty_rows, windows, scales=None):
    """The composed route of the n-step ops: the single-step kernels (``symbols``), one launch per step, step ``j`` on
    ``query[:, j]`` with the lengths ``len - (S - 1 - j)`` computed on the device.  Each call zeroes its empty rows; rows of
    sequences without keys are then left out of the copy where the caller keeps them (graph replay contract)."""
    steps = query.shape[1]
    leave = _capturing(query) if leave_empty_rows is None else leave_empty_rows
    out = torch.empty(query.shape, dtype=query.dtype, device=query.device)
    keep = (total_seq_lens > 0)[:, None, None] if leave else None
    for j in range(steps):
        back = steps - 1 - j
        lens_j = total_seq_lens if back == 0 else torch.where(total_seq_lens > 0, total_seq_lens - back, total_seq_lens)
        o_j = _paged_decode(op, what, symbols, query[:, j], key_cache, value_cache, lens_j, block_table,
                            softmax_scale, max_total_seq_len, False, scales=scales, windows=windows)
        out[:, j] = o_j if keep is None else torch.where(keep, o_j, out[:, j])
    return out


class HIPPagedDecodeNstepSWA(MojoPagedDecodeNstepSWA):
    """``S`` query tokens per sequence in one pass over the paged cache: the matrix-core decode kernel with
    (step, head) pairs in the 16 columns of its score product, so the K/V bytes are read once per block of ``16 // G`` steps.
    ``S = 1`` is `HIPPagedDecodeSWA`, bit for bit.

    Geometries that kernel does not take — ``head_dim`` other than 64 / 128, pages that are no power of two >= 16, more than
    16 query heads per kv head, ``MOJO_HIP_DECODE_MFMA=0`` — run the COMPOSED route: ``S`` single-step launches, step ``j``
    on ``query[:, j]`` with the lengths ``len - (S - 1 - j)`` (computed on the device: no sync, capture-safe).  It is
    correct and costs ``S`` times the bytes.

    Beyond the golden: a row with ``0 < len < S`` (the golden returns NaN) stores zeros for the steps that see no key, and
    raises ``ValueError`` under ``MOJO_HIP_VALIDATE=1``; negative page ids are holes as in the single-step ops."""
    supported_platforms_list = _ROCM

    def forward(self, query, key_cache, value_cache, total_seq_lens, block_table, softmax_scale: Optional[float] = None,
                *, max_total_seq_len: Optional[int] = None, leave_empty_rows: Optional[bool] = None):
        what = "HIPPagedDecodeNstepSWA"
        assert_paged_decode_contract(block_table, total_seq_lens)
        assert_nstep_query(query)
        if not self.is_causal:
            raise NotImplementedError(f"{what} supports causal attention only")
        windows = _swa_windows(self, what)
        L.require_cuda(query, key_cache, value_cache, total_seq_lens, block_table)
        _check_16bit_caches(what, query, key_cache, value_cache)
        batch, steps, hq, dim = query.shape
        if steps == 0:
            return torch.empty_like(query)
        if _validate_tables() and batch > 0 and bool(((total_seq_lens > 0) & (total_seq_lens < steps)).any()):
            raise ValueError(f"{what}: a row holds fewer keys than the {steps} query steps it counts")
        hint = int(max_total_seq_len) if max_total_seq_len is not None else 0
        fused = L.load().mojo_hip_paged_decode_nstep_workspace_bytes(
            batch, hq, key_cache.shape[1], dim, key_cache.shape[2], block_table.shape[1], hint, *windows, steps) >= 0
        if fused:
            return _paged_decode(self, what, _DECODE_NSTEP, query, key_cache, value_cache, total_seq_lens, block_table,
                                 softmax_scale, max_total_seq_len, leave_empty_rows, windows=(*windows, steps))
        return _nstep_composed(self, what, _DECODE_SWA, query, key_cache, value_cache, total_seq_lens, block_table,
                               softmax_scale, max_total_seq_len, leave_empty_rows, windows)


class HIPPagedPrefillSWA(MojoPagedPrefillSWA):
    """Sliding-window paged prefill: the GQA prefill kernel walking the key tiles of the global range and of the block's
    local range only.  With no window its entry point runs the GQA op itself, bit for bit."""
    supported_platforms_list = _ROCM

    def forward(self, query, key_cache, value_cache, cu_q_lens, block_table, softmax_scale: Optional[float] = None,
                cu_total_seq_lens: Optional[torch.Tensor] = None, *, max_q_len: Optional[int] = None,
                max_total_seq_len: Optional[int] = None):
        assert_paged_prefill_contract(cu_q_lens, block_table, cu_total_seq_lens)
        if not self.is_causal:
            raise NotImplementedError("HIPPagedPrefillSWA supports causal attention only")
        windows = _swa_windows(self, "HIPPagedPrefillSWA")
        L.require_cuda(query, key_cache, value_cache, cu_q_lens, block_table, cu_total_seq_lens)
        _check_16bit_caches("HIPPagedPrefillSWA", query, key_cache, value_cache)
        return _paged_prefill(self, "HIPPagedPrefillSWA", _PREFILL_SWA, query, key_cache, value_cache, cu_q_lens,
                              block_table, softmax_scale, cu_total_seq_lens, max_q_len, max_total_seq_len, windows=windows)


def _kv_in_place(key, value) -> bool:
    """K and V can be read where they are: one set of strides, dense in head_dim, token and head strides multiples of 8
    elements (16-byte rows), both bases 16-byte aligned.  Views into a fused QKV projection qualify."""
    return (key.stride() == value.stride() and key.stride(2) == 1 and key.stride(0) % 8 == 0 and key.stride(1) % 8 == 0
            and key.data_ptr() % 16 == 0 and value.data_ptr() % 16 == 0)


class HIPSWA(MojoSWA):
    """Packed var-len attention over contiguous K/V: the paged prefill kernel with the row of a key computed
    (``(cu_total_seq_lens[b] + key) * token stride``, 64-bit) where the paged ops look it up — no table, no page-id loads,
    no hole scan.  The same bits as `HIPPagedPrefillSWA` / `HIPPagedPrefillGQA` on the same tokens at the same key split.

    K and V are read in place when they share strides, are dense in ``head_dim``, have token and head strides that are
    multiples of 8 elements and 16-byte aligned bases (views into a fused QKV buffer do); otherwise both are made contiguous.
    No host sync, capture-safe; ``max_q_len`` / ``max_total_seq_len`` are the upper-bound hints of the paged prefill.

    Contract: ``cu_q_lens[0] == 0``; ``cu_total_seq_lens[0]`` may be positive; ``kv_len >= q_len`` per sequence.  Beyond the
    reference: rows of a sequence with ``kv_len <= 0`` and rows at or past ``cu_q_lens[-1]`` are zeros.
    ``MOJO_HIP_VALIDATE=1`` (a host sync) raises ``ValueError`` for arrays that decrease, ends past ``Tq`` / ``Tk``,
    ``kv_len < q_len`` and a length above its hint.  Without it such a call is computed as the paged prefill computes the same
    lengths: a length above its hint is truncated to the hint (query rows past it are zeros, keys past it unseen), the
    ``q_len - kv_len`` leading rows of a sequence with fewer keys than queries see no key and hold no defined value, and
    every ``cu_total_seq_lens`` entry is clamped to ``[0, Tk]`` by the kernel, so no read leaves the tensors."""
    supported_platforms_list = _ROCM

    def forward(self, query, key, value, cu_q_lens, cu_total_seq_lens, softmax_scale: Optional[float] = None, *,
                max_q_len: Optional[int] = None, max_total_seq_len: Optional[int] = None):
        what = "HIPSWA"
        assert_swa_packed_contract(query, key, value, cu_q_lens, cu_total_seq_lens)
        if not self.is_causal:
            raise NotImplementedError(f"{what} supports causal attention only")
        windows = _swa_windows(self, what)
        L.require_cuda(query, key, value, cu_q_lens, cu_total_seq_lens)
        tokens, hq, dim = query.shape
        kv_tokens, hkv = key.shape[:2]
        batch = cu_q_lens.shape[0] - 1
        hint_q = int(max_q_len) if max_q_len else 0
        hint_kv = int(max_total_seq_len) if max_total_seq_len else 0
        if _validate_tables() and batch > 0:
            q_lens, kv_lens = cu_q_lens[1:] - cu_q_lens[:-1], cu_total_seq_lens[1:] - cu_total_seq_lens[:-1]
            if int(cu_q_lens[0]) != 0 or int(cu_total_seq_lens[0]) < 0 or bool((q_lens < 0).any()) or bool((kv_lens < 0).any()):
                raise ValueError(f"{what}: cu_q_lens must start at 0 and both cumulative arrays must be non-decreasing")
            if int(cu_q_lens[-1]) > tokens or int(cu_total_seq_lens[-1]) > kv_tokens:
                raise ValueError(f"{what}: the cumulative lengths end past the query ({tokens}) or key ({kv_tokens}) tokens")
            if bool((kv_lens < q_lens).any()):
                raise ValueError(f"{what}: a sequence has fewer keys than queries (kv_len >= q_len is the contract)")
            if (hint_q and int(q_lens.max()) > hint_q) or (hint_kv and int(kv_lens.max()) > hint_kv):
                raise ValueError(f"{what}: a sequence's length exceeds its max_q_len / max_total_seq_len hint")
        q = query if query.is_contiguous() else query.contiguous()
        if tokens == 0:
            return torch.empty_like(q)
        if kv_tokens == 0:                                 # no key anywhere: every row reads as zeros
            return torch.zeros_like(q)
        k, v = (key, value) if _kv_in_place(key, value) else (key.contiguous(), value.contiguous())
        cu_q, cu_kv = cu_q_lens.contiguous(), cu_total_seq_lens.contiguous()
        scale = 1.0 / math.sqrt(dim) if softmax_scale is None else float(softmax_scale)
        out = torch.empty_like(q)
        lib = L.load()
        ws_bytes = getattr(lib, _SWA_PACKED[0])(tokens, kv_tokens, batch, hq, hkv, dim, hint_q, hint_kv, *windows)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device) if ws_bytes > 0 else None
        L.check(getattr(lib, _SWA_PACKED[1])(
            L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(cu_q), L.ptr(cu_kv), L.ptr(out), tokens, kv_tokens, batch, hq, hkv, dim,
            k.stride(0), k.stride(1), hint_q, hint_kv, scale, 1 if self.gqa_layout == "ABAB" else 0,
            L.dtype_code(q.dtype), L.ptr(ws), ws_bytes, *windows, L.stream_of(q)), what)
        return out


def _sdpa_in_place(t) -> bool:
    """A ``[B,H,S,D]`` tensor the kernel addresses where it is: dense in ``head_dim``, batch / head / token strides that are
    multiples of 8 elements (16-byte rows), a 16-byte aligned base.  The token-major view (``[B,S,H,D]`` memory seen as
    ``[B,H,S,D]``) and a contiguous tensor both qualify."""
    return t.stride(3) == 1 and all(st % 8 == 0 for st in t.stride()[:3]) and t.data_ptr() % 16 == 0


def _dense_aligned(t):
    """A contiguous copy on a 16-byte boundary (a contiguous tensor on a misaligned base is copied too)."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


_SDPA_DIMS, _SDPA_GROUPS = (64, 96, 128), (1, 2, 4, 8)


class HIPSdpa(MojoSdpa):
    """Bidirectional attention with an optional mask: the linear prefill kernel without its diagonal.  Every
    row sees the keys ``[0, Sk)``; ``Sk < Sq`` is legal (cross-attention).

    ``query`` is ``[B,Hq,Sq,D]`` (3-D: one batch entry), read in place as the token-major view (``x.view(b, s, n,
    d).transpose(1, 2)``) or as a contiguous tensor, and the output has the query's form; anything else is made contiguous.
    K and V are read in place under the rule of `_kv_in_place` (shared strides, dense ``head_dim``, 16-byte rows and bases),
    otherwise copied.  ``enable_gqa=True`` groups heads as ``repeat_interleave`` does (AABB).

    ``attn_mask`` must be broadcastable to ``[B,Hq,Sq,Sk]`` and is read in place through its own strides — a broadcast
    dimension is never expanded; a mask whose last stride is not 1 is made contiguous.  Boolean: ``False`` hides the key.
    Floating (the query's dtype or fp32): added to the scaled score, ``-inf`` allowed.

    Envelope: bf16 / fp16, ``head_dim`` 64 / 96 / 128, ``Hq / Hkv`` 1 / 2 / 4 / 8, at most four dimensions; anything else raises
    ``NotImplementedError``.  Beyond the reference: a row with no visible key (all ``False`` / ``-inf``) is zeros where torch
    leaves NaN, and ``Sk == 0`` returns zeros.  No host sync, capture-safe."""
    supported_platforms_list = _ROCM

    def forward(self, query, key, value, attn_mask: Optional[torch.Tensor] = None):
        what = "HIPSdpa"
        if query.dim() > 4 or key.dim() > 4 or value.dim() > 4:
            raise NotImplementedError(f"{what}: at most four dimensions [B,H,S,D], got {query.dim()}")
        if query.dim() < 3 or key.dim() != query.dim() or value.dim() != query.dim():
            raise RuntimeError(f"{what}: query, key and value must all be [B,H,S,D] or all [H,S,D]")
        squeeze = query.dim() == 3
        q, k, v = (t.unsqueeze(0) if squeeze else t for t in (query, key, value))
        batch, hq, sq, dim = q.shape
        hkv, sk = k.shape[1], k.shape[2]
        if k.shape[0] != batch or k.shape[3] != dim or v.shape != k.shape:
            raise RuntimeError(f"{what}: key {tuple(key.shape)} / value {tuple(value.shape)} do not match query "
                               f"{tuple(query.shape)} in batch, head_dim or each other")
        if hq != hkv and not (self.enable_gqa and hkv > 0 and hq % hkv == 0):
            raise RuntimeError(f"{what}: {hq} query heads against {hkv} key/value heads "
                               f"(enable_gqa={self.enable_gqa}: the counts must be equal, or a multiple with enable_gqa=True)")
        if not (query.dtype == key.dtype == value.dtype):
            raise RuntimeError(f"{what}: query, key and value must share a dtype, got {query.dtype}, {key.dtype}, {value.dtype}")
        if query.dtype not in (torch.bfloat16, torch.float16):
            raise NotImplementedError(f"{what}: dtype {query.dtype} (bf16 / fp16)")
        if dim not in _SDPA_DIMS:
            raise NotImplementedError(f"{what}: head_dim {dim} {_SDPA_DIMS}")
        if hq // hkv not in _SDPA_GROUPS:
            raise NotImplementedError(f"{what}: {hq // hkv} query heads per kv head {_SDPA_GROUPS}")
        mask, kind, m_strides = None, 0, (0, 0, 0)
        if attn_mask is not None:
            mask = attn_mask
            if mask.dim() > 4:
                raise NotImplementedError(f"{what}: a mask of {mask.dim()} dimensions (at most four)")
            if mask.dtype == torch.bool:
                kind = 1
            elif mask.dtype == query.dtype:
                kind = 2
            elif mask.dtype == torch.float32:
                kind = 3
            else:
                raise NotImplementedError(f"{what}: mask dtype {mask.dtype} (bool, {query.dtype} or float32)")
            shape = (1,) * (4 - mask.dim()) + tuple(mask.shape)
            if any(m != 1 and m != full for m, full in zip(shape, (batch, hq, sq, sk))):
                raise RuntimeError(f"{what}: mask {tuple(attn_mask.shape)} is not broadcastable to {(batch, hq, sq, sk)}")
            mask = mask.reshape(shape)
            if shape[3] != sk:                             # one value per row: the only broadcast that is materialised
                mask = mask.expand(shape[0], shape[1], shape[2], sk).contiguous()
            elif mask.stride(3) != 1 and sk > 1:
                mask = mask.contiguous()
            # a broadcast dimension (size 1, or expanded by the caller) is addressed with stride 0
            m_strides = tuple(0 if mask.shape[i] == 1 else mask.stride(i) for i in range(3))
            if (sq - 1) * m_strides[2] + sk + 64 >= 1 << 31:
                raise NotImplementedError(f"{what}: a (batch, head) plane of the mask must stay below 2^31 elements")
        L.require_cuda(query, key, value, attn_mask)
        if not _sdpa_in_place(q):
            q = _dense_aligned(q)
        if not (_sdpa_in_place(k) and _sdpa_in_place(v) and k.stride() == v.stride()):
            k, v = _dense_aligned(k), _dense_aligned(v)
        # the output in the query's form: token-major stays token-major, everything else is contiguous [B,H,S,D]
        if sq > 1 and hq > 1 and q.stride(2) == hq * dim and q.stride(1) == dim:
            out = torch.empty((batch, sq, hq, dim), dtype=q.dtype, device=q.device).transpose(1, 2)
        else:
            out = torch.empty((batch, hq, sq, dim), dtype=q.dtype, device=q.device)
        if batch == 0 or hq == 0 or sq == 0:
            return out[0] if squeeze else out
        if sk == 0:                                        # no key anywhere: every row reads as zeros
            out.zero_()
            return out[0] if squeeze else out
        scale = 1.0 / math.sqrt(dim) if self.scale is None else float(self.scale)
        lib = L.load()
        ws_bytes = getattr(lib, _SDPA[0])(batch, hq, hkv, sq, sk, dim)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device) if ws_bytes > 0 else None
        L.check(getattr(lib, _SDPA[1])(
            L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(mask), L.ptr(out), batch, hq, hkv, sq, sk, dim,
            q.stride(0), q.stride(1), q.stride(2), out.stride(0), out.stride(1), out.stride(2),
            k.stride(0), k.stride(1), k.stride(2), kind, *m_strides, scale, L.dtype_code(q.dtype),
            L.ptr(ws), ws_bytes, L.stream_of(q)), what)
        return out[0] if squeeze else out


class HIPPackedSdpa(MojoPackedSdpa):
    """Packed var-len bidirectional attention: the linear prefill kernel of `HIPSWA` with the walk of `HIPSdpa`
    — no offset, every whole key tile on the unmasked fast-staged loop, only a sequence's tail tile masked.  One packed
    sequence of ``Sq x Sk`` gives the bits of `HIPSdpa` on the same tokens at the same key split.

    K and V are read in place under the rule of `_kv_in_place` (views into a fused QKV buffer qualify); otherwise both are
    made contiguous.  Both GQA layouts.  Envelope: bf16 / fp16, ``head_dim`` 64 / 96 / 128, ``Hq / Hkv`` 1 / 2 / 4 / 8; anything
    else raises ``NotImplementedError`` (``head_dim`` 72 / 80 is the caller's padding to 96).  No host sync, capture-safe.

    Contract: ``cu_q_lens[0] == 0``; ``cu_total_seq_lens[0]`` may be positive; ``q_len`` and ``kv_len`` of a sequence are
    independent.  Beyond the reference: rows of a sequence with ``kv_len <= 0`` and rows at or past ``cu_q_lens[-1]`` are
    zeros.  ``max_q_len`` / ``max_total_seq_len`` are upper-bound hints: a sequence longer than ``max_q_len`` has its rows past
    the hint written as zeros, and keys at or past ``max_total_seq_len`` of a sequence are not seen.  ``MOJO_HIP_VALIDATE=1``
    (a host sync) raises ``ValueError`` for arrays that decrease, ends past ``Tq`` / ``Tk`` and a length above its hint.
    Without it every ``cu_total_seq_lens`` entry is clamped to ``[0, Tk]`` by the kernel, so no read leaves the tensors."""
    supported_platforms_list = _ROCM

    def forward(self, query, key, value, cu_q_lens, cu_total_seq_lens, softmax_scale: Optional[float] = None, *,
                max_q_len: Optional[int] = None, max_total_seq_len: Optional[int] = None):
        what = "HIPPackedSdpa"
        assert_swa_packed_contract(query, key, value, cu_q_lens, cu_total_seq_lens)
        tokens, hq, dim = query.shape
        kv_tokens, hkv = key.shape[:2]
        if query.dtype not in (torch.bfloat16, torch.float16):
            raise NotImplementedError(f"{what}: dtype {query.dtype} (bf16 / fp16)")
        if dim not in _SDPA_DIMS:
            raise NotImplementedError(f"{what}: head_dim {dim} {_SDPA_DIMS}")
        if hq // hkv not in _SDPA_GROUPS:
            raise NotImplementedError(f"{what}: {hq // hkv} query heads per kv head {_SDPA_GROUPS}")
        L.require_cuda(query, key, value, cu_q_lens, cu_total_seq_lens)
        batch = cu_q_lens.shape[0] - 1
        hint_q = int(max_q_len) if max_q_len else 0
        hint_kv = int(max_total_seq_len) if max_total_seq_len else 0
        if _validate_tables() and batch > 0:
            q_lens, kv_lens = cu_q_lens[1:] - cu_q_lens[:-1], cu_total_seq_lens[1:] - cu_total_seq_lens[:-1]
            if int(cu_q_lens[0]) != 0 or int(cu_total_seq_lens[0]) < 0 or bool((q_lens < 0).any()) or bool((kv_lens < 0).any()):
                raise ValueError(f"{what}: cu_q_lens must start at 0 and both cumulative arrays must be non-decreasing")
            if int(cu_q_lens[-1]) > tokens or int(cu_total_seq_lens[-1]) > kv_tokens:
                raise ValueError(f"{what}: the cumulative lengths end past the query ({tokens}) or key ({kv_tokens}) tokens")
            if (hint_q and int(q_lens.max()) > hint_q) or (hint_kv and int(kv_lens.max()) > hint_kv):
                raise ValueError(f"{what}: a sequence's length exceeds its max_q_len / max_total_seq_len hint")
        q = query if query.is_contiguous() else query.contiguous()
        if tokens == 0:
            return torch.empty_like(q)
        if kv_tokens == 0:                                 # no key anywhere: every row reads as zeros
            return torch.zeros_like(q)
        k, v = (key, value) if _kv_in_place(key, value) else (key.contiguous(), value.contiguous())
        cu_q, cu_kv = cu_q_lens.contiguous(), cu_total_seq_lens.contiguous()
        scale = 1.0 / math.sqrt(dim) if softmax_scale is None else float(softmax_scale)
        out = torch.empty_like(q)
        lib = L.load()
        ws_bytes = getattr(lib, _PACKED_SDPA[0])(tokens, kv_tokens, batch, hq, hkv, dim, hint_q, hint_kv)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device) if ws_bytes > 0 else None
        L.check(getattr(lib, _PACKED_SDPA[1])(
            L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(cu_q), L.ptr(cu_kv), L.ptr(out), tokens, kv_tokens, batch, hq, hkv, dim,
            k.stride(0), k.stride(1), hint_q, hint_kv, scale, 1 if self.gqa_layout == "ABAB" else 0,
            L.dtype_code(q.dtype), L.ptr(ws), ws_bytes, L.stream_of(q)), what)
        return out
