"""HIP<Op> classes of the HBM-streaming operators: SwiGLU, (ResidualAdd)RMSNorm, RoPE,
RotaryEmbedding, StorePagedKVCache, the DiT block's (ResidualAdd)LayerNorm, Gelu, Silu and GridRoPE, and the vision tower's
VisionRotaryEmbedding2D, ApplyVisionRoPE2D and MRoPE(Inplace).  Each `forward` validates the reference's contract, hands raw
device pointers to the C ABI and returns torch tensors; there is no torch compute in here."""
from typing import Optional

import torch

from ....core.operators.activation import MojoGelu, MojoSilu, MojoSwiGLU
from ....core.operators.kv_cache import (MojoStorePagedKVCache, MojoStorePagedMLAKVCache,
                                           assert_paged_kv_layout_contract)
from ....core.operators.normalization import (MojoLayerNorm, MojoResidualAddLayerNorm, MojoResidualAddRMSNorm, MojoRMSNorm,
                                                MojoRMSNormInplace)
from ....core.operators.position_embedding import (MojoApplyRoPE, MojoApplyVisionRoPE2D, MojoGridRoPE, MojoMRoPE,
                                                     MojoMRoPEInplace, MojoRotaryEmbedding, MojoVisionRotaryEmbedding2D,
                                                     check_mrope_contract)
from .. import lib as L

_ROCM = ["rocm"]


def _dense(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous() else t.contiguous()


def _row_view(t: torch.Tensor):
    """(rows, row stride in elements) when ``t`` is a stack of rows with one uniform row stride and a dense last dimension
    (a column slice of a dense [.., N] tensor); None otherwise."""
    if t.dim() == 0 or t.stride(-1) != 1 or t.numel() == 0:
        return None
    cols = t.shape[-1]
    if t.dim() == 1:
        return 1, cols
    ld = t.stride(-2)
    rows, expect = 1, ld
    for size, stride in zip(reversed(t.shape[:-1]), reversed(t.stride()[:-1])):
        if size != 1 and stride != expect:
            return None
        expect *= size
        rows *= size
    return rows, ld


class HIPSwiGLU(MojoSwiGLU):
    supported_platforms_list = _ROCM

    def forward(self, gate_out: torch.Tensor, up_out: torch.Tensor) -> torch.Tensor:
        L.require_cuda(gate_out, up_out)
        if gate_out.shape != up_out.shape or gate_out.dtype != up_out.dtype:
            raise NotImplementedError("HIPSwiGLU: gate_out and up_out must have identical shape and dtype")
        if gate_out.is_contiguous() and up_out.is_contiguous():
            g, u = gate_out, up_out
            out = torch.empty_like(g)
            L.check(L.load().mojo_hip_swiglu(L.ptr(g), L.ptr(u), L.ptr(out), g.numel(), L.dtype_code(g.dtype),
                                             float(self.swiglu_limit), L.stream_of(g)), "HIPSwiGLU")
            return out
        # Row-strided views — the two halves of a fused [.., 2 * inter] projection (`gate, up = gu.chunk(2, -1)`) — are read in
        # place: no copy of either half.  Anything else is made dense first.
        rows_g, rows_u = _row_view(gate_out), _row_view(up_out)
        if rows_g is None or rows_u is None or (rows_g[1] * gate_out.element_size()) % 16 or (rows_u[1] * up_out.element_size()) % 16 \
                or gate_out.data_ptr() % 16 or up_out.data_ptr() % 16:
            return self.forward(_dense(gate_out), _dense(up_out))
        cols = gate_out.shape[-1]
        out = torch.empty(gate_out.shape, dtype=gate_out.dtype, device=gate_out.device)
        L.check(L.load().mojo_hip_swiglu_rows(L.ptr(gate_out), L.ptr(up_out), L.ptr(out), rows_g[0], cols, rows_g[1], rows_u[1], cols,
                                              L.dtype_code(gate_out.dtype), float(self.swiglu_limit), L.stream_of(gate_out)), "HIPSwiGLU")
        return out


def _rmsnorm(hidden, residual, weight, eps, want_sum, out=None):
    L.require_cuda(hidden, residual, weight)
    if weight.dtype != hidden.dtype or (residual is not None and residual.dtype != hidden.dtype):
        raise NotImplementedError("hip rmsnorm: hidden, residual and weight must share one dtype")
    if residual is not None and residual.shape != hidden.shape:
        raise NotImplementedError("hip rmsnorm: hidden and residual must have identical shapes")
    dim = hidden.shape[-1]
    assert weight.shape == (dim,), f"weight shape {tuple(weight.shape)} does not match hidden size {dim}"
    h = _dense(hidden)
    r = None if residual is None else _dense(residual)
    normed = torch.empty_like(h) if out is None else out
    summed = torch.empty_like(h) if want_sum else None
    rows = h.numel() // dim if dim else 0
    L.check(L.load().mojo_hip_residual_add_rmsnorm(L.ptr(h), L.ptr(r), L.ptr(_dense(weight.detach())), L.ptr(normed),
                                                   L.ptr(summed), rows, dim, L.dtype_code(h.dtype), float(eps),
                                                   L.stream_of(h)), "hip rmsnorm")
    return normed, summed


class HIPRMSNorm(MojoRMSNorm):
    supported_platforms_list = _ROCM

    def forward(self, hidden_state: torch.Tensor) -> torch.Tensor:
        return _rmsnorm(hidden_state, None, self.weight, self.variance_epsilon, False)[0]


class HIPRMSNormInplace(MojoRMSNormInplace):
    """``inplace=True``: the kernel's output pointer IS the input (each thread reads its elements of a row before the
    row's reduction and writes the same elements after it, so no element is read after it was overwritten)."""

    supported_platforms_list = _ROCM

    def forward(self, hidden_state: torch.Tensor) -> torch.Tensor:
        if not self.inplace:
            return _rmsnorm(hidden_state, None, self.weight, self.variance_epsilon, False)[0]
        if hidden_state.is_contiguous():
            _rmsnorm(hidden_state, None, self.weight, self.variance_epsilon, False, out=hidden_state)
        else:                                # a strided view (e.g. the q slice of a fused qkv): normalise a dense copy, write back
            hidden_state.copy_(_rmsnorm(hidden_state, None, self.weight, self.variance_epsilon, False)[0])
        return hidden_state


class HIPResidualAddRMSNorm(MojoResidualAddRMSNorm):
    supported_platforms_list = _ROCM

    def forward(self, hidden_state: torch.Tensor, residual: torch.Tensor):
        pre = self.norm_pos == "pre"
        normed, summed = _rmsnorm(hidden_state, residual, self.weight, self.variance_epsilon, pre)
        return (normed, summed) if pre else (normed, normed)


_FLOATS = (torch.float32, torch.float16, torch.bfloat16)


def _require_float(what: str, t: torch.Tensor) -> None:
    """fp32 / fp16 / bf16 or a refusal that names the dtype: an integer tensor (or fp64) is never cast behind the caller's back."""
    if not t.is_floating_point():
        raise NotImplementedError(f"{what}: integer input of dtype {t.dtype}; the op is defined on floating-point tensors")
    if t.dtype not in _FLOATS:
        raise NotImplementedError(f"{what}: dtype {t.dtype} is not supported (fp32, fp16, bf16)")


def _layernorm(what, hidden, residual, weight, bias, eps, want_sum):
    """(normed, sum or None).  ``hidden`` / ``residual`` whose last dimension is dense and whose leading dimensions collapse to
    one row stride (a column slice of a wider tensor) are read in place; anything else is made dense first."""
    _require_float(what, hidden)
    dim = hidden.shape[-1] if hidden.dim() else 0
    if hidden.dim() == 0:
        raise ValueError(f"{what}: hidden_state needs a last dimension to normalise over")
    if residual is not None and (residual.dtype != hidden.dtype or residual.shape != hidden.shape):
        raise NotImplementedError(f"{what}: hidden_state and residual must share one shape and dtype")
    if (weight is None) != (bias is None):
        raise NotImplementedError(f"{what}: weight and bias come together or not at all")
    if weight is not None:
        if weight.dtype != hidden.dtype or bias.dtype != hidden.dtype:
            raise NotImplementedError(f"{what}: weight and bias ({weight.dtype}, {bias.dtype}) must have the activation dtype {hidden.dtype}")
        if tuple(weight.shape) != (dim,) or tuple(bias.shape) != (dim,):
            raise ValueError(f"{what}: weight length {tuple(weight.shape)} / bias length {tuple(bias.shape)} do not match the hidden size {dim}")
    L.require_cuda(hidden, residual, weight, bias)
    normed = torch.empty(hidden.shape, dtype=hidden.dtype, device=hidden.device)
    summed = torch.empty_like(normed) if want_sum else None
    if hidden.numel() == 0:                                   # rows == 0 (or dim == 0): nothing to launch
        return normed, summed
    rows_h = _row_view(hidden)
    if rows_h is None or rows_h[1] < dim:                     # (a row stride below dim: an expanded tensor)
        hidden = hidden.contiguous()
        rows_h = _row_view(hidden)
    rows_r = None
    if residual is not None:
        rows_r = _row_view(residual)
        if rows_r is None or rows_r[1] < dim:
            residual = residual.contiguous()
            rows_r = _row_view(residual)
    w = None if weight is None else _dense(weight.detach())
    b = None if bias is None else _dense(bias.detach())
    L.check(L.load().mojo_hip_layernorm(L.ptr(hidden), L.ptr(residual), L.ptr(w), L.ptr(b), L.ptr(normed), L.ptr(summed), rows_h[0], dim,
                                        rows_h[1], rows_r[1] if rows_r else 0, L.dtype_code(hidden.dtype), float(eps),
                                        L.stream_of(hidden)), what)
    return normed, summed


class HIPLayerNorm(MojoLayerNorm):
    supported_platforms_list = _ROCM

    def forward(self, hidden_state: torch.Tensor) -> torch.Tensor:
        return _layernorm("HIPLayerNorm", hidden_state, None, self.weight, self.bias, self.variance_epsilon, False)[0]


class HIPResidualAddLayerNorm(MojoResidualAddLayerNorm):
    supported_platforms_list = _ROCM

    def forward(self, hidden_state: torch.Tensor, residual: torch.Tensor):
        pre = self.norm_pos == "pre"
        normed, summed = _layernorm("HIPResidualAddLayerNorm", hidden_state, residual, self.weight, self.bias, self.variance_epsilon, pre)
        return (normed, summed) if pre else (normed, normed)


ACT_GELU_ERF, ACT_SILU = 0, 1                 # `kind` of mojo_hip_activation


def _activation(what, x, kind, out=None):
    """``out`` (dense, the shape and dtype of ``x``) may be ``x`` itself.  A non-contiguous ``x`` is copied once, to a dense
    tensor, before the kernel reads it: an elementwise pass has no stride pattern worth a kernel form of its own."""
    _require_float(what, x)
    L.require_cuda(x, out)
    if out is None:
        x = _dense(x)
        out = torch.empty_like(x)
    elif not (x.is_contiguous() and out.is_contiguous() and out.shape == x.shape and out.dtype == x.dtype):
        raise NotImplementedError(f"{what}: an explicit output needs dense x and out of one shape and dtype")
    if x.numel():
        L.check(L.load().mojo_hip_activation(L.ptr(x), L.ptr(out), x.numel(), kind, L.dtype_code(x.dtype), L.stream_of(x)), what)
    return out


class HIPGelu(MojoGelu):
    """The erf form.  A non-contiguous input is copied once in Python (`_activation`)."""

    supported_platforms_list = _ROCM

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _activation("HIPGelu", x, ACT_GELU_ERF)


class HIPSilu(MojoSilu):
    """A non-contiguous input is copied once in Python (`_activation`)."""

    supported_platforms_list = _ROCM

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _activation("HIPSilu", x, ACT_SILU)


class HIPGridRoPE(MojoGridRoPE):
    """``x`` is read in place through its strides (the last dimension dense, the others even: a slice of a fused QKV buffer
    is), the complex64 frequencies through ``view_as_real`` without a copy.  ``freqs_list`` entries that are all one tensor
    are passed as one pointer; distinct entries are packed into one buffer per call.

    ``grid_sizes`` on the CPU is checked here (a grid with more cells than ``L`` or than its frequency entry has rows raises,
    as the golden's reshape and broadcast do) and copied to the device; ``grid_sizes`` on the device is read by the kernel,
    with no host synchronisation, and then a grid larger than its entry is the caller's error: the kernel rotates the tokens
    the entry has rows for, copies the rest, and never reads past an entry."""

    supported_platforms_list = _ROCM

    def forward(self, x: torch.Tensor, grid_sizes: torch.Tensor, freqs_list):
        self.check_shape_contract(x, grid_sizes, freqs_list)
        _require_float("HIPGridRoPE", x)
        if grid_sizes.is_floating_point() or grid_sizes.dtype == torch.bool:
            raise NotImplementedError(f"HIPGridRoPE: grid_sizes must be an integer tensor, got {grid_sizes.dtype}")
        batch, tokens, heads, dim = x.shape
        half = dim // 2
        freqs = list(freqs_list[:batch])
        rows = []
        for i, f in enumerate(freqs):
            if f.dtype != torch.complex64:
                raise NotImplementedError(f"HIPGridRoPE: freqs_list[{i}] is {f.dtype}; the frequencies must be complex64")
            if half and (f.dim() == 0 or f.shape[-1] != half or f.numel() % half or f.numel() // half != f.shape[0]):
                raise ValueError(f"HIPGridRoPE: freqs_list[{i}] of shape {tuple(f.shape)} is not [seq_len, 1, {half}]")
            rows.append(f.shape[0] if f.dim() else 0)
        if not grid_sizes.is_cuda:
            for i, (gf, gh, gw) in enumerate(grid_sizes.tolist()):
                cells = gf * gh * gw
                if cells > tokens or cells > rows[i]:
                    raise ValueError(f"HIPGridRoPE: grid {(gf, gh, gw)} of sample {i} has {cells} cells, more than the {tokens} tokens "
                                     f"of x or the {rows[i]} rows of freqs_list[{i}]")
        L.require_cuda(x, *freqs)
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        if x.numel() == 0:
            return out
        elt_pair = 2 * x.element_size()
        if x.stride(-1) != 1 or any(st % 2 for st in x.stride()[:3]) or x.data_ptr() % elt_pair:
            x = x.contiguous()
        grid = grid_sizes if grid_sizes.dtype in (torch.int32, torch.int64) else grid_sizes.to(torch.int64)
        grid = _dense(grid.to(x.device))
        first = freqs[0]
        if all(f is first or (f.data_ptr() == first.data_ptr() and f.shape == first.shape and f.stride() == first.stride()) for f in freqs):
            table, shared_rows = None, rows[0]
            packed = torch.view_as_real(_dense(first))
        else:
            starts = [sum(rows[:i]) for i in range(batch)]
            table = torch.tensor([[s0, r] for s0, r in zip(starts, rows)], dtype=torch.int64).to(x.device)
            shared_rows = 0
            packed = torch.cat([torch.view_as_real(_dense(f)).reshape(r, dim) for f, r in zip(freqs, rows)])
        L.check(L.load().mojo_hip_grid_rope(L.ptr(x), L.ptr(out), L.ptr(packed), L.ptr(grid), int(grid.dtype == torch.int64), L.ptr(table),
                                            shared_rows, batch, tokens, heads, dim, L.strides3(*x.stride()[:3]), L.dtype_code(x.dtype),
                                            L.stream_of(x)), "HIPGridRoPE")
        return out


class HIPApplyRoPE(MojoApplyRoPE):
    supported_platforms_list = _ROCM

    @staticmethod
    def _btn_strides(t: torch.Tensor, head_first: bool):
        """(batch, token, head) strides of a 3-D/4-D q or k in the caller's layout."""
        s = t.stride()
        if t.ndim == 3:
            return (0, s[1], s[0]) if head_first else (0, s[0], s[1])
        return (s[0], s[2], s[1]) if head_first else (s[0], s[1], s[2])

    def forward(self, q, k, cos, sin, head_first: bool = True):
        self.check_shape_contract(q, k, cos, sin)
        L.require_cuda(q, k, cos, sin)
        if q.dtype != k.dtype:
            raise NotImplementedError("HIPApplyRoPE: q and k must share one dtype")
        if q.stride(-1) != 1:
            q = q.contiguous()
        if k.stride(-1) != 1:
            k = k.contiguous()
        cos = _dense(cos.float())
        sin = _dense(sin.float())
        head_axis, tok_axis = (-3, -2) if head_first else (-2, -3)
        batch = q.shape[0] if q.ndim == 4 else 1
        tokens = q.shape[tok_axis]
        assert k.shape[tok_axis] == tokens and k.shape[-1] == q.shape[-1] and (k.ndim == 3 or k.shape[0] == batch)
        rope_dim = cos.shape[-1]
        assert cos.shape[-2] == tokens, "cos/sin rows must match the token dimension of q/k"
        if cos.ndim == 3:
            assert q.ndim == 4 and cos.shape[0] == batch
            cos_b, cos_t = cos.stride(0), cos.stride(1)
        else:
            cos_b, cos_t = 0, cos.stride(0)
        q_out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        k_out = torch.empty(k.shape, dtype=k.dtype, device=k.device)
        L.check(L.load().mojo_hip_apply_rope(
            L.ptr(q), L.ptr(k), L.ptr(q_out), L.ptr(k_out), L.ptr(cos), L.ptr(sin),
            batch, tokens, q.shape[head_axis], k.shape[head_axis], q.shape[-1], rope_dim,
            L.strides3(*self._btn_strides(q, head_first)), L.strides3(*self._btn_strides(k, head_first)),
            L.strides3(*self._btn_strides(q_out, head_first)), L.strides3(*self._btn_strides(k_out, head_first)),
            cos_b, cos_t, L.dtype_code(q.dtype), L.stream_of(q)), "HIPApplyRoPE")
        return q_out, k_out


class HIPRotaryEmbedding(MojoRotaryEmbedding):
    supported_platforms_list = _ROCM

    def forward(self, x, cu_q_lens=None, total_seq_lens=None, position_ids=None):
        self.check_index_contract(x, cu_q_lens, total_seq_lens, position_ids)
        L.require_cuda(x, cu_q_lens, total_seq_lens, position_ids)
        dev = x.device
        d = 2 * self.inv_freq.shape[0]            # rope_dim (the reference's class keeps only inv_freq)
        batch = 0
        if cu_q_lens is not None:
            mode, lead = 2, (x.shape[0],)
            batch = cu_q_lens.shape[0] - 1
            cu_q_lens = _dense(cu_q_lens)
            total_seq_lens = None if total_seq_lens is None else _dense(total_seq_lens)
        elif position_ids is not None:
            mode, lead = 0, tuple(position_ids.shape)
            position_ids = _dense(position_ids)
        else:
            mode, lead = 1, (x.shape[1],)
        n_pos = 1
        for s in lead:
            n_pos *= s
        cos = torch.empty(*lead, d, dtype=torch.float32, device=dev)
        sin = torch.empty_like(cos)
        if mode == 2 and batch == 0:
            mode, position_ids = 0, torch.full(lead, -1, dtype=torch.int32, device=dev)
        cached = self.init_max_length is not None
        inv_freq = _dense(self.inv_freq.to(dev))
        L.check(L.load().mojo_hip_rotary_embedding(
            L.ptr(cos), L.ptr(sin), n_pos, d, mode, L.ptr(position_ids), L.ptr(cu_q_lens), L.ptr(total_seq_lens),
            batch, L.ptr(self.cos.to(dev)) if cached else None, L.ptr(self.sin.to(dev)) if cached else None,
            self.init_max_length if cached else 0, L.ptr(inv_freq), float(self.attention_scaling),
            L.stream_of(cos)), "HIPRotaryEmbedding")
        return cos, sin


class HIPStorePagedKVCache(MojoStorePagedKVCache):
    supported_platforms_list = _ROCM

    def forward(self, key_states, value_states, key_cache, value_cache, block_table: Optional[torch.Tensor] = None,
                cu_q_lens: Optional[torch.Tensor] = None, context_kv_lens: Optional[torch.Tensor] = None, *,
                chunk_metadata: Optional[torch.Tensor] = None):
        self.check_call_contract(key_states, value_states, block_table, cu_q_lens, context_kv_lens, chunk_metadata)
        L.require_cuda(key_states, value_states, key_cache, value_cache, block_table, cu_q_lens, context_kv_lens,
                       chunk_metadata)
        assert key_cache.shape == value_cache.shape and key_cache.dim() == 4
        assert key_cache.dtype == key_states.dtype == value_states.dtype == value_cache.dtype
        n_blocks, heads, page, dim = key_cache.shape
        tokens = key_states.shape[0]
        assert key_states.shape[1:] == (heads, dim), "key/value states do not match the cache's (heads, head_dim)"
        if key_cache.stride(-1) != 1 or value_cache.stride(-1) != 1 or key_cache.stride() != value_cache.stride():
            raise NotImplementedError("HIPStorePagedKVCache: caches must share strides and be dense in head_dim")
        if key_states.stride(-1) != 1 or key_states.stride() != value_states.stride():
            key_states, value_states = key_states.contiguous(), value_states.contiguous()
        eb = key_cache.element_size()
        common = (tokens, heads, dim, n_blocks, page, eb, key_states.stride(0), key_states.stride(1),
                  key_cache.stride(0), key_cache.stride(1), key_cache.stride(2), L.stream_of(key_cache))
        lib = L.load()
        if chunk_metadata is not None:
            plan = _dense(chunk_metadata)
            L.check(lib.mojo_hip_store_paged_kv_plan(L.ptr(key_states), L.ptr(value_states), L.ptr(key_cache),
                                                     L.ptr(value_cache), L.ptr(plan), plan.shape[0], *common),
                    "HIPStorePagedKVCache")
        else:
            assert_paged_kv_layout_contract(block_table, cu_q_lens, context_kv_lens)
            batch = context_kv_lens.shape[0]
            if cu_q_lens is not None:
                assert cu_q_lens.shape[0] == batch + 1
            table = block_table if block_table.stride(1) == 1 else block_table.contiguous()
            L.check(lib.mojo_hip_store_paged_kv_layout(
                L.ptr(key_states), L.ptr(value_states), L.ptr(key_cache), L.ptr(value_cache), L.ptr(table),
                table.stride(0), table.shape[1], L.ptr(None if cu_q_lens is None else _dense(cu_q_lens)),
                L.ptr(_dense(context_kv_lens)), batch, *common), "HIPStorePagedKVCache")
        return key_cache, value_cache


class HIPStorePagedMLAKVCache(MojoStorePagedMLAKVCache):
    supported_platforms_list = _ROCM

    def forward(self, compressed_kv_states, k_pe_states, compressed_kv_cache, k_pe_cache, block_table, cu_q_lens,
                context_kv_lens):
        assert_paged_kv_layout_contract(block_table, cu_q_lens, context_kv_lens)
        L.require_cuda(compressed_kv_states, k_pe_states, compressed_kv_cache, k_pe_cache, block_table, cu_q_lens,
                       context_kv_lens)
        if context_kv_lens is None:
            return compressed_kv_cache, k_pe_cache
        assert compressed_kv_cache.dim() == 4 and k_pe_cache.dim() == 4 and compressed_kv_cache.shape[1] == 1
        assert compressed_kv_cache.shape[:3] == k_pe_cache.shape[:3]
        n_blocks, _, page, r = compressed_kv_cache.shape
        rope = k_pe_cache.shape[3]
        assert compressed_kv_states.dim() == 2 and compressed_kv_states.shape[1] == r
        assert k_pe_states.dim() == 2 and k_pe_states.shape[1] == rope
        assert compressed_kv_states.shape[0] == k_pe_states.shape[0]
        dt = compressed_kv_cache.dtype
        if not (dt == k_pe_cache.dtype == compressed_kv_states.dtype == k_pe_states.dtype):
            raise NotImplementedError("HIPStorePagedMLAKVCache: states and caches must share one dtype")
        if compressed_kv_cache.stride(3) != 1 or k_pe_cache.stride(3) != 1:
            raise NotImplementedError("HIPStorePagedMLAKVCache: caches must be dense in their last dimension")
        ckv = compressed_kv_states if compressed_kv_states.stride(1) == 1 else compressed_kv_states.contiguous()
        kpe = k_pe_states if k_pe_states.stride(1) == 1 else k_pe_states.contiguous()
        batch = context_kv_lens.shape[0]
        if cu_q_lens is not None:
            assert cu_q_lens.shape[0] == batch + 1
        table = block_table if block_table.stride(1) == 1 else block_table.contiguous()
        L.check(L.load().mojo_hip_store_paged_mla_kv(
            L.ptr(ckv), L.ptr(kpe), L.ptr(compressed_kv_cache), L.ptr(k_pe_cache), L.ptr(table), table.stride(0),
            table.shape[1], L.ptr(None if cu_q_lens is None else _dense(cu_q_lens)), L.ptr(_dense(context_kv_lens)), batch,
            ckv.shape[0], r, rope, n_blocks, page, dt.itemsize, ckv.stride(0), kpe.stride(0),
            compressed_kv_cache.stride(0), compressed_kv_cache.stride(2), k_pe_cache.stride(0), k_pe_cache.stride(2),
            L.stream_of(compressed_kv_cache)), "HIPStorePagedMLAKVCache")
        return compressed_kv_cache, k_pe_cache


class HIPVisionRotaryEmbedding2D(MojoVisionRotaryEmbedding2D):
    """One launch computes every token's ``(h, w)`` position under the adapooling regrouping from its index and writes its
    ``(cos, sin)`` row, where the reference loops over the samples on the host and gathers from a
    ``max_grid x rope_dim / 4`` table.  The angle is the fp32 product ``pos * inv_freq[i]``, rounded once as the golden's
    ``outer`` rounds it; cos and sin are the device's ``cosf`` / ``sinf``.

    Not capture-safe: the output size ``sum(h * w)`` is a host quantity, so ``grid_hw`` is read on the host once (the
    reference's contract contains the same read).  The outputs live on the device of ``inv_freq``."""
    supported_platforms_list = _ROCM

    def forward(self, grid_hw: torch.Tensor):
        grids = self.check_grid_contract(grid_hw, self.adapooling_factor)
        L.require_cuda(self.inv_freq)
        dev = self.inv_freq.device
        firsts, total = [], 0
        for gh, gw in grids:
            firsts.append(total)
            total += gh * gw
        cos = torch.empty(total, self.rope_dim, dtype=torch.float32, device=dev)
        sin = torch.empty_like(cos)
        if total == 0:
            return cos, sin
        samples = torch.tensor([[f, gh, gw] for f, (gh, gw) in zip(firsts, grids)], dtype=torch.int64).to(dev)
        inv_freq = _dense(self.inv_freq.float())
        L.check(L.load().mojo_hip_vision_rotary_2d(L.ptr(cos), L.ptr(sin), L.ptr(samples), len(grids), total, self.rope_dim,
                                                   self.adapooling_factor, L.ptr(inv_freq), L.stream_of(cos)),
                "HIPVisionRotaryEmbedding2D")
        return cos, sin


class HIPApplyVisionRoPE2D(MojoApplyVisionRoPE2D):
    """`mojo_hip_apply_rope` with ``rope_dim = head_dim`` on token-first tensors: its two rounded fp32 products and rounded sum
    are the golden's ``x * cos + rotate_half(x) * sin`` bit for bit, so this op is a host path over that
    kernel.  q and k are read in place through their token and head strides (the last dimension dense: slices of a fused
    ``[T, 3, N, D]`` projection qualify); the vector width follows ``D / 2``, the strides and the base alignment (16-, 8-,
    4-byte or element loads).  fp32 tables are read in place; a 16-bit table is widened to fp32 first — the golden's own
    promotion, exact — as one pass over ``[T, D]``."""
    supported_platforms_list = _ROCM

    def forward(self, q, k, cos, sin):
        self.check_shape_contract(q, k, cos, sin)
        L.require_cuda(q, k, cos, sin)
        if q.dtype != k.dtype:
            raise NotImplementedError("HIPApplyVisionRoPE2D: q and k must share one dtype")
        _require_float("HIPApplyVisionRoPE2D", q)
        if q.shape[-1] % 2:
            raise ValueError(f"HIPApplyVisionRoPE2D: head_dim {q.shape[-1]} must be even")
        if q.stride(-1) != 1:
            q = q.contiguous()
        if k.stride(-1) != 1:
            k = k.contiguous()
        cos, sin = _dense(cos.float()), _dense(sin.float())
        tokens, dim = q.shape[0], q.shape[-1]
        q_out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        k_out = torch.empty(k.shape, dtype=k.dtype, device=k.device)
        L.check(L.load().mojo_hip_apply_rope(
            L.ptr(q), L.ptr(k), L.ptr(q_out), L.ptr(k_out), L.ptr(cos), L.ptr(sin), 1, tokens, q.shape[1], k.shape[1], dim, dim,
            L.strides3(0, q.stride(0), q.stride(1)), L.strides3(0, k.stride(0), k.stride(1)),
            L.strides3(0, q_out.stride(0), q_out.stride(1)), L.strides3(0, k_out.stride(0), k_out.stride(1)),
            0, cos.stride(0), L.dtype_code(q.dtype), L.stream_of(q)), "HIPApplyVisionRoPE2D")
        return q_out, k_out


def _mrope(what, query, key, cos_table, sin_table, mrope_section, is_interleaved, head_dim, inplace):
    """The host path of both MRoPE classes: validation, then one launch over q and k.  Rows are addressed by their stride
    (the last dimension dense), so slices of a fused QKV row are read — and, in place, written — where they are."""
    head_dim, half, hq, hk = check_mrope_contract(query, key, cos_table, sin_table, mrope_section, head_dim)
    L.require_cuda(query, key, cos_table, sin_table)
    if query.dtype != key.dtype:
        raise NotImplementedError(f"{what}: query and key must share one dtype")
    _require_float(what, query)
    _require_float(what, cos_table)
    tokens = query.shape[0]
    q_in, k_in = query, key
    if inplace:
        for name, t in (("query", query), ("key", key)):
            if t.numel() and t.stride(-1) != 1:
                raise NotImplementedError(f"{what}: the in-place form needs a dense last dimension of {name}")
        q_out, k_out = query, key
    else:
        q_in = query if query.stride(-1) == 1 else query.contiguous()
        k_in = key if key.stride(-1) == 1 else key.contiguous()
        q_out = torch.empty(query.shape, dtype=query.dtype, device=query.device)
        k_out = torch.empty(key.shape, dtype=key.dtype, device=key.device)
    if tokens == 0:
        return q_out, k_out
    cos, sin = cos_table, sin_table
    if cos.stride(-1) != 1 or cos.stride() != sin.stride():
        cos, sin = cos.contiguous(), sin.contiguous()
    sec_stride, tok_stride = (cos.stride(0), cos.stride(1)) if cos.dim() == 3 else (0, cos.stride(0))
    L.check(L.load().mojo_hip_mrope(
        L.ptr(q_in), L.ptr(k_in), L.ptr(q_out), L.ptr(k_out), L.ptr(cos), L.ptr(sin), tokens, hq, hk, head_dim,
        q_in.stride(0), k_in.stride(0), q_out.stride(0), k_out.stride(0), sec_stride, tok_stride,
        L.strides3(*[int(s) for s in mrope_section]), 1 if is_interleaved else 0, L.dtype_code(cos.dtype),
        L.dtype_code(query.dtype), L.stream_of(query)), what)
    return q_out, k_out


class HIPMRoPE(MojoMRoPE):
    """Multimodal RoPE, out of place: one launch over q and k; for ``[3, T, half]`` tables the kernel picks the
    table per element and never materialises a merged one.  Math in fp32 — each product rounded, no contraction — and one
    rounding to the storage type.

    The result has the QUERY's dtype.  The reference's out-of-place golden returns fp32 when the tables are fp32 (torch's
    promotion inside ``cat``); this op returns that fp32 result rounded once to the query's dtype, which is bit for bit what
    `MojoMRoPEInplace(inplace=True)` stores.  16-bit tables are converted on read and computed in fp32 (the golden computes in
    the 16-bit type there and rounds three times).  No host sync, capture-safe."""
    supported_platforms_list = _ROCM

    def forward(self, query, key, cos_table, sin_table, mrope_section, is_interleaved: bool = False,
                head_dim: Optional[int] = None):
        return _mrope("HIPMRoPE", query, key, cos_table, sin_table, mrope_section, is_interleaved, head_dim, False)


class HIPMRoPEInplace(MojoMRoPEInplace):
    """Multimodal RoPE in its serving form: with ``inplace=True`` the rotated elements are written back into
    ``query`` and ``key`` (slices of a fused QKV row are written where they are; elements at or past ``2 * sum(mrope_section)``
    are not touched) and the inputs are returned; bit for bit the golden with fp32 tables.  ``inplace=False`` is `HIPMRoPE`."""
    supported_platforms_list = _ROCM

    def forward(self, query, key, cos_table, sin_table, mrope_section, is_interleaved: bool = False,
                head_dim: Optional[int] = None):
        return _mrope("HIPMRoPEInplace", query, key, cos_table, sin_table, mrope_section, is_interleaved, head_dim,
                      bool(self.inplace))
