"""API classes `MojoRotaryEmbedding` / `MojoApplyRoPE`.

Follows `mojo_opset/core/operators/position_embedding.py:9-175`.  ``inv_freq`` and the optional
``cos``/``sin`` cache are non-persistent buffers with the reference's names, computed in fp32.
The tables are computed once on the host and then moved to the factory device, so the cached
gather path is bit-identical to the CPU golden regardless of the device's libm.  `MojoGridRoPE` (``DIT_BLOCK_OPS``) follows
`mojo_opset/experimental/operators/position_embedding.py:80-118`.
"""
from typing import Optional

import torch

from ..operator import MojoOperator


def rope_inv_freq(rope_theta, rope_dim: int) -> torch.Tensor:
    """``1 / theta ** (arange(0, d, 2) / d)`` in fp32 (reference :13-15)."""
    return 1.0 / (rope_theta ** (torch.arange(0, rope_dim, 2, dtype=torch.float32) / rope_dim))


def rope_table(inv_freq: torch.Tensor, max_length: int, attention_scaling: float):
    """fp32 ``cos, sin [max_length, rope_dim]`` = f(cat(freqs, freqs)) * scaling (reference :33-41)."""
    pos = torch.arange(max_length)
    freqs = pos[..., None] * inv_freq[None, :]
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos() * attention_scaling, emb.sin() * attention_scaling


class MojoRotaryEmbedding(MojoOperator):
    """forward(x, cu_q_lens=None, total_seq_lens=None, position_ids=None) -> (cos, sin) fp32.

    1. var-len prefill: ``x [T, H]`` + ``cu_q_lens [B+1]`` (+ ``total_seq_lens [B]``) -> ``[T, d]``
    2. padded prefill:  ``x [B, S, H]`` and nothing else                              -> ``[S, d]``
    3. decode / explicit: ``position_ids`` shaped like ``x.shape[:-1]``                -> ``[..., d]``
    """

    def __init__(self, rope_theta, rope_dim, attention_scaling: float = 1.0,
                 init_max_length: Optional[int] = None, **kwargs):
        super().__init__(**kwargs)
        device = self.tensor_factory_kwargs.get("device")
        self.rope_theta = rope_theta
        self.rope_dim = rope_dim
        self.attention_scaling = attention_scaling
        self.init_max_length = None
        self.register_buffer("inv_freq", rope_inv_freq(rope_theta, rope_dim).to(device), persistent=False)
        if init_max_length is not None:
            self._rope_init(init_max_length)

        def _ignore_rope_buffers(module, incompatible_keys) -> None:
            missing = incompatible_keys.missing_keys
            missing[:] = [k for k in missing if k.split(".")[-1] not in ("inv_freq", "cos", "sin")]

        self.register_load_state_dict_post_hook(_ignore_rope_buffers)

    def _rope_init(self, max_length: int) -> None:
        device = self.tensor_factory_kwargs.get("device")
        self.init_max_length = max_length
        cos, sin = rope_table(self.inv_freq.detach().cpu(), max_length, self.attention_scaling)
        self.register_buffer("cos", cos.to(device), persistent=False)
        self.register_buffer("sin", sin.to(device), persistent=False)

    @staticmethod
    def check_index_contract(x, cu_q_lens, total_seq_lens, position_ids) -> None:
        """int32 index tensors; at most one of ``cu_q_lens`` / ``position_ids`` (reference :59-65,:82)."""
        for t in (cu_q_lens, total_seq_lens, position_ids):
            if t is not None:
                assert t.dtype == torch.int32
        assert position_ids is None or cu_q_lens is None, "At most one of cu_q_lens or position_ids should be provided"
        if cu_q_lens is not None:
            assert x.dim() == 2, "x must be 2D: [T, D]"
        elif position_ids is not None:
            assert position_ids.shape == x.shape[:-1], (
                "position_ids must have the same shape as x except the hidden dimension"
            )


class MojoApplyRoPE(MojoOperator):
    """forward(q, k, cos, sin, head_first=True) -> (q_rot, k_rot), rotate-half on the last
    ``cos.shape[-1]`` features of every head; the leading features pass through."""

    def __init__(self, interleaved: bool = False):
        super().__init__()
        assert not interleaved, "interleaved impl is not supported yet."
        self.interleaved = interleaved

    @staticmethod
    def check_shape_contract(q, k, cos, sin) -> None:
        assert q.ndim == k.ndim, "q and k must have the same dimension"
        assert q.ndim == 3 or q.ndim == 4, "q and k must be 3D or 4D"
        assert cos.shape == sin.shape, "cos and sin must have the same shape"
        if q.ndim == 3:
            assert cos.ndim == 2, (
                "rotary position embedding (cos/sin) must be of shape [num_tokens, rope_dim] "
                "for varlen prefill or decode"
            )

    def extra_repr(self) -> str:
        return f"interleaved={self.interleaved!r}"


class MojoGridRoPE(MojoOperator):
    """forward(x [B, L, N, D], grid_sizes [B, 3], freqs_list) -> x with the first ``F_i * H_i * W_i`` tokens of sample ``i``
    rotated pair by pair, ``(x[2j] + i x[2j+1]) * freqs_list[i][t, 0, j]``, and the padding tokens behind them unchanged.
    ``freqs_list[i]`` is a complex64 ``[F_i * H_i * W_i, 1, D / 2]`` of unit phases; D is even."""

    def __init__(self):
        super().__init__()

    @staticmethod
    def check_shape_contract(x, grid_sizes, freqs_list) -> None:
        assert x.dim() == 4, "x must be 4D: [B, L, N, D]"
        assert x.size(-1) % 2 == 0, "D must be even for complex pairing"
        assert grid_sizes.dim() == 2 and grid_sizes.size(1) == 3, "grid_sizes must be [B, 3]"
        assert grid_sizes.size(0) == x.size(0) and len(freqs_list) >= x.size(0), "one grid and one frequency tensor per sample"


class MojoVisionRotaryEmbedding2D(MojoOperator):
    """forward(grid_hw [B, 2] int) -> (cos, sin) fp32 ``[sum(h * w), rope_dim]``: the 2-D rotary table of a vision tower.

    Sample ``b`` is a grid of ``(h, w)`` patches in the adapooling order: the grid is cut into ``f x f`` windows
    (``f = adapooling_factor``), the windows are walked row-major and the patches of a window row-major inside it.  A row is
    ``[h * inv_freq | w * inv_freq]`` twice, ``inv_freq = 1 / theta ** (arange(0, rope_dim / 2, 2) / (rope_dim / 2))``.
    The output size is a host quantity: ``grid_hw`` is read on the host (reference
    `mojo_opset/core/operators/position_embedding.py:281-363`)."""

    def __init__(self, rope_theta: float = 10000.0, rope_dim: int = 64, adapooling_factor: int = 1, **kwargs):
        super().__init__(**kwargs)
        assert adapooling_factor >= 1, "adapooling_factor must be >= 1"
        assert rope_dim % 4 == 0, "vision 2D rope_dim must be divisible by 4"
        self.rope_theta = rope_theta
        self.rope_dim = rope_dim
        self.adapooling_factor = adapooling_factor
        rotary_dim = rope_dim // 2
        inv_freq = 1.0 / (rope_theta ** (torch.arange(0, rotary_dim, 2, dtype=torch.float32) / rotary_dim))
        self.register_buffer("inv_freq", inv_freq.to(self.tensor_factory_kwargs.get("device")), persistent=False)

    def extra_repr(self) -> str:
        return f"rope_theta={self.rope_theta}, rope_dim={self.rope_dim}, adapooling_factor={self.adapooling_factor}"

    @staticmethod
    def check_grid_contract(grid_hw, adapooling_factor: int):
        """The golden's assertions; returns the grids as a list of ``(h, w)`` Python ints (the one host read)."""
        assert grid_hw.ndim == 2 and grid_hw.size(-1) == 2, "grid_hw must be [B, 2]"
        assert not torch.is_floating_point(grid_hw) and grid_hw.dtype != torch.bool, "grid_hw must be an integer tensor"
        grids = [(int(gh), int(gw)) for gh, gw in grid_hw.to(device="cpu", dtype=torch.int64).tolist()]
        for gh, gw in grids:
            assert gh > 0 and gw > 0, "grid height/width must be positive"
            assert gh % adapooling_factor == 0 and gw % adapooling_factor == 0, (
                "grid height/width must be divisible by adapooling_factor")
        return grids


class MojoApplyVisionRoPE2D(MojoOperator):
    """forward(q [T, N, D], k [T, Nk, D], cos [T, D], sin [T, D]) -> (q_rot, k_rot): rotate-half over the FULL ``head_dim`` of
    packed token-first tensors, ``x * cos + rotate_half(x) * sin`` in fp32, rounded once to the input dtype (reference
    `mojo_opset/core/operators/position_embedding.py:366-407`)."""

    def __init__(self):
        super().__init__()

    @staticmethod
    def check_shape_contract(q, k, cos, sin) -> None:
        assert q.ndim == k.ndim, "q and k must have the same dimension"
        assert q.ndim == 3, "q and k must be 3D packed token-first tensors"
        assert q.shape[-1] == k.shape[-1], "q and k must have the same head_dim"
        assert cos.shape == sin.shape, "cos and sin must have the same shape"
        assert cos.ndim == 2, "vision rotary embedding (cos/sin) must be of shape [num_tokens, rope_dim]"
        assert q.shape[0] == cos.shape[0], "packed token count must match cos/sin sequence length"
        assert k.shape[0] == cos.shape[0], "packed token count must match cos/sin sequence length"
        assert q.shape[-1] == cos.shape[-1], "vision rope rotates the full head_dim"
        assert k.shape[-1] == cos.shape[-1], "vision rope rotates the full head_dim"


def check_mrope_contract(query, key, cos_table, sin_table, mrope_section, head_dim):
    """The shared validation of `MojoMRoPE` / `MojoMRoPEInplace`: ``ValueError``s that name the argument.  Returns
    ``(head_dim, half, q_heads, k_heads)``."""
    if len(mrope_section) != 3:
        raise ValueError(f"mrope_section must hold 3 sizes (temporal, height, width), got {list(mrope_section)}")
    sec = [int(s) for s in mrope_section]
    if any(s < 0 for s in sec) or sum(sec) <= 0:
        raise ValueError(f"mrope_section must be non-negative with a positive sum, got {sec}")
    half = sum(sec)
    if head_dim is None:
        head_dim = 2 * half
    head_dim = int(head_dim)
    if 2 * half > head_dim:
        raise ValueError(f"mrope_section {sec} rotates {2 * half} features, more than head_dim {head_dim}")
    if query.dim() != 2 or key.dim() != 2:
        raise ValueError(f"query and key must be 2-D [tokens, heads * head_dim], got {tuple(query.shape)} and {tuple(key.shape)}")
    if query.shape[1] % head_dim:
        raise ValueError(f"query row width {query.shape[1]} is not a multiple of head_dim {head_dim}")
    if key.shape[1] % head_dim:
        raise ValueError(f"key row width {key.shape[1]} is not a multiple of head_dim {head_dim}")
    if query.shape[0] != key.shape[0]:
        raise ValueError(f"query has {query.shape[0]} tokens, key {key.shape[0]}: the token counts must be equal")
    tokens = query.shape[0]
    if cos_table.shape != sin_table.shape or cos_table.dtype != sin_table.dtype:
        raise ValueError(f"cos_table {tuple(cos_table.shape)} and sin_table {tuple(sin_table.shape)} must share shape and dtype")
    want = ((3, tokens, half), (tokens, half))
    if tuple(cos_table.shape) not in want:
        raise ValueError(f"cos_table of shape {tuple(cos_table.shape)}: [3, {tokens}, {half}], or [{tokens}, {half}] when merged")
    return head_dim, half, query.shape[1] // head_dim, key.shape[1] // head_dim


class MojoMRoPE(MojoOperator):
    """forward(query [T, Hq * hd], key [T, Hk * hd], cos_table, sin_table, mrope_section, is_interleaved=False,
    head_dim=None) -> (query, key) with the first ``2 * sum(mrope_section)`` features of every head rotated:
    ``h1 * c - h2 * s`` and ``h2 * c + h1 * s`` over the halves, the rest passed through (reference
    `mojo_opset/core/operators/position_embedding.py:178-278`).  Tables are ``[3, T, half]`` (temporal, height, width: element
    ``i`` takes the table of the section it falls in, or with ``is_interleaved`` table 1 where ``i % 3 == 1 and
    i < 3 * section[1]``, table 2 where ``i % 3 == 2 and i < 3 * section[2]``, table 0 elsewhere) or ``[T, half]`` when already
    merged."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)

    def extra_repr(self) -> str:
        return ""


class MojoMRoPEInplace(MojoOperator):
    """`MojoMRoPE` in its serving form (reference `mojo_opset/experimental/operators/position_embedding.py:121-236`): with
    ``inplace=True`` the rotated features are written back into ``query`` and ``key``, which are returned."""

    def __init__(self, inplace: bool = False, **kwargs):
        super().__init__(**kwargs)
        self.inplace = inplace

    def extra_repr(self) -> str:
        return ""
