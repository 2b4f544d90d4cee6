"""API classes of the over-encoding input layer (`EMBEDDING_OPS`): constructors, attributes, buffers and `state_dict` keys of the
reference's `mojo_opset/core/operators/over_encoding.py`; the torch goldens live in ``tests/embedding_golden.py``.

Over-encoding adds, to the row of the original table, one row of a "mega" table per n-gram vocabulary ``g``.  The row is picked
by an id that hashes the token and its ``oe_grams[g] - 1`` predecessors into ``[0, oe_vocab_sizes[g])``::

    id = x[t]; carry = ori_vocab_size
    for i in 1 .. n - 1:  id = (id + p(i) * carry) mod V;  carry = carry * ori_vocab_size mod V
    out[t, g] = id + oe_vocab_offsets[g]

``p(i)`` is the token ``i`` places before ``t``: ``input_ids[t - i]`` inside the sequence, before its start the history row of
that sequence read from its END (``history[H + t - i]``; a history longer than ``max gram - 1`` is legal, only its tail counts).
The first carry is not reduced, and a gram of 1 applies no modulus at all."""
from typing import List, Optional

import torch
from torch.nn import Parameter

from ..operator import MojoOperator

WORKSPACE_BUFFERS = ("oe_vocab_sizes", "oe_grams", "oe_vocab_offsets")

NF4_CODEBOOK = (
    -1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635, -0.18477343022823334,
    -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
    0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0,
)


def get_nf4_codebook(device, dtype: torch.dtype = torch.float16) -> torch.Tensor:
    """The 16 NF4 levels.  The reference holds them in fp16: the ROUNDED constants are the codebook."""
    return torch.tensor(NF4_CODEBOOK, device=device, dtype=dtype)


def ignore_workspace_buffers_hook(ignore_keys=WORKSPACE_BUFFERS):
    """A `load_state_dict` post hook: a checkpoint that lacks the three derived buffers still loads strictly."""
    def load_state_dict_post_hook(module, incompatible_keys) -> None:
        for miss in [k for k in incompatible_keys.missing_keys if k.split(".")[-1] in ignore_keys]:
            incompatible_keys.missing_keys.remove(miss)

    return load_state_dict_post_hook


def vocab_offsets(oe_vocab_sizes: torch.Tensor) -> torch.Tensor:
    """int64 exclusive prefix sum of the vocabulary sizes: where each vocabulary starts in the mega table."""
    zero = torch.tensor([0], device=oe_vocab_sizes.device, dtype=oe_vocab_sizes.dtype)
    return torch.cumsum(torch.cat([zero, oe_vocab_sizes[:-1]], dim=0).to(torch.long), dim=0)


def check_oe_call_contract(input_ids, oe_history_input, q_lens, max_gram: int) -> None:
    """The reference's assertions on the two call forms, and a ``ValueError`` for a history shorter than ``max gram - 1``
    (the reference fails there with a broadcast ``RuntimeError``)."""
    if q_lens is not None:
        assert input_ids.dim() == 1, "packed form: input_ids must be [total_tokens]"
        assert oe_history_input.dim() == 2 and oe_history_input.size(0) == q_lens.size(0), (
            "packed form: oe_history_input must be [batch_size, >= max_n_gram - 1] with one row per q_lens entry")
        assert q_lens.dim() == 1, "q_lens must be [batch_size]"
    else:
        assert input_ids.dim() == 2, "batched form: input_ids must be [batch_size, seq_len]"
        assert oe_history_input.dim() == 2 and oe_history_input.size(0) == input_ids.size(0), (
            "batched form: oe_history_input must be [batch_size, >= max_n_gram - 1]")
    if oe_history_input.size(1) < max_gram - 1:
        raise ValueError(f"oe_history_input holds {oe_history_input.size(1)} tokens per sequence, fewer than max gram - 1 = "
                         f"{max_gram - 1}")


class MojoOverEncodingNGram(MojoOperator):
    """forward(input_ids, oe_history_input, q_lens=None) -> n-gram ids ``[..., G]`` in the dtype of ``input_ids`` (reference
    `core/operators/over_encoding.py:61-156`).  Packed: ``input_ids [T]`` with ``q_lens [B]`` and ``oe_history_input [B, H]``;
    batched: ``input_ids [B, S]`` with ``oe_history_input [B, H]``."""

    def __init__(self, ori_vocab_size: int, oe_vocab_sizes: List[int], oe_grams: List[int], **kwargs):
        super().__init__(**kwargs)
        self.ori_vocab_size = ori_vocab_size
        self._oe_vocab_sizes = oe_vocab_sizes
        self._oe_grams = oe_grams
        self._oe_post_init()

    def _oe_post_init(self):
        device = torch.tensor([]).device
        if device == torch.device("meta"):
            device = torch.device("cpu")
        self.register_buffer("oe_vocab_sizes", torch.tensor(self._oe_vocab_sizes, device=device, dtype=torch.int64),
                             persistent=False)
        self.register_buffer("oe_grams", torch.tensor(self._oe_grams, device=device, dtype=torch.int64), persistent=False)
        self.register_buffer("oe_vocab_offsets", vocab_offsets(self.oe_vocab_sizes), persistent=False)

    def extra_repr(self) -> str:
        return f"ori_vocab_size={self.ori_vocab_size}, oe_vocab_sizes={self._oe_vocab_sizes}, oe_grams={self._oe_grams}"


class MojoNF4DequantEmbedding(MojoOperator):
    """forward(input int ``(*)``) -> ``(*, embedding_dim)`` in ``output_dtype``: rows of a packed-NF4 table, dequantised on the
    fly (reference `core/operators/over_encoding.py:480-584`).  ``qweight [rows, dim / 2]`` int8 / uint8 holds element ``2j`` in
    the low and ``2j + 1`` in the high nibble of byte ``j``; ``scale`` / ``mean`` are ``[rows, dim / group_size]``; the value is
    ``fp32(codebook[nibble]) * fp32(scale) + fp32(mean)`` — two fp32 roundings — rounded once to ``output_dtype``.  An id
    outside ``[vocab_start_id, vocab_start_id + rows)`` gives a row of zeros."""

    def __init__(self, qweight: torch.Tensor, scale: torch.Tensor, mean: torch.Tensor, *, group_size: int,
                 vocab_start_id: int = 0, cpu_only: bool = False, output_dtype: torch.dtype = torch.bfloat16, **kwargs):
        super().__init__(**kwargs)
        if qweight.ndim != 2 or scale.ndim != 2 or mean.ndim != 2:
            raise ValueError("NF4 embedding tensors must all be 2D, "
                             f"got qweight={tuple(qweight.shape)}, scale={tuple(scale.shape)}, mean={tuple(mean.shape)}.")
        if scale.shape != mean.shape:
            raise ValueError(f"`scale` and `mean` must have the same shape, got {scale.shape} and {mean.shape}.")
        if group_size <= 0:
            raise ValueError(f"`group_size` must be > 0, got {group_size}.")
        self.embedding_dim = scale.size(1) * group_size
        if qweight.size(1) * 2 != self.embedding_dim:
            raise ValueError(f"`weight` shape {tuple(qweight.shape)} is incompatible with "
                             f"`scale` shape {tuple(scale.shape)} and group_size={group_size}.")
        self.group_size = group_size
        self.output_dtype = output_dtype
        self.vocab_start_id = vocab_start_id
        codebook = get_nf4_codebook(device=qweight.device, dtype=torch.float16)
        if not cpu_only:
            self.register_parameter("weight", Parameter(qweight, requires_grad=False))
            self.register_parameter("scale", Parameter(scale, requires_grad=False))
            self.register_parameter("mean", Parameter(mean, requires_grad=False))
            self.register_parameter("codebook", Parameter(codebook, requires_grad=False))
        else:                                     # plain attributes: the table stays on the CPU whatever the module moves to
            self.weight, self.scale, self.mean, self.codebook = qweight, scale, mean, codebook

    def extra_repr(self) -> str:
        return (f"vocab_size={self.weight.size(0)}, embedding_dim={self.scale.size(1) * self.group_size}, "
                f"group_size={self.group_size}, output_dtype={self.output_dtype}")


class MojoOverEncoding(MojoOperator):
    """forward(input_tensor, oe_history_input, q_lens=None) -> ``[..., ori_embed_dim]``: the original table's row of every token
    and the mega table's rows of its ``G`` n-gram ids, concatenated in that order and multiplied by ``oe_up_proj`` (reference
    `core/operators/over_encoding.py:159-375`).  The mega table is a dense ``torch.nn.Embedding`` or, when weight, scale and mean
    are all given, a `MojoNF4DequantEmbedding` of this layer's backend."""

    def __init__(self, ori_vocab_size: int, ori_embed_dim: int, oe_embed_dim: int, oe_vocab_sizes, oe_grams,
                 _ori_embedding_weight: torch.Tensor = None, _mega_embedding_weight: torch.Tensor = None,
                 _mega_embedding_scale: torch.Tensor = None, _mega_embedding_mean: torch.Tensor = None,
                 _mega_embedding_group_size: int = 1, _mega_embedding_vocab_start_id: int = 0,
                 mega_embedding_cpu_only=False, **kwargs):
        super().__init__(**kwargs)
        self.ori_vocab_size = ori_vocab_size
        self.ori_embed_dim = ori_embed_dim
        self.oe_embed_dim = oe_embed_dim
        self.mega_embedding_cpu_only = mega_embedding_cpu_only
        as_tensor = lambda v: v if isinstance(v, torch.Tensor) else torch.tensor(v, **self.tensor_factory_kwargs)  # noqa: E731
        self.register_buffer("oe_vocab_sizes", as_tensor(oe_vocab_sizes))
        self.register_buffer("oe_grams", as_tensor(oe_grams))
        self.register_buffer("oe_vocab_offsets", vocab_offsets(self.oe_vocab_sizes))
        self.register_load_state_dict_post_hook(ignore_workspace_buffers_hook())
        device = self.tensor_factory_kwargs.get("device", None)
        self.ori_embedding = torch.nn.Embedding(self.ori_vocab_size, self.ori_embed_dim, _weight=_ori_embedding_weight,
                                                device=device)
        self.oe_mega_embedding = self._create_mega_embedding(_mega_embedding_weight, _mega_embedding_scale,
                                                             _mega_embedding_mean, _mega_embedding_group_size,
                                                             _mega_embedding_vocab_start_id)
        self.oe_up_proj = torch.nn.Linear(len(self.oe_vocab_sizes) * self.oe_embed_dim + self.ori_embed_dim,
                                          self.ori_embed_dim, bias=False, device=device)

    def _nf4_embedding_class(self):
        return MojoNF4DequantEmbedding.get_registry().get(self._backend)

    def _create_mega_embedding(self, weight, scale, mean, group_size, vocab_start_id) -> torch.nn.Module:
        if weight is not None and scale is not None and mean is not None:
            return self._nf4_embedding_class()(weight, scale, mean, group_size=group_size, vocab_start_id=vocab_start_id,
                                               output_dtype=self.tensor_factory_kwargs.get("dtype", None),
                                               cpu_only=self.mega_embedding_cpu_only)
        mega = torch.nn.Embedding(sum(self.oe_vocab_sizes).item(), self.oe_embed_dim, _weight=weight,
                                  device=self.tensor_factory_kwargs.get("device", None))
        if self.mega_embedding_cpu_only:
            assert weight is not None and weight.device.type == "cpu"
            delattr(mega, "weight")               # no longer a Parameter: it stays on the CPU whatever the module moves to
            mega.weight = weight
        return mega

    def extra_repr(self) -> str:
        return (f"{self.ori_vocab_size=}, {self.ori_embed_dim=}, {self.oe_embed_dim=}, {self.oe_vocab_sizes=}, "
                f"{self.oe_grams=}, {self.mega_embedding_cpu_only=}").replace("self.", "")
