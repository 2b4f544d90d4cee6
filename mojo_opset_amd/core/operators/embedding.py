"""API classes of the plain embedding lookups (`EMBEDDING_OPS`): constructors, attributes and `state_dict` keys of the
reference's `mojo_opset/core/operators/embedding.py`; the torch goldens live in ``tests/embedding_golden.py``."""
import math
from typing import Optional

import torch
import torch.distributed as dist
import torch.nn as nn

from ..operator import MojoOperator


def is_dist_initialized() -> bool:
    return dist.is_available() and dist.is_initialized()


class MojoEmbedding(MojoOperator):
    """forward(input int ``(*)``) -> ``(*, embedding_dim)``: the rows ``weight[input]`` (a drop-in for ``torch.nn.Embedding``;
    reference `core/operators/embedding.py:16-70`).  ``padding_idx`` zeroes that row at initialisation and has no effect in a
    forward pass; ``max_norm`` renormalises the table in place before the lookup."""

    def __init__(self, num_embeddings: int, embedding_dim: int, padding_idx: Optional[int] = None,
                 max_norm: Optional[float] = None, norm_type: float = 2.0, device=None, dtype=None):
        super().__init__()
        self.num_embeddings = num_embeddings
        self.embedding_dim = embedding_dim
        self.padding_idx = padding_idx
        self.max_norm = max_norm
        self.norm_type = norm_type
        self.weight = nn.Parameter(torch.empty(num_embeddings, embedding_dim, device=device, dtype=dtype))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        nn.init.normal_(self.weight)
        if self.padding_idx is not None:
            with torch.no_grad():
                self.weight[self.padding_idx].fill_(0)

    def extra_repr(self) -> str:
        s = f"num_embeddings={self.num_embeddings}, embedding_dim={self.embedding_dim}"
        if self.padding_idx is not None:
            s += f", padding_idx={self.padding_idx}"
        if self.max_norm is not None:
            s += f", max_norm={self.max_norm}, norm_type={self.norm_type}"
        return s


class MojoParallelEmbedding(MojoOperator):
    """Vocabulary-parallel embedding (reference `core/operators/embedding.py:73-169`): rank ``r`` of ``w`` holds the rows
    ``[r * ceil(num / w), min((r + 1) * ceil(num / w), num))``; an index outside the local range gives a row of zeros and an
    ``all_reduce`` (sum) assembles the result.  Without an initialised process group it is one shard holding everything."""

    def __init__(self, num_embeddings: int, embedding_dim: int, padding_idx: Optional[int] = None,
                 max_norm: Optional[float] = None, norm_type: float = 2.0, process_group=None, device=None, dtype=None):
        super().__init__()
        self.num_embeddings = num_embeddings
        self.embedding_dim = embedding_dim
        self.padding_idx = padding_idx
        self.max_norm = max_norm
        self.norm_type = norm_type
        self.process_group = process_group
        if is_dist_initialized():
            world_size, rank = dist.get_world_size(group=process_group), dist.get_rank(group=process_group)
        else:
            world_size, rank = 1, 0
        local_size = math.ceil(num_embeddings / world_size)          # the last rank may own fewer rows
        self.vocab_start_index = rank * local_size
        self.vocab_end_index = min(self.vocab_start_index + local_size, num_embeddings)
        self.local_num_embeddings = self.vocab_end_index - self.vocab_start_index
        self.weight = nn.Parameter(torch.empty(self.local_num_embeddings, embedding_dim, device=device, dtype=dtype))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        nn.init.normal_(self.weight)
        if self.padding_idx is not None:
            local_pad = self.padding_idx - self.vocab_start_index
            if 0 <= local_pad < self.local_num_embeddings:
                with torch.no_grad():
                    self.weight[local_pad].fill_(0)

    def extra_repr(self) -> str:
        s = (f"num_embeddings={self.num_embeddings}, embedding_dim={self.embedding_dim}, "
             f"local_range=[{self.vocab_start_index}, {self.vocab_end_index})")
        if self.padding_idx is not None:
            s += f", padding_idx={self.padding_idx}"
        return s
