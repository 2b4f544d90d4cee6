"""Paged-cache helpers shared by every golden of the package and by the fixture recipes (`oracle/make_*_golden.py`).

Two page gathers stand side by side because the reference has two: `gather_pages` stops at the first negative page id
(the §8 GQA pair), `index_pages` indexes the cache with the table as it is (the sliding-window and int8-cache ops).
"""
from typing import Optional

import torch


def cu(lens) -> torch.Tensor:
    """int32 ``[len(lens) + 1]``: the running sum of ``lens`` behind a leading 0."""
    return torch.tensor([0] + list(torch.tensor(lens).cumsum(0).tolist()), dtype=torch.int32)


def gather_pages(cache: torch.Tensor, table_row: torch.Tensor, length: int) -> torch.Tensor:
    """``[length, heads, D]`` rows of one sequence pulled out of ``cache [N, heads, page, D]``.

    Pages are walked in logical order; the walk stops at the first negative id and the remaining
    rows stay zero — the behaviour of the reference's ``break`` inside a zero-initialised buffer
    (`core/operators/attention.py:190-207`, :405-419).
    """
    page = cache.shape[2]
    heads, dim = cache.shape[1], cache.shape[3]
    out = torch.zeros(length, heads, dim, dtype=cache.dtype, device=cache.device)
    n_pages = (length + page - 1) // page
    ids = table_row[:n_pages].to(torch.int64)
    bad = (ids < 0).nonzero()
    if bad.numel():
        n_pages = int(bad[0])
        ids = ids[:n_pages]
    if n_pages == 0:
        return out
    rows = cache[ids].permute(0, 2, 1, 3).reshape(n_pages * page, heads, dim)   # token-major
    take = min(length, n_pages * page)
    out[:take] = rows[:take]
    return out


def index_pages(cache: torch.Tensor, table_row: torch.Tensor, kv_len: int) -> torch.Tensor:
    """``[heads, kv_len, D]`` of one sequence: its first ceil(kv_len / page) pages by plain indexing of the table (a
    negative id indexes from the end of the cache, as in the reference), token-major within each head."""
    heads, page, dim = cache.shape[1], cache.shape[2], cache.shape[3]
    blocks = (kv_len + page - 1) // page
    x = cache[table_row[:blocks].long()]                             # [blocks, heads, page, D]
    return x.permute(1, 0, 2, 3).reshape(heads, blocks * page, dim)[:, :kv_len]


def expand_kv_heads(x: torch.Tensor, group: int, layout: str, dim: int = 0) -> torch.Tensor:
    """``Hkv -> Hq = group * Hkv`` along ``dim``: AABB repeats each kv head, ABAB tiles them
    (`core/operators/attention.py:209-214`)."""
    if group == 1:
        return x
    if layout == "AABB":
        return x.repeat_interleave(group, dim=dim)
    reps = [1] * x.dim()
    reps[dim] = group
    return x.repeat(reps)


def window_mask(q_len: int, kv_len: int, local: Optional[int], glob: Optional[int]) -> torch.Tensor:
    """``[q_len, kv_len]`` bool: row i (position ``p = kv_len - q_len + i``) sees key j iff ``j <= p`` and, when a window
    is set, ``j >= p - local`` or ``j < glob`` (`core/operators/attention.py:507-531`)."""
    pos = torch.arange(q_len)[:, None] + (kv_len - q_len)
    key = torch.arange(kv_len)[None, :]
    mask = key <= pos
    if local is not None or glob is not None:
        win = torch.zeros(q_len, kv_len, dtype=torch.bool)
        if local is not None:
            win |= pos <= key + local
        if glob is not None:
            win |= key < glob
        mask &= win
    return mask
