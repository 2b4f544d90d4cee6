"""An fp64 model of native-sparse-attention prefill (row ``t`` is `nsa_golden.model_one` on its first ``t_kv`` keys; ``t_kv <= 0``
gives zeros and ``0 < t_kv < compress_ratio`` takes groups of one key) and the input builder of its tests."""
import functools

import numpy as np
import torch

from mojo_opset_amd.core.operators.attention import MojoPagedPrefillNSA, MojoPrefillNSA
from nsa_golden import CFG, HEADS, model_one, paged, with_gate  # noqa: F401

SEQS = ((0, 0), (3, 3), (37, 37), (5, 70), (1, 129), (150, 150), (33, 200))        # (q_len, kv_len)
STEP = 6.0           # what one level of the graded plant adds to a key's score (4 leaves a worst taken / not-taken ratio of 1.67)


class TorchPrefillNSA(MojoPrefillNSA):
    """The core class's golden ``forward`` as the ``torch`` backend."""
    supported_platforms_list = ["rocm", "cpu"]


class TorchPagedPrefillNSA(MojoPagedPrefillNSA):
    supported_platforms_list = ["rocm", "cpu"]


def model(c, key=None, value=None, check=False):
    """``out64 [T,H,D]`` of case ``c`` (on ``key`` / ``value`` [B,S,H,D] instead of the case's own when given).  ``check``: assert
    for every (row, head) that the lowest taken block score is at least 4 x the highest one not taken."""
    key, value = c["key"] if key is None else key, c["value"] if value is None else value
    q, gate, cfg = c["query"].double().numpy(), c["gate"].double().numpy(), c["cfg"]
    out, row = np.zeros(q.shape), 0
    for i, (q_len, kv_len) in enumerate(c["seqs"]):
        k, v = key[i, :kv_len].double().numpy(), value[i, :kv_len].double().numpy()
        for t in range(q_len):
            t_kv = kv_len - q_len + t + 1 if c["causal"] else kv_len
            if t_kv >= cfg["compress_ratio"]:
                out[row], scores, taken = model_one(q[row], k[:t_kv], v[:t_kv], gate, c["scale"], **cfg)
                for h in range(q.shape[1] if check else 0):
                    rest = np.delete(scores[h], taken[h])
                    assert rest.size == 0 or scores[h, taken[h]].min() >= 4 * rest.max(), (i, t, h, scores[h])
            elif t_kv > 0:                                   # not compressed: groups of one key, one block
                one = dict(cfg, compress_ratio=1, block_size=max(cfg["block_size"], t_kv))
                out[row] = model_one(q[row], k[:t_kv], v[:t_kv], gate, c["scale"], **one)[0]
            row += 1
    return torch.from_numpy(out)


@functools.lru_cache(maxsize=None)
def build(dim, dtype, seqs=SEQS, heads=HEADS, cfg=tuple(CFG.items()), plant=True, causal=True, seed=0):
    """Seeded inputs in ``dtype``.  Graded plant: per (sequence, head) a direction ``u``, queries ``u + 0.5 noise``, and every key
    of selection block ``b`` gains ``level_b STEP / (scale |u|^2) u`` with ``level`` a permutation of ``0..nb-1`` per head, so
    the blocks are strictly ordered for every row and every prefix; `model` asserts the margin.  K / V ``[B,S,H,D]`` are NaN past
    a sequence's length; ``query`` / ``out64`` are packed ``[T,H,D]``."""
    cfg, gen = dict(cfg), torch.Generator().manual_seed(seed)
    cap, scale, bs = max(max(kv for _, kv in seqs), 1), dim ** -0.5, dict(cfg)["block_size"]
    k, v = torch.randn(len(seqs), cap, heads, dim, generator=gen), torch.randn(len(seqs), cap, heads, dim, generator=gen)
    gate, qs = (torch.randn(heads, dim, 3, generator=gen) * scale).to(dtype), []
    for i, (q_len, kv_len) in enumerate(seqs):
        u = torch.randn(heads, dim, generator=gen)
        qs.append(u + 0.5 * torch.randn(q_len, heads, dim, generator=gen) if plant else torch.randn(q_len, heads, dim, generator=gen))
        nb = -(-kv_len // bs)
        for h in range(heads if plant else 0):
            level = torch.randperm(nb, generator=gen).repeat_interleave(bs)[:kv_len].double()
            k[i, :kv_len, h] += (level * STEP / (scale * u[h].dot(u[h])))[:, None] * u[h]
        k[i, kv_len:], v[i, kv_len:] = float("nan"), float("nan")
    cu = lambda j: torch.tensor([0] + [s[j] for s in seqs], dtype=torch.int32).cumsum(0).int()  # noqa: E731
    c = dict(query=torch.cat(qs).to(dtype), key=k.to(dtype), value=v.to(dtype), gate=gate, seqs=seqs, cu_q=cu(0), cu_kv=cu(1),
             lens=torch.tensor([kv for _, kv in seqs], dtype=torch.int32), scale=scale, cfg=cfg, causal=causal)
    c["out64"] = model(c, check=plant)
    return c


def run(op, c, page, device="cpu", hole=None):
    """Case ``c`` through ``op``: packed contiguous K/V for ``page`` None (every kv_len = q_len), else caches of that page size."""
    op = with_gate(op, c, device)
    if page is None:
        key, value = (torch.cat([x[i, :kv] for i, (_, kv) in enumerate(c["seqs"])]) for x in (c["key"], c["value"]))
        return op(c["query"].to(device), key.to(device), value.to(device), c["cu_q"].to(device))
    kc, vc, table = paged(c, page, hole)
    return op(c["query"].to(device), kc.to(device), vc.to(device), c["cu_q"].to(device), table.to(device),
              cu_total_seq_lens=c["cu_kv"].to(device))
