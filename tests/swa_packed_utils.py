"""Inputs of the `MojoSWA` tests: packed contiguous K/V, and the same tokens scattered into a paged cache."""
import torch


def cumulative(lens, start=0):
    out = [start]
    for n in lens:
        out.append(out[-1] + n)
    return torch.tensor(out, dtype=torch.int32)


def packed_inputs(kv_lens, q_lens, hq=8, hkv=2, d=128, dtype=torch.bfloat16, seed=0, lead=0, tail=0, q_pad=0):
    """(query, key, value, cu_q_lens, cu_total_seq_lens): ``lead`` unused K/V tokens in front of the first sequence, ``tail``
    behind the last one, ``q_pad`` query rows no sequence owns."""
    g = torch.Generator().manual_seed(seed)
    cu_q, cu_kv = cumulative(q_lens), cumulative(kv_lens, lead)
    q = torch.randn(int(cu_q[-1]) + q_pad, hq, d, generator=g).to(dtype)
    k = torch.randn(int(cu_kv[-1]) + tail, hkv, d, generator=g).to(dtype)
    v = torch.randn(int(cu_kv[-1]) + tail, hkv, d, generator=g).to(dtype)
    return q, k, v, cu_q, cu_kv


def scatter_to_pages(key, value, cu_kv, page, seed=0, spare=3):
    """The tokens of every sequence copied into pages of ``page`` keys handed out in random order: (key_cache, value_cache
    [N, Hkv, page, D], block_table [B, max_pages], cu_total_seq_lens starting at 0).  Unused slots hold zeros."""
    g = torch.Generator().manual_seed(seed + 99)
    cu = cu_kv.tolist()
    lens = [cu[b + 1] - cu[b] for b in range(len(cu) - 1)]
    need = [max((n + page - 1) // page, 0) for n in lens]
    total = sum(need) + spare
    hkv, d = key.shape[1:]
    kc = torch.zeros(total, hkv, page, d, dtype=key.dtype)
    vc = torch.zeros(total, hkv, page, d, dtype=key.dtype)
    table = torch.full((len(lens), max(max(need, default=0), 1)), -1, dtype=torch.int32)
    free = torch.randperm(total, generator=g, dtype=torch.int32)
    at = 0
    for b, n in enumerate(need):
        table[b, :n] = free[at: at + n]
        at += n
        for p in range(n):
            lo = cu[b] + p * page
            hi = min(lo + page, cu[b + 1])
            kc[int(table[b, p]), :, : hi - lo] = key[lo:hi].permute(1, 0, 2)
            vc[int(table[b, p]), :, : hi - lo] = value[lo:hi].permute(1, 0, 2)
    return kc, vc, table, cumulative(lens)
