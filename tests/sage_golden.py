"""An fp64 model of `MojoPagedPrefillSageGQA` (the class docstring's six steps as a plain loop over sequences and heads) and the
one input builder of its tests.  The scores are the fp32 products of step 2, in their order, and ``s - m`` is an fp32 difference;
``exp``, the sums and the quotient are fp64 / exact integers."""
import numpy as np
import torch

from mojo_opset_amd.core.operators.attention import MojoPagedPrefillSageGQA


class TorchPagedPrefillSageGQA(MojoPagedPrefillSageGQA):
    """The core class's golden ``forward`` as the ``torch`` backend (what the reference generates for every core op)."""
    supported_platforms_list = ["rocm", "cpu"]


def model(c, layout="AABB"):
    """``out64 [T, Hq, D]`` (fp64, zeros where no key is seen) and the integer row sums ``S [T, Hq]`` of case ``c``."""
    q, k, v = c["query"].numpy(), c["key_cache"].numpy(), c["value_cache"].numpy()
    qs, ks, vs = c["query_scale"].numpy(), c["key_scale"].numpy(), c["value_scale"].numpy()
    tokens, hq, dim = q.shape
    hkv, page = k.shape[1], k.shape[2]
    scale = np.float32(c["softmax_scale"])
    out, sums = np.zeros((tokens, hq, dim)), np.zeros((tokens, hq), dtype=np.int64)
    cu_q, cu_kv, table = c["cu_q_lens"].tolist(), c["cu_total_seq_lens"].tolist(), c["block_tables"].tolist()
    for b in range(len(cu_q) - 1):
        q_len, kv_len = cu_q[b + 1] - cu_q[b], cu_kv[b + 1] - cu_kv[b]
        for h in range(hq):
            kh = h % hkv if layout == "ABAB" else h // (hq // hkv)
            keys = [(table[b][j // page], j % page) for j in range(kv_len)]
            k8 = np.array([k[n, kh, i] for n, i in keys], dtype=np.int64).reshape(kv_len, dim)
            v8 = np.array([v[n, kh, i] for n, i in keys], dtype=np.int64).reshape(kv_len, dim)
            k_scale = np.array([ks[n, kh, i] for n, i in keys], dtype=np.float32)
            for i in range(q_len):
                t, seen = cu_q[b] + i, kv_len - q_len + i + 1
                if seen <= 0:
                    continue
                dot = (k8[:seen] @ q[t, h].astype(np.int64)).astype(np.float32)
                s = ((dot * scale) * qs[h, t]) * k_scale[:seen]
                p = np.rint(np.exp((s - s.max()).astype(np.float64)) * 127).astype(np.int64)
                sums[t, h] = p.sum()
                out[t, h] = vs[kh].astype(np.float64) * (p @ v8[:seen]) / p.sum()
    return torch.from_numpy(out), torch.from_numpy(sums)


def build(dim, page, hq, hkv, q_lens, cached, seed=0, spare=3, extra_width=2):
    """Seeded normal data quantised per token (Q, K) and per channel (V); shuffled page ids, a table wider than needed padded
    with -1; spare pages and the unused tail of every last page hold ``key_scale = NaN`` and 127s in K and V."""
    gen = torch.Generator().manual_seed(seed)
    kv_lens = [a + b for a, b in zip(q_lens, cached)]
    tokens, need = sum(q_lens), [(n + page - 1) // page for n in kv_lens]
    n_blocks = sum(need) + spare

    def quant(x, axis):
        s = x.abs().amax(dim=axis, keepdim=True).clamp_min(1e-6) / 127
        return torch.round(x / s).clamp(-127, 127).to(torch.int8), s.squeeze(axis).float()

    q8, qs = quant(torch.randn(tokens, hq, dim, generator=gen), -1)
    key_cache = torch.full((n_blocks, hkv, page, dim), 127, dtype=torch.int8)
    value_cache = torch.full((n_blocks, hkv, page, dim), 127, dtype=torch.int8)
    key_scale = torch.full((n_blocks, hkv, page), float("nan"))
    ids = torch.randperm(n_blocks, generator=gen).tolist()
    table = torch.full((len(q_lens), max(need) + extra_width), -1, dtype=torch.int32)
    v_all = torch.randn(sum(kv_lens), hkv, dim, generator=gen)
    v8_all, vs = quant(v_all, 0)
    at = 0
    for b, n in enumerate(kv_lens):
        k8, ks = quant(torch.randn(n, hkv, dim, generator=gen), -1)
        for j in range(n):
            blk = ids[sum(need[:b]) + j // page]
            table[b, j // page] = blk
            key_cache[blk, :, j % page], key_scale[blk, :, j % page] = k8[j], ks[j]
            value_cache[blk, :, j % page] = v8_all[at + j]
        at += n
    cu = lambda lens: torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)   # noqa: E731
    return dict(query=q8, query_scale=qs.T.contiguous(), key_cache=key_cache, key_scale=key_scale, value_cache=value_cache,
                value_scale=vs, cu_q_lens=cu(q_lens), block_tables=table, softmax_scale=dim ** -0.5,
                cu_total_seq_lens=cu(kv_lens))


ARGS = ("query", "query_scale", "key_cache", "key_scale", "value_cache", "value_scale", "cu_q_lens", "block_tables",
        "softmax_scale", "cu_total_seq_lens")


def call(op, c, device="cpu", **kw):
    return op(*[c[k].to(device) if isinstance(c[k], torch.Tensor) else c[k] for k in ARGS], **kw)
