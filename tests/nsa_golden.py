"""An fp64 model of the native-sparse-attention decode step (the definition in `_NSADecodeBase`'s docstring, branch by branch,
as a loop over sequences and heads; among equal block scores the lower block index is taken) and the input builder of its
tests."""
import functools

import numpy as np
import torch

from mojo_opset_amd.core.operators.attention import MojoDecodeNSA, MojoPagedDecodeNSA

LENS, HEADS, CFG = [0, 3, 61, 333, 1030], 3, dict(compress_ratio=4, block_size=32, num_selected_blocks=2, window_size=48)
PLANT = 6.0          # what a planted key's score gains: e^6 = 403 in ONE group outweighs 4 x a whole unplanted block (8 groups ~ e^0.1)


class TorchDecodeNSA(MojoDecodeNSA):
    """The core class's golden ``forward`` as the ``torch`` backend (what the reference generates for every core op)."""
    supported_platforms_list = ["rocm", "cpu"]


class TorchPagedDecodeNSA(MojoPagedDecodeNSA):
    supported_platforms_list = ["rocm", "cpu"]


def _softmax(x):
    e = np.exp(x - x.max()) if x.size else x
    return e / e.sum() if x.size else e


def model_one(q, k, v, gate, scale, compress_ratio, block_size, num_selected_blocks, window_size):
    """q [H,D], k / v [sl,H,D], gate [H,D,3], all fp64 -> (out [H,D], block scores [H,nb], taken blocks per head)."""
    sl, heads, dim = k.shape
    cr, bs = compress_ratio, block_size
    n_groups, nb = sl // cr, -(-sl // bs)
    out, scores, taken = np.zeros((heads, dim)), np.zeros((heads, nb)), []
    for h in range(heads):
        ck = k[:n_groups * cr, h].reshape(n_groups, cr, dim).mean(axis=1)
        cv = v[:n_groups * cr, h].reshape(n_groups, cr, dim).mean(axis=1)
        pc = _softmax(scale * ck @ q[h])
        for b in range(nb):
            scores[h, b] = pc[b * (bs // cr):min((b + 1) * (bs // cr), n_groups)].sum()
        chosen = sorted(range(nb), key=lambda b: (-scores[h, b], b))[:min(num_selected_blocks, nb)]
        taken.append(chosen)
        s = scale * k[:, h] @ q[h]
        keys = np.concatenate([np.arange(b * bs, min((b + 1) * bs, sl)) for b in sorted(chosen)]) if chosen else np.arange(0)
        win = np.arange(max(0, sl - window_size), sl)
        g = 1.0 / (1.0 + np.exp(-(q[h] @ gate[h])))
        out[h] = g[0] * (pc @ cv) + g[1] * (_softmax(s[keys]) @ v[keys, h]) + g[2] * (_softmax(s[win]) @ v[win, h])
    return out, scores, taken


def model(c, key=None, value=None):
    """``out64 [B,H,D]`` of case ``c`` (on ``key`` / ``value`` [B,S,H,D] instead of the case's own when given)."""
    key, value = c["key"] if key is None else key, c["value"] if value is None else value
    out = np.zeros(c["query"].shape)
    for i, sl in enumerate(c["lens"].tolist()):
        if sl > 0:
            out[i] = model_one(c["query"][i].double().numpy(), key[i, :sl].double().numpy(), value[i, :sl].double().numpy(),
                               c["gate"].double().numpy(), c["scale"], **c["cfg"])[0]
    return torch.from_numpy(out)


@functools.lru_cache(maxsize=None)
def build(dim, dtype, lens=tuple(LENS), heads=HEADS, cfg=tuple(CFG.items()), plant=True, seed=0):
    """Seeded normal q / K / V in ``dtype``; per (sequence, head) ``min(nsel, nb)`` planted blocks (another set per head) whose
    keys gain ``PLANT / (scale |q|^2) * q``.  Asserts, in fp64, that the lowest taken block score is at least 4 x the highest
    one not taken: the taken set is then the same under the golden's roundings and a kernel's.  K / V past a sequence's length
    are NaN.  ``out64`` is the model's result."""
    cfg, gen = dict(cfg), torch.Generator().manual_seed(seed)
    batch, cap, scale = len(lens), max(lens), dim ** -0.5
    q = torch.randn(batch, heads, dim, generator=gen).to(dtype)
    k, v = torch.randn(batch, cap, heads, dim, generator=gen), torch.randn(batch, cap, heads, dim, generator=gen)
    gate = (torch.randn(heads, dim, 3, generator=gen) * scale).to(dtype)
    bs, nsel = cfg["block_size"], cfg["num_selected_blocks"]
    for i, sl in enumerate(lens):
        nb = -(-sl // bs)
        for h in range(heads if plant else 0):
            qf = q[i, h].float()
            for b in torch.randperm(nb, generator=gen)[:min(nsel, nb)].tolist():
                k[i, b * bs:(b + 1) * bs, h] += PLANT / (scale * qf.dot(qf)) * qf
        k[i, sl:], v[i, sl:] = float("nan"), float("nan")
    c = dict(query=q, key=k.to(dtype), value=v.to(dtype), gate=gate, lens=torch.tensor(lens, dtype=torch.int32), scale=scale, cfg=cfg)
    for i, sl in enumerate(lens):
        if plant and sl > 0:
            _, scores, taken = model_one(q[i].double().numpy(), c["key"][i, :sl].double().numpy(), c["value"][i, :sl].double().numpy(),
                                         gate.double().numpy(), scale, **cfg)
            for h in range(heads):
                rest = np.delete(scores[h], taken[h])
                assert rest.size == 0 or scores[h, taken[h]].min() >= 4 * rest.max(), (i, h, scores[h])
    c["out64"] = model(c)
    return c


def paged(c, page, hole=None, seed=1):
    """The case's K / V as caches ``[N,H,page,D]`` with shuffled page ids, NaN in spare pages and behind every sequence's last
    key, and a table two columns wider than needed padded with -1.  ``hole = (sequence, page index)``: -1 from there on."""
    key, value, lens = c["key"], c["value"], c["lens"].tolist()
    heads, dim = key.shape[2:]
    need = [-(-sl // page) for sl in lens]
    ids = torch.randperm(sum(need) + 3, generator=torch.Generator().manual_seed(seed)).tolist()
    kc = torch.full((sum(need) + 3, heads, page, dim), float("nan"), dtype=key.dtype)
    vc, table = kc.clone(), torch.full((len(lens), max(need) + 2), -1, dtype=torch.int32)
    for i, sl in enumerate(lens):
        for j in range(need[i]):
            n, t = ids.pop(), min(page, sl - j * page)
            table[i, j] = n
            kc[n, :, :t], vc[n, :, :t] = key[i, j * page:j * page + t].transpose(0, 1), value[i, j * page:j * page + t].transpose(0, 1)
    if hole is not None:
        table[hole[0], hole[1]:] = -1
    return kc, vc, table


def with_gate(op, c, device="cpu"):
    op = op.to(device)
    with torch.no_grad():
        op.gate_proj.data = c["gate"].to(device)
    return op
