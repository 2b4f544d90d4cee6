"""The gated-delta-rule ops (`LINEAR_ATTN_OPS`) benchmark (standalone; not part of bench.py):
python -m benchmarks.gated_delta_bench [--out profiles/gated_delta_bench.json]

Qwen3-Next geometry: Hk 16, Hv 32, Dk = Dv 128, bf16, the l2 norm on, g and beta in fp32.  HIP events, the median of 5 timed
regions after warm-up with min and max beside it.

  decode_b64            `HIPGatedDeltaRuleUpdateState`, B 64, T 1, timed as replays of a captured graph of 20 calls.  ``sibling``
                        is `HIPSilu` (a streaming kernel: reads and writes every byte once) on a bf16 tensor of the state's
                        bytes; the op may take the sibling's time scaled by bytes read plus written, plus the sibling's own
                        min-to-max spread in this run, plus 5 % of the sibling's median (``allowed_us``, ``hip_within_margin``).
  prefill_1x8192, prefill_packed_4x2048, prefill_ragged_16 (16 packed sequences of 512 .. 1024 tokens)
                        `HIPGatedDeltaRule` with `initial_state` and `output_final_state`.  ``torch`` is the same chunked
                        algorithm as a torch composition on the GPU (bf16 `matmul`s with fp32 results, `solve_triangular`, a
                        host loop over the chunks and, for the ragged leg, over the sequences); ``torch_over_hip`` its ratio.

FLOPs of a prefill leg: the chunk algebra at C = 64 per token and value head, the key-side products counted once per value
head: K K^T, Q K^T and Tm (beta exp(G) K) 2 C Dk each, Tm (beta V) and P Vn 2 C Dv each, W S, Q S and K^T Vn 2 Dk Dv each:
``tokens * Hv * 2 * (C * (3 Dk + 2 Dv) + 3 Dk Dv)`` = 180 224 per token and head here; the triangular inverse is not counted.
One JSON object."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.extras import _hbm, _mfma, _time, _time_graph, _want, hip  # noqa: E402

BF16 = torch.bfloat16
HK, HV, DK, DV, C = 16, 32, 128, 128, 64


def _inputs(batch, tokens, device):
    q, k = (torch.randn(batch, tokens, HK, DK, device=device).to(BF16) for _ in range(2))
    v = torch.randn(batch, tokens, HV, DV, device=device).to(BF16)
    g = -F.softplus(torch.randn(batch, tokens, HV, device=device)) * 0.3
    return q, k, v, g, torch.sigmoid(torch.randn(batch, tokens, HV, device=device))


def _torch_chunked(q, k, v, g, beta, state):
    """[N, T, ...] sequences of one length through the chunk algebra; ``state`` [N, Hv, Dk, Dv] fp32.  Returns (out, state)."""
    n, tokens = q.shape[:2]
    pad = -tokens % C
    q, k, v, g, beta = (F.pad(x, (0, 0) * (x.dim() - 2) + (0, pad)) for x in (q, k, v, g, beta))
    nc, mm = (tokens + pad) // C, lambda a, b: torch.matmul(a.to(BF16), b.to(BF16)).float()    # noqa: E731
    norm = lambda x: F.normalize(x.float(), dim=-1, eps=1e-6).repeat_interleave(HV // HK, 2)     # noqa: E731
    chunks = lambda x: x.transpose(1, 2).unflatten(2, (nc, C))                                   # noqa: E731  [N, H, nc, C, ..]
    q, k, v, g, beta = chunks(norm(q)), chunks(norm(k)), chunks(v.float()), chunks(g), chunks(beta)
    big_g = g.cumsum(-1)
    low = torch.ones(C, C, dtype=torch.bool, device=q.device).tril()
    gamma = torch.where(low, torch.exp(torch.where(low, big_g[..., :, None] - big_g[..., None, :], 0.0)), 0.0)
    eye = torch.eye(C, device=q.device)
    a = (beta[..., None] * mm(k, k.transpose(-1, -2)) * gamma).tril(-1)
    tm = torch.linalg.solve_triangular(eye + a, eye.expand_as(a), upper=False)
    w, u = mm(tm, (beta * big_g.exp())[..., None] * k), mm(tm, beta[..., None] * v)
    p, qg = mm(q, k.transpose(-1, -2)) * gamma, big_g.exp()[..., None] * q
    kd = ((big_g[..., -1:] - big_g).exp()[..., None] * k).transpose(-1, -2)
    out, state = torch.empty_like(v), state.clone()
    for c in range(nc):
        vn = u[:, :, c] - mm(w[:, :, c], state)
        out[:, :, c] = DK ** -0.5 * (mm(qg[:, :, c], state) + mm(p[:, :, c], vn))
        state = big_g[:, :, c, -1].exp()[..., None, None] * state + mm(kd[:, :, c], vn)
    return out.flatten(2, 3)[:, :, :tokens].transpose(1, 2).to(BF16), state


def bench(device):
    out = {}
    prefill, update, silu = hip("MojoGatedDeltaRule")(), hip("MojoGatedDeltaRuleUpdateState")(), hip("MojoSilu")()
    if _want("decode_b64"):
        q, k, v, g, beta = _inputs(64, 1, device)
        state = torch.randn(64, HV, DK, DV, device=device) * 0.1
        like = torch.randn(state.numel() * 2, device=device).to(BF16)             # the state's bytes in bf16
        small = sum(x.numel() * x.element_size() for x in (q, k, v, v, g, beta))
        nbytes, sib_bytes = 2 * state.numel() * 4 + small, 2 * like.numel() * 2
        res = {"hip": _hbm(_time_graph(lambda: update(q, k, v, g, beta, state)), nbytes),
               "sibling": _hbm(_time_graph(lambda: silu(like)), sib_bytes), "timing": "graph"}
        sib = res["sibling"]
        res["bytes"], res["sibling_bytes"] = nbytes, sib_bytes
        res["allowed_us"] = (sib["us"] + (sib["us_max"] - sib["us_min"]) + 0.05 * sib["us"]) * nbytes / sib_bytes
        res["hip_within_margin"] = res["hip"]["us"] <= res["allowed_us"]
        out["decode_b64"] = res
        del state, like
        torch.cuda.empty_cache()
    legs = {"prefill_1x8192": [8192], "prefill_packed_4x2048": [2048] * 4,
            "prefill_ragged_16": [512 + 64 * ((5 * i) % 9) for i in range(16)]}
    for name, lengths in legs.items():
        if not _want(name):
            continue
        tokens = sum(lengths)
        q, k, v, g, beta = _inputs(1, tokens, device)
        init = torch.randn(len(lengths), HV, DK, DV, device=device) * 0.1
        cu = torch.tensor([0] + lengths, device=device).cumsum(0).to(torch.int32)
        bounds = cu.tolist()

        def composition():
            if len(set(lengths)) == 1:
                return _torch_chunked(*(x.view(len(lengths), lengths[0], *x.shape[2:]) for x in (q, k, v, g, beta)), init)
            return [_torch_chunked(*(x[:, b0:b1] for x in (q, k, v, g, beta)), init[i:i + 1])
                    for i, (b0, b1) in enumerate(zip(bounds[:-1], bounds[1:]))]

        flops = tokens * HV * 2.0 * (C * (3 * DK + 2 * DV) + 3 * DK * DV)
        res = {"hip": _mfma(_time(lambda: prefill(q, k, v, g, beta, initial_state=init, output_final_state=True,
                                                  cu_seqlens=cu if len(lengths) > 1 else None)), flops),
               "torch": _mfma(_time(composition, iters=2, warmup=1), flops), "timing": "eager", "lengths": lengths}
        res["torch_over_hip"] = res["torch"]["us"] / res["hip"]["us"]
        out[name] = res
        del q, k, v, g, beta, init
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "gated_delta_bench.json"))
    ns = ap.parse_args()
    line = json.dumps({"gated_delta": bench(torch.device("cuda", 0))})
    with open(ns.out, "w") as f:
        f.write(line + "\n")
    print(line)
