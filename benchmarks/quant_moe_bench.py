"""W8A8 MoE experts benchmark (standalone; not part of bench.py): python benchmarks/quant_moe_bench.py

`MojoQuantExperts` next to `MojoExperts` on the shapes benchmarks/extras.py:bench_moe reports for the bf16 experts, the two
legs alternated in the same process, five medians per leg (their spread is reported):

* prefill: T 8192 x top-2, E 8, H 4096, I 14336 (HIP events);
* decode: T 64, top-8 of 64 experts, H 4096, I 2048 by graph replay — the experts alone and the whole layer (gating ->
  dispatch -> experts -> combine, the chain `MojoQuantMoE` / `MojoMoE` run);
* one DeepSeek-V3-like local slice: E 32, H 7168, I 2048, 4096 rows (HIP events).

Bytes and integer operations are ALGORITHMIC, computed from the shapes below.  MOJO_BENCH_ONLY=<substring> runs one case.
One JSON object."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.extras import _time, _time_graph, _want, hip  # noqa: E402

LEGS = 5


def quantize_rows(w):
    scale = (w.float().abs().amax(dim=-1, keepdim=True) / 127).clamp(min=1e-12)
    return torch.round(w.float() / scale).clamp(-128, 127).to(torch.int8), scale.squeeze(-1).to(torch.bfloat16)


def make_experts(device, e, h, i, std=0.02):
    """bf16 experts and int8 experts holding the SAME weights (quantised per output channel, amax / 127)."""
    bf = hip("MojoExperts")(num_experts=e, hidden_size=h, intermediate_size=i).to(torch.bfloat16).to(device)
    q8 = hip("MojoQuantExperts")(num_experts=e, hidden_size=h, intermediate_size=i).to(device)
    with torch.no_grad():
        bf.up_proj_weight.normal_(std=std)
        bf.down_proj_weight.normal_(std=std)
        for x in range(e):                                     # one expert at a time: the fp32 copy of a weight set is large
            q8.up_proj_weight[x], q8.up_proj_weight_scale[x] = quantize_rows(bf.up_proj_weight[x])
            q8.down_proj_weight[x], q8.down_proj_weight_scale[x] = quantize_rows(bf.down_proj_weight[x])
        q8.up_proj_quantize.inv_smooth_scale.copy_(1.0 / (torch.rand(e, h, device=device) + 0.5))
        q8.down_proj_quantize.inv_smooth_scale.copy_(1.0 / (torch.rand(e, i, device=device) + 0.5))
    return bf, q8


def legs(f16, f8, timer):
    t16, t8 = [], []
    for _ in range(LEGS):                                      # alternated legs
        t16.append(timer(f16))
        t8.append(timer(f8))
    return t16, t8


def report(t16, t8, rows, h, i, weight_elems):
    """weight_elems: elements of the expert weights that are read (every expert with rows: 3 * H * I each)."""
    m16, m8 = statistics.median(t16), statistics.median(t8)
    ops = 2.0 * rows * h * (2 * i) + 2.0 * rows * i * h
    # bf16 (fused first projection + SwiGLU): weights, x read, the [M, I] activation written and read, out written
    bytes16 = weight_elems * 2 + rows * h * 2 + 2 * rows * i * 2 + rows * h * 2
    # int8: weights once; x read (2 B) and written as int8; fc1 [M, 2I] written and read in 16 bits; act int8 written and read; out
    bytes8 = weight_elems + rows * (3 * h + 5 * i) + rows * h + rows * i + rows * h * 2
    spread = max(max(t16) - min(t16), max(t8) - min(t8))
    return {
        "bf16": {"us": m16 * 1e6, "us_legs": [t * 1e6 for t in t16], "spread_us": (max(t16) - min(t16)) * 1e6,
                 "tflops": ops / m16 / 1e12, "bytes": bytes16, "GB/s": bytes16 / m16 / 1e9},
        "int8": {"us": m8 * 1e6, "us_legs": [t * 1e6 for t in t8], "spread_us": (max(t8) - min(t8)) * 1e6,
                 "tops": ops / m8 / 1e12, "bytes": bytes8, "GB/s": bytes8 / m8 / 1e9},
        "integer_ops": ops, "int8_over_bf16_time": m8 / m16, "bytes_predict": bytes8 / bytes16,
        "faster_by_more_than_the_spread": (m16 - m8) > spread,
    }


def routed_rows(device, tokens, e, k, h, seed, uniform=False):
    """Rows sorted by expert and their counts, through the package's own gating and dispatch (zero-mean inputs spread the routing)."""
    torch.manual_seed(seed)
    x = (torch.rand if uniform else torch.randn)(tokens, h, device=device, dtype=torch.bfloat16)
    gating = hip("MojoMoEGating")(hidden_size=h, num_experts=e, top_k=k).to(device)
    with torch.no_grad():
        gating.gate_weight.copy_(torch.randn(h, e) * 0.02)
    idx, gates = gating(x)
    rows, counts, _, _ = hip("MojoMoEDispatch")(num_experts=e)(x, gates, idx)
    return x, gating, rows, counts


def bench_prefill(device):
    out = {}
    for name, (tokens, e, k, h, i, seed, uniform) in {"experts_T8192x2_E8_H4096_I14336": (8192, 8, 2, 4096, 14336, 20260716, True),
                                                      "experts_rows4096_E32_H7168_I2048": (512, 32, 8, 7168, 2048, 20260718, False)}.items():
        if not _want(name):
            continue
        _, _, rows, counts = routed_rows(device, tokens, e, k, h, seed, uniform)
        bf, q8 = make_experts(device, e, h, i)
        t16, t8 = legs(lambda: bf(rows, counts), lambda: q8(rows, counts), lambda f: _time(f, 5, 1))
        used = int((counts > 0).sum())
        out[name] = report(t16, t8, rows.shape[0], h, i, used * 3 * h * i)
        out[name]["rows"], out[name]["experts_with_rows"] = rows.shape[0], used
        del bf, q8
        torch.cuda.empty_cache()
    return out


def bench_decode(device):
    name = "moe_layer_decode_T64_E64_k8_H4096_I2048"
    if not _want(name):
        return {}
    tokens, e, k, h, i = 64, 64, 8, 4096, 2048
    x, gating, rows, counts = routed_rows(device, tokens, e, k, h, 20260717)
    bf, q8 = make_experts(device, e, h, i)
    used = int((counts > 0).sum())                             # (read once, outside the timed region)
    timer = lambda f: _time_graph(f, reps=5, replays=3)        # noqa: E731
    t16, t8 = legs(lambda: bf(rows, counts), lambda: q8(rows, counts), timer)
    res = {"experts_only": report(t16, t8, rows.shape[0], h, i, used * 3 * h * i), "experts_with_rows": used}
    dispatch, combine = hip("MojoMoEDispatch")(num_experts=e), hip("MojoMoECombine")()
    buf = torch.empty_like(x)

    def layer(experts):
        def run():
            i2, g2 = gating(x)
            a, c, b, d = dispatch(x, g2, i2)
            return combine(buf, experts(a, c), b, d)
        return run
    t16, t8 = legs(layer(bf), layer(q8), timer)
    res["layer"] = report(t16, t8, rows.shape[0], h, i, used * 3 * h * i)
    return {name: res}


if __name__ == "__main__":
    dev = torch.device("cuda", 0)
    print(json.dumps({"quant_experts_prefill": bench_prefill(dev), "quant_moe_decode": bench_decode(dev)}))
