"""The MXFP4 MoE experts (`MXFP4_MOE_OPS`) benchmark (standalone; not part of bench.py):
python -m benchmarks.mxfp4_moe_bench [--out profiles/mxfp4_moe_bench.json]

HIP events, the median of 5 timed regions after warm-up with min and max beside it.  Every leg runs, in the same process on the same
shape and the same row counts (a multinomial split of the routed rows over the experts, seeded):

  experts   `HIPMXFP4Experts` against its W8A8 sibling `HIPQuantExperts`.  ``allowed_us`` is the sibling's median plus its
            min-to-max spread plus 5 % of its median; ``hip_within_margin`` says whether the fp4 experts stay inside it.
  fc1       `HIPMXFP4GroupGemm(swiglu_quant=True)` against the unfused pair, `HIPMXFP4GroupGemm` with a bf16 output followed by
            `HIPMXFP4SwiGLUQuant`; ``fused_over_unfused`` is the ratio of the medians.

  gpt_oss_prefill   E 128, hidden 2880, I 2880, 16384 routed rows, eager launches
  mixtral_prefill   E 8, hidden 4096, I 14336, 8192 rows, eager launches
  decode            E 128, hidden 2880, I 2880, 512 rows (4 per expert on average), replays of a captured graph
The weights of a leg (0.7 to 1.6 GB in fp4) exceed the last-level cache, so every call streams them from HBM.  Operations are
ALGORITHMIC: 6 * rows * hidden * I.  MOJO_BENCH_ONLY=<substring> runs one leg.  One JSON object."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.extras import _mfma, _time, _time_graph, _want, hip  # noqa: E402
from mojo_opset_amd.backends.hip import lib as L  # noqa: E402

BF16 = torch.bfloat16
LEGS = {"gpt_oss_prefill": (128, 2880, 2880, 16384, False), "mixtral_prefill": (8, 4096, 14336, 8192, False),
        "decode": (128, 2880, 2880, 512, True)}


def _bytes(shape, device, lo=0, hi=256):
    return torch.randint(lo, hi, shape, device=device).to(torch.uint8)


def _fp4_experts(e, h, i, device):
    op = hip("MojoMXFP4Experts")(e, h, i)
    op.up_proj_weight, op.up_proj_weight_scale = _bytes((e, 2 * i, h // 2), device), _bytes((e, 2 * i, h // 32), device, 116, 122)
    op.down_proj_weight, op.down_proj_weight_scale = _bytes((e, h, i // 2), device), _bytes((e, h, i // 32), device, 116, 122)
    return op


def _w8a8_experts(e, h, i, device):
    op = hip("MojoQuantExperts")(num_experts=e, hidden_size=h, intermediate_size=i).to(device)
    with torch.no_grad():
        op.up_proj_weight.copy_(torch.randint(-127, 128, (e, 2 * i, h), device=device).to(torch.int8))
        op.down_proj_weight.copy_(torch.randint(-127, 128, (e, h, i), device=device).to(torch.int8))
        op.up_proj_weight_scale.copy_(torch.rand(e, 2 * i, device=device) * 1e-4 + 1e-4)
        op.down_proj_weight_scale.copy_(torch.rand(e, h, device=device) * 1e-4 + 1e-4)
        op.up_proj_quantize.inv_smooth_scale.fill_(1.0)
        op.down_proj_quantize.inv_smooth_scale.fill_(1.0)
    return op


def leg(e, h, i, rows, graph, device):
    timer = (lambda fn: _time_graph(fn, reps=10)) if graph else _time
    gen = torch.Generator().manual_seed(e * 31 + rows)
    probs = torch.softmax(torch.randn(e, generator=gen) * 0.5, 0)
    counts = torch.bincount(torch.multinomial(probs, rows, replacement=True, generator=gen), minlength=e).to(torch.int32).to(device)
    x = torch.randn(rows, h, device=device).to(BF16)
    flops = 6.0 * rows * h * i
    res = {"rows_per_expert": {"min": int(counts.min()), "max": int(counts.max()), "over_32": int((counts > 32).sum())}}
    fp4 = _fp4_experts(e, h, i, device)
    res["hip"] = _mfma(timer(lambda: fp4(x, counts)), flops)
    res["kernel_form"] = L.last_launch()
    # fc1 alone, on the experts' own weights: fused epilogue against product + stand-alone stage
    a, sa = hip("MojoMXFP4Quant")()(x)
    fused, plain = (hip("MojoMXFP4GroupGemm")(e, h, 2 * i, BF16, swiglu_quant=flag) for flag in (True, False))
    for op in (fused, plain):
        op.weight, op.weight_scale = fp4.up_proj_weight, fp4.up_proj_weight_scale
    stage = hip("MojoMXFP4SwiGLUQuant")()
    res["fc1_fused"] = _mfma(timer(lambda: fused(a, sa, counts)), 4.0 * rows * h * i)
    res["fc1_unfused"] = _mfma(timer(lambda: stage(plain(a, sa, counts))), 4.0 * rows * h * i)
    res["fused_over_unfused"] = res["fc1_fused"]["us"] / res["fc1_unfused"]["us"]
    del fp4, fused, plain
    torch.cuda.empty_cache()
    w8a8 = _w8a8_experts(e, h, i, device)
    sib = res["sibling"] = _mfma(timer(lambda: w8a8(x, counts)), flops)
    res["allowed_us"] = sib["us"] + (sib["us_max"] - sib["us_min"]) + 0.05 * sib["us"]
    res["hip_within_margin"] = res["hip"]["us"] <= res["allowed_us"]
    del w8a8
    torch.cuda.empty_cache()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "mxfp4_moe_bench.json"))
    ns = ap.parse_args()
    device = torch.device("cuda", 0)
    line = json.dumps({"mxfp4_moe": {name: leg(*shape, device) for name, shape in LEGS.items() if _want(name)}})
    with open(ns.out, "w") as f:
        f.write(line + "\n")
    print(line)
