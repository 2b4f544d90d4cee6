"""The MXFP4 ops (`MXFP4_OPS`) benchmark (standalone; not part of bench.py):
python -m benchmarks.mxfp4_bench [--out profiles/mxfp4_bench.json]

HIP events, the median of 5 timed regions after warm-up with min and max beside it.  Every product leg runs `HIPMXFP4Gemm` and, in
the same run on the same ``(M, N, K)``, its sibling `HIPQuantGemm` in fp8 with ``[N, K]`` weights; both on COLD weights: every call
takes another copy of the weight (copies x bytes >= 768 MB, three times the last-level cache), which is what a model's layers see.
``allowed_us`` is the sibling's median plus its min-to-max spread plus 5 % of its median.

  tile_<M>x<K>x<N>      prefill-sized, eager launches.  ``allowed_us`` unscaled: the fp4 route must not lose to fp8.
                        ``time_vs_half_sibling`` is the stretch figure: the instruction rate predicts half the sibling's time.
  skinny_<M>x<K>x<N>    decode-sized, replays of a captured graph.  ``allowed_us`` scaled by the bytes moved (weights, scales,
                        activations, output) of the two routes.
  quant_8192x4096       `HIPMXFP4Quant` on bf16 rows against `HIPDynamicQuant` (int8, one scale per row) on the same rows, scaled
                        by bytes moved.
One JSON object."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.extras import _hbm, _mfma, _time, _time_graph, _want, hip  # noqa: E402
from mojo_opset_amd.backends.hip import lib as L  # noqa: E402

BF16, FP8 = torch.bfloat16, torch.float8_e4m3fn
TILE = [(8192, 4096, 14336), (1024, 4096, 4096), (2048, 2880, 5760)]
SKINNY = [(16, 8192, 8192), (64, 8192, 8192), (64, 2880, 5760)]
COLD_BYTES = 768 * 2 ** 20


def _allowed(sib, scale=1.0):
    return (sib["us"] + (sib["us_max"] - sib["us_min"]) + 0.05 * sib["us"]) * scale


def _rotating(ops, *args):
    turn = [0]

    def call():
        turn[0] += 1
        return ops[turn[0] % len(ops)](*args)
    return call


def _fp4_ops(m, k, n, copies, device):
    ops = []
    for _ in range(copies):
        op = hip("MojoMXFP4Gemm")(k, n, BF16)
        op.weight = torch.randint(0, 256, (n, k // 2), dtype=torch.uint8, device=device)
        op.weight_scale = torch.randint(120, 128, (n, k // 32), device=device).to(torch.uint8)
        ops.append(op)
    a = torch.randint(0, 256, (m, k // 2), dtype=torch.uint8, device=device)
    return ops, a, torch.randint(120, 128, (m, k // 32), device=device).to(torch.uint8)


def _fp8_ops(m, k, n, copies, device):
    ops = []
    for _ in range(copies):
        op = hip("MojoQuantGemm")(k, n, output_dtype=BF16, trans_weight=True, quant_dtype=FP8, weight_dtype=FP8)
        op.weight = torch.randn(n, k, device=device).to(FP8)
        op.weight_scale = (torch.rand(n, device=device) * 0.01 + 0.01).to(BF16)
        ops.append(op)
    return ops, torch.randn(m, k, device=device).to(FP8), torch.rand(m, device=device) * 0.01 + 0.01


def product_leg(m, k, n, skinny, device):
    timer = (lambda fn, copies: _time_graph(fn, reps=max(10, copies))) if skinny else (lambda fn, copies: _time(fn))
    flops = 2.0 * m * k * n
    copies4, copies8 = (max(2, -(-COLD_BYTES // b)) for b in (n * k // 2, n * k))
    ops, a, sa = _fp4_ops(m, k, n, copies4, device)
    res = {"hip": _mfma(timer(_rotating(ops, a, sa), copies4), flops), "kernel_form": L.last_launch(), "weight_copies": copies4}
    del ops
    torch.cuda.empty_cache()
    ops, x, sx = _fp8_ops(m, k, n, copies8, device)
    res["sibling"] = _mfma(timer(_rotating(ops, x, sx), copies8), flops)
    res["sibling_form"] = L.last_launch()
    del ops
    torch.cuda.empty_cache()
    scale = 1.0
    if skinny:
        res["bytes"] = n * k // 2 + n * k // 32 + m * k // 2 + m * k // 32 + m * n * 2
        res["sibling_bytes"] = n * k + n * 2 + m * k + m * 4 + m * n * 2
        scale = res["bytes"] / res["sibling_bytes"]
    else:
        res["time_vs_half_sibling"] = res["hip"]["us"] / (0.5 * res["sibling"]["us"])
    res["allowed_us"] = _allowed(res["sibling"], scale)
    res["hip_within_margin"] = res["hip"]["us"] <= res["allowed_us"]
    return res


def bench(device):
    out = {}
    for skinny, shapes in ((False, TILE), (True, SKINNY)):
        for m, k, n in shapes:
            name = f"{'skinny' if skinny else 'tile'}_{m}x{k}x{n}"
            if _want(name):
                out[name] = product_leg(m, k, n, skinny, device)
    if _want("quant_8192x4096"):
        m, k = 8192, 4096
        x = torch.randn(m, k, device=device).to(BF16)
        quant, sibling = hip("MojoMXFP4Quant")(), hip("MojoDynamicQuant")()
        nbytes, sib_bytes = m * k * 2 + m * k // 2 + m * k // 32, m * k * 2 + m * k + m * 4
        res = {"hip": _hbm(_time(lambda: quant(x)), nbytes), "sibling": _hbm(_time(lambda: sibling(x)), sib_bytes),
               "bytes": nbytes, "sibling_bytes": sib_bytes}
        res["allowed_us"] = _allowed(res["sibling"], nbytes / sib_bytes)
        res["hip_within_margin"] = res["hip"]["us"] <= res["allowed_us"]
        out["quant_8192x4096"] = res
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "mxfp4_bench.json"))
    ns = ap.parse_args()
    line = json.dumps({"mxfp4": bench(torch.device("cuda", 0))})
    with open(ns.out, "w") as f:
        f.write(line + "\n")
    print(line)
