"""The dense W8A8 quantiser ops (`QUANT_DENSE_OPS`) benchmark (standalone; not part of bench.py):
python -m benchmarks.quant_dense_bench

bf16 activations, int8 out, HIP events, rows 64 and 8192 at hidden 4096; the fc1 -> fc2 stage at I = 14336 with one group and
with 8 groups of 1024 rows, on int32 accumulators and on bf16.  Per op, in one process:

  hip        the HIP<Op>
  torch      the torch composition of its golden, on the GPU (several launches, fp32 intermediates in memory)
  sibling    the nearest existing kernel on the same bytes: `MojoResidualAddRMSNormQuant` (pre) for the residual-add LayerNorm,
             its kernel without a residual (`MojoRMSNormQuant`) for the plain LayerNorm, `MojoDynamicQuant` for the static
             quantiser, `mojo_hip_moe_dynamic_quant` with glu = 1 for the SwiGLU stage on 16-bit input (none reads int32; the
             dequantiser has none either)

Every figure is the median of 5 timed regions after warm-up (min and max beside it); bytes are ALGORITHMIC (each input and output
element once; the per-column vectors are cache-resident and left out).  ``hip_minus_sibling_us`` against ``sibling_spread_us`` (the
sibling's own min-to-max in this run) says whether a difference is inside the yardstick's noise.  One JSON object."""
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.extras import _hbm, _time, _want, hip  # noqa: E402
from mojo_opset_amd.backends.hip.operators.quantize import moe_dynamic_quant  # noqa: E402

HIDDEN, INTER = 4096, 14336
BF16, I8 = torch.bfloat16, torch.int8


def _quantise(y):
    scale = y.abs().amax(dim=-1, keepdim=True).clamp(min=1e-12) / 127
    return torch.clamp(torch.round(y / scale), -128, 127).to(I8), scale


def _judge(res):
    if "sibling" in res:
        res["hip_minus_sibling_us"] = res["hip"]["us"] - res["sibling"]["us"]
        res["sibling_spread_us"] = res["sibling"]["us_max"] - res["sibling"]["us_min"]
        res["hip_within_sibling_spread"] = res["hip_minus_sibling_us"] <= res["sibling_spread_us"]
    res["torch_over_hip"] = res["torch"]["us"] / res["hip"]["us"]
    return res


def _param(op, **values):
    with torch.no_grad():
        for k, v in values.items():
            getattr(op, k).copy_(v)
    return op


def norm_cases(device, rows, out):
    x = torch.randn(rows, HIDDEN, device=device, dtype=BF16)
    r = torch.randn(rows, HIDDEN, device=device, dtype=BF16)
    w, b = torch.randn(HIDDEN, device=device), torch.randn(HIDDEN, device=device)
    n = rows * HIDDEN
    rms = _param(hip("MojoRMSNormQuant")(HIDDEN).to(device), weight=w)
    ln = _param(hip("MojoLayerNormQuant")(HIDDEN).to(device), weight=w, bias=b)
    add_ln = _param(hip("MojoResidualAddLayerNormQuant")(HIDDEN).to(device), weight=w, bias=b)
    add_rms = _param(hip("MojoResidualAddRMSNormQuant")(HIDDEN).to(device), weight=w)
    plain_bytes, add_bytes = n * 3 + rows * 4, n * 7 + rows * 4
    cases = {
        f"rmsnorm_quant_{rows}x{HIDDEN}": (plain_bytes, {
            "hip": lambda: rms(x),
            "torch": lambda: _quantise(F.rms_norm(x.float(), [HIDDEN], weight=w, eps=1e-5))}),
        f"layernorm_quant_{rows}x{HIDDEN}": (plain_bytes, {
            "hip": lambda: ln(x), "sibling": lambda: rms(x),
            "torch": lambda: _quantise(F.layer_norm(x.float(), [HIDDEN], weight=w, bias=b, eps=1e-5))}),
        f"add_layernorm_quant_{rows}x{HIDDEN}": (add_bytes, {
            "hip": lambda: add_ln(x, r), "sibling": lambda: add_rms(x, r),
            "torch": lambda: _quantise(F.layer_norm((x + r).float(), [HIDDEN], weight=w, bias=b, eps=1e-5))}),
    }
    _run(cases, out)


def elementwise_cases(device, rows, out):
    x = torch.randn(rows, HIDDEN, device=device, dtype=BF16)
    scale = torch.rand(HIDDEN, device=device) * 0.02 + 0.01
    n = rows * HIDDEN
    static = _param(hip("MojoStaticQuant")(HIDDEN).to(device), scale=scale)
    dynamic = hip("MojoDynamicQuant")()
    dequant = hip("MojoDequant")(output_dtype=BF16)
    q, token_scale = dynamic(x)
    cases = {
        f"static_quant_{rows}x{HIDDEN}": (n * 3, {
            "hip": lambda: static(x), "sibling": lambda: dynamic(x),
            "torch": lambda: torch.clamp(torch.round(x.float() / scale), -128, 127).to(I8)}),
        f"dequant_trailing_{rows}x{HIDDEN}": (n * 3, {
            "hip": lambda: dequant(q, scale), "torch": lambda: (q.float() * scale).to(BF16)}),
        f"dequant_token_{rows}x{HIDDEN}": (n * 3 + rows * 4, {
            "hip": lambda: dequant(q, token_scale), "torch": lambda: (q.float() * token_scale).to(BF16)}),
    }
    _run(cases, out)


def swiglu_cases(device, rows, groups, out):
    counts = torch.full((groups,), rows // groups, dtype=torch.int32, device=device)
    expert = torch.arange(groups, device=device).repeat_interleave(rows // groups)
    ws = torch.rand(groups, 2 * INTER, device=device) * 0.008 + 0.001
    qs = torch.rand(groups, INTER, device=device) + 0.5
    act = torch.rand(rows, device=device) * 0.3 + 0.05
    stage = _param(hip("MojoDequantSwiGLUQuant")(groups, INTER).to(device), weight_scale=ws, quant_scale=qs)
    token_count = counts if groups > 1 else None

    def composition(x):
        y = x.float() * ws[expert] * act.unsqueeze(-1)
        left, right = y.chunk(2, dim=-1)
        return _quantise(F.silu(right) * left * qs[expert])

    cases = {}
    for name, dtype in (("int32", torch.int32), ("bf16", BF16)):
        acc = (torch.randn(rows, 2 * INTER, device=device) * 3000).round()
        x = acc.to(torch.int32) if dtype == torch.int32 else (acc / 64).to(BF16)
        del acc
        nbytes = rows * INTER * (2 * x.element_size() + 1) + rows * 8
        legs = {"hip": lambda x=x: stage(x, act, None, None, token_count), "torch": lambda x=x: composition(x)}
        if dtype == BF16:
            legs["sibling"] = lambda x=x: moe_dynamic_quant(x, qs, counts, INTER, True, "bench")
        cases[f"dequant_swiglu_quant_{name}_{rows}x{INTER}_g{groups}"] = (nbytes, legs)
    _run(cases, out)


def _run(cases, out):
    for name, (nbytes, legs) in cases.items():
        if not _want(name):
            continue
        res = {leg: _hbm(_time(fn), nbytes) for leg, fn in legs.items()}
        res["bytes"] = nbytes
        out[name] = _judge(res)
    torch.cuda.empty_cache()


def bench(device):
    out = {}
    for rows in (64, 8192):
        norm_cases(device, rows, out)
        elementwise_cases(device, rows, out)
        swiglu_cases(device, rows, 1, out)
    swiglu_cases(device, 8192, 8, out)
    return out


if __name__ == "__main__":
    print(json.dumps({"quant_dense": bench(torch.device("cuda", 0))}))
