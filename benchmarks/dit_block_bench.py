"""The DiT block ops (`DIT_BLOCK_OPS`) benchmark (standalone; not part of bench.py):
python -m benchmarks.dit_block_bench

Wan2.2-14B geometry in bf16, HIP events: 75 600 tokens x 5120 (and 4096 rows) for the norms, the FFN's 75 600 x 13 824 for GELU,
75 600 x 5120 for SiLU, q of 40 heads x 128 for grid RoPE on the (21, 45, 80) grid and on a batch of two (21, 30, 52) grids with
8 padding tokens.  Per op, in one process:

  hip        the HIP<Op>
  torch      the torch composition of its golden, on the GPU
  sibling    the nearest existing kernel: `MojoRMSNorm` / `MojoResidualAddRMSNorm` on the same rows (the same bytes) for the two
             norms, `MojoSwiGLU` (two reads and a write per element, against one and one) for the activations, `MojoApplyRoPE`
             with rope_dim = head_dim on the same q (and a k of one head, which it cannot do without) for grid RoPE

Every figure is the median of 5 timed regions after warm-up (min and max beside it); bytes are ALGORITHMIC (each input and output
element once; weight, bias and the frequency rows are cache-resident and left out).  The norms move their sibling's bytes, so
they are judged on time: ``hip_minus_sibling_us`` against ``sibling_spread_us`` (the sibling's own min-to-max in this run) plus 5 %
of the sibling's median.  The others move other bytes than their sibling, so they are judged on bytes per second with the same
margin, turned into the time the op may take at the sibling's rate (``allowed_us``).  One JSON object."""
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.extras import _hbm, _time, _want, hip  # noqa: E402

TOKENS, HIDDEN, FFN, HEADS, HEAD_DIM = 75600, 5120, 13824, 40, 128
BF16 = torch.bfloat16


def _judge(res, same_bytes):
    if "sibling" in res:
        sib = res["sibling"]
        res["sibling_spread_us"] = sib["us_max"] - sib["us_min"]
        # the time the op may take: the sibling's time for the op's bytes, plus the sibling's spread and 5 % of its median
        at_rate = sib["us"] if same_bytes else sib["us"] * res["bytes"] / res["sibling_bytes"]
        scale = 1.0 if same_bytes else res["bytes"] / res["sibling_bytes"]
        res["allowed_us"] = at_rate + (res["sibling_spread_us"] + 0.05 * sib["us"]) * scale
        res["hip_minus_sibling_us"] = res["hip"]["us"] - at_rate
        res["hip_within_margin"] = res["hip"]["us"] <= res["allowed_us"]
    res["torch_over_hip"] = res["torch"]["us"] / res["hip"]["us"]
    return res


def _param(op, **values):
    with torch.no_grad():
        for k, v in values.items():
            getattr(op, k).copy_(v)
    return op


def _run(cases, out):
    for name, (nbytes, sibling_bytes, legs) in cases.items():
        if not _want(name):
            continue
        res = {leg: _hbm(_time(fn), sibling_bytes if leg == "sibling" else nbytes) for leg, fn in legs.items()}
        res["bytes"], res["sibling_bytes"] = nbytes, sibling_bytes
        out[name] = _judge(res, nbytes == sibling_bytes)
    torch.cuda.empty_cache()


def norm_cases(device, rows, out):
    x = torch.randn(rows, HIDDEN, device=device, dtype=BF16)
    r = torch.randn(rows, HIDDEN, device=device, dtype=BF16)
    w, b = torch.randn(HIDDEN, device=device, dtype=BF16), torch.randn(HIDDEN, device=device, dtype=BF16)
    n = rows * HIDDEN * 2
    kw = dict(dtype=BF16, device=device)
    ln = _param(hip("MojoLayerNorm")(HIDDEN, **kw), weight=w, bias=b)
    bare = hip("MojoLayerNorm")(HIDDEN, 1e-6, False, **kw)
    add_ln = _param(hip("MojoResidualAddLayerNorm")(HIDDEN, **kw), weight=w, bias=b)
    rms = _param(hip("MojoRMSNorm")(HIDDEN, **kw), weight=w)
    add_rms = _param(hip("MojoResidualAddRMSNorm")(HIDDEN, **kw), weight=w)
    _run({
        f"layernorm_{rows}x{HIDDEN}": (2 * n, 2 * n, {
            "hip": lambda: ln(x), "sibling": lambda: rms(x), "torch": lambda: F.layer_norm(x, (HIDDEN,), w, b, 1e-5)}),
        f"layernorm_no_affine_{rows}x{HIDDEN}": (2 * n, 2 * n, {
            "hip": lambda: bare(x), "sibling": lambda: rms(x), "torch": lambda: F.layer_norm(x, (HIDDEN,), None, None, 1e-6)}),
        f"add_layernorm_{rows}x{HIDDEN}": (4 * n, 4 * n, {
            "hip": lambda: add_ln(x, r), "sibling": lambda: add_rms(x, r),
            "torch": lambda: F.layer_norm(x + r, (HIDDEN,), w, b, 1e-5)}),
    }, out)


def activation_cases(device, out):
    swiglu = hip("MojoSwiGLU")()
    for name, cols, op, golden in (("gelu", FFN, hip("MojoGelu")(), F.gelu), ("silu", HIDDEN, hip("MojoSilu")(), F.silu)):
        x = torch.randn(TOKENS, cols, device=device, dtype=BF16)
        u = torch.randn(TOKENS, cols, device=device, dtype=BF16)
        n = TOKENS * cols * 2
        _run({f"{name}_{TOKENS}x{cols}": (2 * n, 3 * n, {
            "hip": lambda: op(x), "sibling": lambda: swiglu(x, u), "torch": lambda: golden(x)})}, out)
        del x, u


def _frequencies(cells, device):
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, HEAD_DIM, 2, dtype=torch.float32, device=device) / HEAD_DIM))
    angle = torch.arange(cells, dtype=torch.float32, device=device)[:, None] * inv_freq[None, :]
    return torch.complex(angle.cos()[:, None, :], angle.sin()[:, None, :])


def _golden_grid_rope(x, grids, freqs_list):
    out = []
    for i, (f, h, w) in enumerate(grids):
        cells = f * h * w
        turned = torch.view_as_complex(x[i, :cells].float().reshape(cells, x.shape[2], -1, 2)) * freqs_list[i]
        out.append(torch.cat([torch.view_as_real(turned).flatten(2), x[i, cells:]]))
    return torch.stack(out).type_as(x)


def rope_cases(device, out):
    rope, apply_rope = hip("MojoGridRoPE")(), hip("MojoApplyRoPE")()
    for name, grids, pad in (("grid_rope_1x75600", [(21, 45, 80)], 0), ("grid_rope_2x32768", [(21, 30, 52)] * 2, 8)):
        cells = grids[0][0] * grids[0][1] * grids[0][2]
        tokens = cells + pad
        x = torch.randn(len(grids), tokens, HEADS, HEAD_DIM, device=device, dtype=BF16)
        k = torch.randn(len(grids), tokens, 1, HEAD_DIM, device=device, dtype=BF16)
        grid = torch.tensor(grids, dtype=torch.int32, device=device)
        freqs = [_frequencies(cells, device)] * len(grids)
        cos = torch.randn(tokens, HEAD_DIM, device=device)
        sin = torch.randn(tokens, HEAD_DIM, device=device)
        n = x.numel() * 2
        _run({name: (2 * n, 2 * (n + k.numel() * 2), {
            "hip": lambda: rope(x, grid, freqs), "sibling": lambda: apply_rope(x, k, cos, sin, head_first=False),
            "torch": lambda: _golden_grid_rope(x, grids, freqs)})}, out)
        del x, k


def bench(device):
    out = {}
    for rows in (TOKENS, 4096):
        norm_cases(device, rows, out)
    activation_cases(device, out)
    rope_cases(device, out)
    return out


if __name__ == "__main__":
    print(json.dumps({"dit_block": bench(torch.device("cuda", 0))}))
