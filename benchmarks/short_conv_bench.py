"""The short-convolution ops (`SHORT_CONV_OPS`) benchmark (standalone; not part of bench.py):
python -m benchmarks.short_conv_bench [--out profiles/short_conv_bench.json]

Legs, bf16, W 4, SiLU, D 8192 (the convolution width of Qwen3-Next's GatedDeltaNet layers), HIP events:

  decode_b64_<time|channel>        `HIPCausalConv1dUpdateState`, B 64, T 1, state of 4 columns updated in place; ``time`` is the
                                   dense ``[B, D, 1]`` column, ``channel`` the transposed view of a ``[B, 1, D]`` projection output
  prefill_packed_4x2048            `HIPCausalConv1d` on 4 packed sequences of 2048 tokens with `initial_state` and
                                   `output_final_state`
  prefill_1x12291_<time|channel>   `HIPCausalConv1dUpdateState` on one sequence of 12 291 tokens (the reference's largest test), as
                                   ``[1, D, T]`` and as the transposed view of ``[1, T, D]``

Per leg, in one process: ``hip`` the op, ``sibling`` `HIPSilu` on a tensor of the output's size (a streaming kernel: reads and
writes every byte once), ``torch`` the reference's composition (``cat``, ``conv1d``, slice, ``silu``, ``copy_``; for the packed leg a
host loop over the sequences in fp32, as the reference's function computes it).

Every figure is the median of 5 timed regions after warm-up (min and max beside it).  The decode legs (``"timing": "graph"``)
are timed as replays of a captured graph of 20 calls, for every column alike: an eager loop there measures the Python shim, not
the kernels.  Judged as benchmarks/embedding_bench.py judges: an op may take its sibling's time scaled by bytes read plus bytes
written, plus the sibling's own min-to-max spread in this run, plus 5 % of the sibling's median (``allowed_us``,
``hip_within_margin``).  One JSON object."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.extras import _hbm, _time, _time_graph, _want, hip  # noqa: E402

BF16 = torch.bfloat16
DIM, WIDTH = 8192, 4


def _judge(res, nbytes, sibling_bytes):
    sibling = res["sibling"]
    scale = nbytes / sibling_bytes
    res["bytes"], res["sibling_bytes"] = nbytes, sibling_bytes
    res["allowed_us"] = (sibling["us"] + (sibling["us_max"] - sibling["us_min"]) + 0.05 * sibling["us"]) * scale
    res["hip_minus_sibling_us"] = res["hip"]["us"] - sibling["us"] * scale
    res["hip_within_margin"] = res["hip"]["us"] <= res["allowed_us"]
    res["torch_over_hip"] = res["torch"]["us"] / res["hip"]["us"]
    return res


def _torch_update(hidden, state, weight, bias):
    cat = torch.cat([state, hidden], dim=-1)
    state.copy_(cat[:, :, -state.shape[-1]:])
    out = F.conv1d(cat, weight.unsqueeze(1), bias, padding=0, groups=weight.shape[0])
    return F.silu(out[:, :, -hidden.shape[-1]:])


def _torch_packed(x, weight, bias, init, bounds):
    w, b = weight.float().unsqueeze(1), bias.float()
    outs, states = [], []
    for n, (bos, eos) in enumerate(bounds):
        cat = torch.cat([init[n:n + 1].float(), x[:, bos:eos].transpose(1, 2).float()], dim=-1)
        outs.append(F.silu(F.conv1d(cat, w, b, padding=0, groups=w.shape[0])).to(x.dtype).transpose(1, 2))
        states.append(cat[:, :, -(w.shape[-1] - 1):].to(x.dtype))
    return torch.cat(outs, dim=1), torch.cat(states, dim=0)


def bench(device):
    out = {}
    silu = hip("MojoSilu")()
    update = hip("MojoCausalConv1dUpdateState")()
    conv = hip("MojoCausalConv1d")()
    weight = (torch.randn(DIM, WIDTH, device=device) * 0.5).to(BF16)
    bias = torch.randn(DIM, device=device).to(BF16)
    taps = weight.numel() * 2 + bias.numel() * 2

    def update_leg(name, batch, seq, layout, timer, timing):
        if not _want(name):
            return
        if layout == "time":
            hidden = torch.randn(batch, DIM, seq, device=device).to(BF16)
        else:
            hidden = torch.randn(batch, seq, DIM, device=device).to(BF16).transpose(1, 2)
        state = torch.randn(batch, DIM, WIDTH, device=device).to(BF16)
        like = torch.randn(batch * seq, DIM, device=device).to(BF16)
        dense = hidden.contiguous()                                    # the composition's conv1d wants the literal layout
        nbytes = 2 * hidden.numel() * 2 + 2 * state.numel() * 2 + taps
        sib_bytes = 2 * like.numel() * 2
        res = {"hip": _hbm(timer(lambda: update(hidden, state, weight, bias, "silu")), nbytes),
               "sibling": _hbm(timer(lambda: silu(like)), sib_bytes),
               "torch": _hbm(timer(lambda: _torch_update(dense, state, weight, bias)), nbytes), "timing": timing}
        out[name] = _judge(res, nbytes, sib_bytes)
        del hidden, state, like, dense
        torch.cuda.empty_cache()

    for layout in ("time", "channel"):
        update_leg(f"decode_b64_{layout}", 64, 1, layout, _time_graph, "graph")
    if _want("prefill_packed_4x2048"):
        tokens = 4 * 2048
        x = torch.randn(1, tokens, DIM, device=device).to(BF16)
        init = torch.randn(4, DIM, WIDTH - 1, device=device).to(BF16)
        cu = torch.arange(0, tokens + 1, 2048, device=device, dtype=torch.int32)
        bounds = [(n * 2048, (n + 1) * 2048) for n in range(4)]
        nbytes = 2 * x.numel() * 2 + 2 * init.numel() * 2 + taps
        sib_bytes = 2 * x.numel() * 2
        like = x.view(tokens, DIM)
        res = {"hip": _hbm(_time(lambda: conv(x, weight, bias=bias, initial_state=init, output_final_state=True, activation="silu",
                                              cu_seqlens=cu)), nbytes),
               "sibling": _hbm(_time(lambda: silu(like)), sib_bytes),
               "torch": _hbm(_time(lambda: _torch_packed(x, weight, bias, init, bounds)), nbytes), "timing": "eager"}
        out["prefill_packed_4x2048"] = _judge(res, nbytes, sib_bytes)
        del x, init, like
        torch.cuda.empty_cache()
    for layout in ("time", "channel"):
        update_leg(f"prefill_1x12291_{layout}", 1, 12291, layout, _time, "eager")
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "short_conv_bench.json"))
    ns = ap.parse_args()
    line = json.dumps({"short_conv": bench(torch.device("cuda", 0))})
    with open(ns.out, "w") as f:
        f.write(line + "\n")
    print(line)
