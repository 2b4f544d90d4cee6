"""N-step paged decode benchmark (standalone; not part of bench.py): python benchmarks/nstep_bench.py

`MojoPagedDecodeNstepSWA` scoring S new tokens per sequence (B 64, head_dim 128, pages of 16, bf16, graph replay, sustained):

  llama8b_S2 / llama8b_S4   ctx 4096, 32 query / 8 kv heads, no window
  llama70b_S2               ctx 4096, 64 query / 8 kv heads, no window
  swa_local4095_S4          ctx 32768, 32 / 8 heads, local window 4095

and, for the default rule, the corners of the kernel's envelope at ctx 4096: tp8_8q1kv_S3 (8 / 1 heads: two blocks of steps,
each streaming K/V), d64_S4 (head_dim 64), mha_S4 (8 / 8 heads: one head per kv head) and g16_S2 (16 / 1 heads: one step per
block, so the bytes of the composed route in one launch).

Every case times three things in the same process, alternating, ROUNDS times each (every figure a median of 5 regions):

  op        the n-step kernel (MOJO_HIP_DECODE_MFMA=1 while its launch is planned, so the case measures the kernel whatever
            the default rule says)
  composed  S launches of the single-step op on query[:, j] and the lengths len - (S - 1 - j): what scoring S tokens costs
            without the op
  single    one single-step launch on the same cache: the byte floor

and reports the median over the rounds, the ratios, and `spread`: the largest (max - min) / median of a figure's repeated
medians, i.e. what a ratio must exceed 1 by to mean anything.  One JSON object."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.extras import _paged, _time_graph, _want, hip  # noqa: E402
from mojo_opset_amd import switches  # noqa: E402

B, D, PAGE, ROUNDS = 64, 128, 16, 3
CASES = (("llama8b_S2", 4096, 32, 8, 2, None, D), ("llama8b_S4", 4096, 32, 8, 4, None, D), ("llama70b_S2", 4096, 64, 8, 2, None, D),
         ("swa_local4095_S4", 32768, 32, 8, 4, 4095, D), ("tp8_8q1kv_S3", 4096, 8, 1, 3, None, D), ("d64_S4", 4096, 32, 8, 4, None, 64),
         ("mha_S4", 4096, 8, 8, 4, None, D), ("g16_S2", 4096, 16, 1, 2, None, D))


class _forced:
    """MOJO_HIP_DECODE_MFMA=<value> while a launch is planned (the switches are latched: reload on both edges)."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("MOJO_HIP_DECODE_MFMA")
        os.environ["MOJO_HIP_DECODE_MFMA"] = self.value
        switches.reload()

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("MOJO_HIP_DECODE_MFMA", None)
        else:
            os.environ["MOJO_HIP_DECODE_MFMA"] = self.old
        switches.reload()
        return False


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def bench_case(device, ctx, hq, hkv, steps, local, d):
    k, v, table = _paged(device, [ctx] * B, hkv, d, PAGE)
    q = torch.randn(B, steps, hq, d, device=device, dtype=torch.bfloat16)
    lens = torch.full((B,), ctx, dtype=torch.int32, device=device)
    nstep = hip("MojoPagedDecodeNstepSWA")(local_window_size=local)
    single = hip("MojoPagedDecodeSWA")(local_window_size=local)
    q_j = [q[:, j].contiguous() for j in range(steps)]
    lens_j = [lens - (steps - 1 - j) for j in range(steps)]

    def run_op():
        return nstep(q, k, v, lens, table, max_total_seq_len=ctx)

    def run_composed():
        return [single(q_j[j], k, v, lens_j[j], table, max_total_seq_len=ctx) for j in range(steps)]

    def run_single():
        return single(q_j[-1], k, v, lens, table, max_total_seq_len=ctx)

    with _forced("1"):
        run_op()
        from mojo_opset_amd.backends.hip import lib
        form = lib.last_launch()
    times = {"op": [], "composed": [], "single": []}
    for _ in range(ROUNDS):
        with _forced("1"):
            times["op"].append(_time_graph(run_op))
        times["composed"].append(_time_graph(run_composed))
        times["single"].append(_time_graph(run_single))
    us = {name: _median(ts) * 1e6 for name, ts in times.items()}
    spread = max((max(ts) - min(ts)) / _median(ts) for ts in times.values())
    keys = ctx if local is None else min(ctx, local + steps)
    return {"form": form, "op_us": us["op"], "composed_us": us["composed"], "single_us": us["single"],
            "composed_vs_op": us["composed"] / us["op"], "op_vs_single": us["op"] / us["single"], "spread": spread,
            "rounds_us": {name: [t * 1e6 for t in ts] for name, ts in times.items()},
            "op_GB/s": (B * keys * hkv * d * 2 * 2 + 2 * B * steps * hq * d * 2) / (us["op"] * 1e-6) / 1e9}


if __name__ == "__main__":
    dev = torch.device("cuda", 0)
    out = {}
    for name, ctx, hq, hkv, steps, local, d in CASES:
        if _want(name):
            out[name] = bench_case(dev, ctx, hq, hkv, steps, local, d)
            torch.cuda.empty_cache()
    print(json.dumps({"paged_decode_nstep": out}))
