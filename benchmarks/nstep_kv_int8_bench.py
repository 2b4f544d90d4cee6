"""N-step paged decode over the int8 KV cache (standalone; not part of bench.py): python benchmarks/nstep_kv_int8_bench.py

`MojoPagedDecodeNstepSWAWithKVDequant` scoring S new tokens per sequence (B 64, head_dim 128, pages of 16, bf16 queries,
graph replay, sustained):

  llama8b_S2 / llama8b_S4   ctx 4096, 32 query / 8 kv heads, no window
  llama70b_S2               ctx 4096, 64 query / 8 kv heads, no window
  swa_local4095_S4          ctx 32768, 32 / 8 heads, local window 4095
  tp8_8q1kv_S3              ctx 4096, 8 / 1 heads: two blocks of steps, each streaming K/V

Every case times five things in the same process, alternating, ROUNDS times each (every figure a median of 5 regions):

  op        the n-step int8 kernel (MOJO_HIP_DECODE_MFMA=1 while its launch is planned, so the case measures the kernel
            whatever the default rule says)
  composed  S launches of the single-step int8 op on query[:, j] and the lengths len - (S - 1 - j): what scoring S tokens
            costs without the op
  single    one such launch on the same cache: the byte floor
  bf16      the 16-bit n-step op (`MojoPagedDecodeNstepSWA`) on a 16-bit cache of the same shape
  prefill   `MojoPagedPrefillSWAWithKVDequant` with q_len = S on the same rows (eager launches timed with events: the op
            sizes a scratch per call)

and reports the median over the rounds, the ratios, and `spread`: the largest (max - min) / median of the repeated medians
of op, composed and single, i.e. what the ratio composed / op must exceed 1 by to mean anything.  The cache contents are
random int8 with random scales: no time here depends on a value.  One JSON object."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.extras import _time, _time_graph, _want, hip  # noqa: E402
from benchmarks.nstep_bench import _forced, _median  # noqa: E402

B, D, PAGE, ROUNDS = 64, 128, 16, 3
CASES = (("llama8b_S2", 4096, 32, 8, 2, None), ("llama8b_S4", 4096, 32, 8, 4, None), ("llama70b_S2", 4096, 64, 8, 2, None),
         ("swa_local4095_S4", 32768, 32, 8, 4, 4095), ("tp8_8q1kv_S3", 4096, 8, 1, 3, None))


def pools(device, ctx, hkv):
    """A bf16 and an int8 K/V pool over one shuffled table (+ per-channel scales)."""
    need = (ctx + PAGE - 1) // PAGE
    total = B * need + 4
    k16 = torch.randn(total, hkv, PAGE, D, device=device, dtype=torch.bfloat16)
    v16 = torch.randn(total, hkv, PAGE, D, device=device, dtype=torch.bfloat16)
    k8 = torch.randint(-127, 128, (total, hkv, PAGE, D), device=device, dtype=torch.int8)
    v8 = torch.randint(-127, 128, (total, hkv, PAGE, D), device=device, dtype=torch.int8)
    scales = (torch.rand(2, hkv, D, device=device) * 0.02 + 0.005).to(torch.bfloat16)
    table = torch.randperm(total, dtype=torch.int32)[: B * need].reshape(B, need).to(device)
    return k16, v16, k8, v8, scales[0], scales[1], table


def bench_case(device, ctx, hq, hkv, steps, local):
    k16, v16, k8, v8, ks, vs, table = pools(device, ctx, hkv)
    q = torch.randn(B, steps, hq, D, device=device, dtype=torch.bfloat16)
    lens = torch.full((B,), ctx, dtype=torch.int32, device=device)
    kw = dict(local_window_size=local)
    nstep8, single8 = hip("MojoPagedDecodeNstepSWAWithKVDequant")(**kw), hip("MojoPagedDecodeSWAWithKVDequant")(**kw)
    nstep16, prefill8 = hip("MojoPagedDecodeNstepSWA")(**kw), hip("MojoPagedPrefillSWAWithKVDequant")(**kw)
    q_j = [q[:, j].contiguous() for j in range(steps)]
    lens_j = [lens - (steps - 1 - j) for j in range(steps)]
    q_rows = q.reshape(B * steps, hq, D)
    cu_q = torch.arange(B + 1, dtype=torch.int32, device=device) * steps
    cu_kv = torch.arange(B + 1, dtype=torch.int32, device=device) * ctx

    def run_op():
        return nstep8(q, None, k8, ks, v8, vs, lens, table, max_total_seq_len=ctx)

    def run_composed():
        return [single8(q_j[j], None, k8, ks, v8, vs, lens_j[j], table, max_total_seq_len=ctx) for j in range(steps)]

    def run_single():
        return single8(q_j[-1], None, k8, ks, v8, vs, lens, table, max_total_seq_len=ctx)

    def run_bf16():
        return nstep16(q, k16, v16, lens, table, max_total_seq_len=ctx)

    def run_prefill():
        return prefill8(q_rows, None, k8, ks, v8, vs, cu_q, table, cu_total_seq_lens=cu_kv, max_q_len=steps,
                        max_total_seq_len=ctx)

    with _forced("1"):
        run_op()
        from mojo_opset_amd.backends.hip import lib
        form = lib.last_launch()
    times = {"op": [], "composed": [], "single": [], "bf16": [], "prefill": []}
    for _ in range(ROUNDS):
        with _forced("1"):
            times["op"].append(_time_graph(run_op))
            times["bf16"].append(_time_graph(run_bf16))
        times["composed"].append(_time_graph(run_composed))
        times["single"].append(_time_graph(run_single))
        times["prefill"].append(_time(run_prefill))
    us = {name: _median(ts) * 1e6 for name, ts in times.items()}
    spread = max((max(times[n]) - min(times[n])) / _median(times[n]) for n in ("op", "composed", "single"))
    keys = ctx if local is None else min(ctx, local + steps)
    return {"form": form, **{f"{name}_us": t for name, t in us.items()},
            "composed_vs_op": us["composed"] / us["op"], "op_vs_single": us["op"] / us["single"],
            "bf16_vs_op": us["bf16"] / us["op"], "prefill_vs_op": us["prefill"] / us["op"], "spread": spread,
            "rounds_us": {name: [t * 1e6 for t in ts] for name, ts in times.items()},
            "op_GB/s": (B * keys * hkv * D * 2 + 2 * B * steps * hq * D * 2) / (us["op"] * 1e-6) / 1e9}


if __name__ == "__main__":
    dev = torch.device("cuda", 0)
    out = {}
    for name, ctx, hq, hkv, steps, local in CASES:
        if _want(name):
            out[name] = bench_case(dev, ctx, hq, hkv, steps, local)
            torch.cuda.empty_cache()
    print(json.dumps({"paged_decode_nstep_kv_int8": out}))
