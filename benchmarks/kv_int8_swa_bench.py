"""Sliding-window attention over the int8 paged KV cache (standalone; not part of bench.py):
python benchmarks/kv_int8_swa_bench.py

Decode (graph replay, sustained): B 64, 32 query / 8 kv heads, head_dim 128, pages of 16, bf16 queries, ctx 32768 with a
local window of 4095 and with the windows (4, 1023) — `MojoPagedDecodeSWAWithKVDequant` next to `MojoPagedDecodeSWA` (the
16-bit cache, same shape) and next to `MojoPagedDecodeGQAWithKVDequant` at a context of the visible keys (4096 / 1024:
the same visible bytes).  Prefill (HIP events): a 512-token chunk on 32768 cached tokens and 1 x 16384, local window 4095 —
`MojoPagedPrefillSWAWithKVDequant` minus `MojoPagedPrefillSWA` on the same shape (what the int8 cache costs with a
window) next to `MojoPagedPrefillGQAWithKVDequant` minus `MojoPagedPrefillGQA` at a context of the visible keys (what it
costs without).  The legs of a case alternate in one process, five medians per leg (their spread is reported).  The cache
contents are random int8 with random scales: no time here depends on a value.  One JSON object."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.extras import _time, _time_graph, _want, hip  # noqa: E402

HQ, HKV, D, PAGE = 32, 8, 128, 16
LEGS = 5


def pools(device, lens):
    """A bf16 and an int8 K/V pool over one shuffled table (+ per-channel scales)."""
    need = [(n + PAGE - 1) // PAGE for n in lens]
    total = sum(need) + 4
    k16 = torch.randn(total, HKV, PAGE, D, device=device, dtype=torch.bfloat16)
    v16 = torch.randn(total, HKV, PAGE, D, device=device, dtype=torch.bfloat16)
    k8 = torch.randint(-127, 128, (total, HKV, PAGE, D), device=device, dtype=torch.int8)
    v8 = torch.randint(-127, 128, (total, HKV, PAGE, D), device=device, dtype=torch.int8)
    scales = (torch.rand(2, HKV, D, device=device) * 0.02 + 0.005).to(torch.bfloat16)
    perm = torch.randperm(total, dtype=torch.int32)
    table = torch.full((len(lens), max(need)), -1, dtype=torch.int32)
    at = 0
    for b, n in enumerate(need):
        table[b, :n] = perm[at: at + n]
        at += n
    return k16, v16, k8, v8, scales[0], scales[1], table.to(device)


def legs(fns, timer):
    """{name: [seconds per leg]} with the legs alternated."""
    times = {name: [] for name in fns}
    for _ in range(LEGS):
        for name, fn in fns.items():
            times[name].append(timer(fn))
    return times


def summary(ts):
    return {"us": statistics.median(ts) * 1e6, "us_legs": [t * 1e6 for t in ts], "spread_us": (max(ts) - min(ts)) * 1e6}


def bench_decode(device):
    out = {}
    b, ctx = 64, 32768
    cases = (("ctx32768_local4095", None, 4095), ("ctx32768_global4_local1023", 4, 1023))
    if not any(_want(name) for name, _, _ in cases):
        return out
    k16, v16, k8, v8, ks, vs, table = pools(device, [ctx] * b)
    q = torch.randn(b, HQ, D, device=device, dtype=torch.bfloat16)
    lens = torch.full((b,), ctx, dtype=torch.int32, device=device)
    for name, glob, local in cases:
        if not _want(name):
            continue
        visible = local + 1                                     # the unwindowed context with the same visible bytes
        short_lens = torch.full((b,), visible, dtype=torch.int32, device=device)
        short_table = table[:, : visible // PAGE].contiguous()
        kw = dict(global_window_size=glob, local_window_size=local)
        swa8, swa16 = hip("MojoPagedDecodeSWAWithKVDequant")(**kw), hip("MojoPagedDecodeSWA")(**kw)
        gqa8 = hip("MojoPagedDecodeGQAWithKVDequant")()
        t = legs({
            "swa_int8": lambda: swa8(q, None, k8, ks, v8, vs, lens, table, max_total_seq_len=ctx),
            "swa_bf16": lambda: swa16(q, k16, v16, lens, table, max_total_seq_len=ctx),
            "gqa_int8_visible_ctx": lambda: gqa8(q, None, k8, ks, v8, vs, short_lens, short_table, max_total_seq_len=visible),
        }, _time_graph)
        res = {leg: summary(ts) for leg, ts in t.items()}
        res["visible_ctx"] = visible
        res["swa_int8_over_gqa_int8_visible_ctx"] = res["swa_int8"]["us"] / res["gqa_int8_visible_ctx"]["us"]
        res["swa_int8_over_swa_bf16"] = res["swa_int8"]["us"] / res["swa_bf16"]["us"]
        res["target_1.15x_met"] = res["swa_int8_over_gqa_int8_visible_ctx"] <= 1.15
        out[name] = res
    return out


def bench_prefill(device):
    out = {}
    cu = lambda l: torch.tensor([0] + list(torch.tensor(l).cumsum(0).tolist()), dtype=torch.int32, device=device)  # noqa: E731
    local = 4095
    for name, q_len, cached in (("chunk512_on_32768_local4095", 512, 32768), ("1x16384_local4095", 16384, 0)):
        if not _want(name):
            continue
        kv = q_len + cached
        k16, v16, k8, v8, ks, vs, table = pools(device, [kv])
        q = torch.randn(q_len, HQ, D, device=device, dtype=torch.bfloat16)
        cu_q, cu_kv = cu([q_len]), cu([kv])
        kw = dict(cu_total_seq_lens=cu_kv, max_q_len=q_len, max_total_seq_len=kv)
        swa8 = hip("MojoPagedPrefillSWAWithKVDequant")(local_window_size=local)
        swa16 = hip("MojoPagedPrefillSWA")(local_window_size=local)
        fns = {"swa_int8": lambda: swa8(q, None, k8, ks, v8, vs, cu_q, table, **kw),
               "swa_bf16": lambda: swa16(q, k16, v16, cu_q, table, **kw)}
        # the unwindowed pair at a context of the keys the chunk can see (the whole sequence when that is shorter)
        vis = min(kv, q_len + local)
        vis_table = table[:, : (vis + PAGE - 1) // PAGE].contiguous()
        cu_vis = cu([vis])
        kw_vis = dict(cu_total_seq_lens=cu_vis, max_q_len=q_len, max_total_seq_len=vis)
        gqa8, gqa16 = hip("MojoPagedPrefillGQAWithKVDequant")(), hip("MojoPagedPrefillGQA")()
        fns["gqa_int8_visible_ctx"] = lambda: gqa8(q, None, k8, ks, v8, vs, cu_q, vis_table, **kw_vis)
        fns["gqa_bf16_visible_ctx"] = lambda: gqa16(q, k16, v16, cu_q, vis_table, **kw_vis)
        t = legs(fns, _time)
        res = {leg: summary(ts) for leg, ts in t.items()}
        res["visible_ctx"] = vis
        res["swa_int8_minus_swa_bf16_us"] = res["swa_int8"]["us"] - res["swa_bf16"]["us"]
        res["gqa_int8_minus_gqa_bf16_us"] = res["gqa_int8_visible_ctx"]["us"] - res["gqa_bf16_visible_ctx"]["us"]
        res["difference_ratio"] = res["swa_int8_minus_swa_bf16_us"] / res["gqa_int8_minus_gqa_bf16_us"]
        res["target_1.15x_met"] = res["difference_ratio"] <= 1.15
        out[name] = res
        del k16, v16, k8, v8
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    dev = torch.device("cuda", 0)
    print(json.dumps({"paged_prefill_swa_kv_int8": bench_prefill(dev), "paged_decode_swa_kv_int8": bench_decode(dev)}))
