"""Sliding-window paged attention benchmark (standalone; not part of bench.py): python benchmarks/swa_bench.py

Decode (graph replay, sustained): B 64, 32 query / 8 kv heads, head_dim 128, pages of 16, bf16, ctx 32768 with a local
window of 4095 and with (global 4, local 1023), and the GQA op at ctx 4096 and 32768 as calibration in the same process.
Prefill (HIP events): 1 x 16384 with local 4095, 4 x 2048 new tokens on 2048 cached ones with (4, 1023) (the cached-prefix
shape of benchmarks/extras.py's prefill cases), and the GQA prefill on the same shapes.  Bytes and FLOPs are ALGORITHMIC and count only the keys a row can see.  One JSON object."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.extras import _hbm, _mfma, _paged, _time, _time_graph, _want, hip  # noqa: E402

HQ, HKV, D, PAGE = 32, 8, 128, 16


def visible(q_pos, glob, local):
    """Keys a query at position q_pos sees."""
    if glob is None and local is None:
        return q_pos + 1
    n = min(q_pos + 1, local + 1) if local is not None else 0
    lo = q_pos - local if local is not None else q_pos + 1
    return n + max(min(glob or 0, lo, q_pos + 1), 0)


def bench_decode(device):
    out = {}
    b = 64
    for name, ctx, glob, local in (("gqa_ctx4096", 4096, None, None), ("swa_ctx32768_local4095", 32768, None, 4095),
                                   ("swa_ctx32768_g4_l1023", 32768, 4, 1023), ("gqa_ctx32768", 32768, None, None)):
        if not _want(name):
            continue
        k, v, table = _paged(device, [ctx] * b, HKV, D, PAGE)
        q = torch.randn(b, HQ, D, device=device, dtype=torch.bfloat16)
        lens = torch.full((b,), ctx, dtype=torch.int32, device=device)
        if glob is None and local is None:
            op = hip("MojoPagedDecodeGQA")()
        else:
            op = hip("MojoPagedDecodeSWA")(global_window_size=glob, local_window_size=local)
        keys = visible(ctx - 1, glob, local)
        nbytes = b * keys * HKV * D * 2 * 2 + 2 * b * HQ * D * 2 + 4 * b * (table.shape[1] + 1)
        t = _time_graph(lambda: op(q, k, v, lens, table, max_total_seq_len=ctx))
        out[name] = {**_hbm(t, nbytes), "visible_keys": keys}
        del k, v
        torch.cuda.empty_cache()
    if "gqa_ctx4096" in out and "swa_ctx32768_local4095" in out:
        out["swa_local4095_vs_gqa_ctx4096"] = out["swa_ctx32768_local4095"]["us"] / out["gqa_ctx4096"]["us"]
    if "gqa_ctx32768" in out and "swa_ctx32768_local4095" in out:
        out["gqa_ctx32768_vs_swa_local4095"] = out["gqa_ctx32768"]["us"] / out["swa_ctx32768_local4095"]["us"]
    return out


def bench_prefill(device):
    out = {}
    for name, q_lens, cached, glob, local in (("swa_1x16384_local4095", [16384], [0], None, 4095),
                                              ("gqa_1x16384", [16384], [0], None, None),
                                              ("swa_4x2048_cached2048_g4_l1023", [2048] * 4, [2048] * 4, 4, 1023),
                                              ("gqa_4x2048_cached2048", [2048] * 4, [2048] * 4, None, None)):
        if not _want(name):
            continue
        kv = [a + c for a, c in zip(q_lens, cached)]
        k, v, table = _paged(device, kv, HKV, D, PAGE)
        q = torch.randn(sum(q_lens), HQ, D, device=device, dtype=torch.bfloat16)
        cu = lambda l: torch.tensor([0] + list(torch.tensor(l).cumsum(0).tolist()), dtype=torch.int32, device=device)  # noqa: E731
        cu_q, cu_kv = cu(q_lens), cu(kv)
        if glob is None and local is None:
            op = hip("MojoPagedPrefillGQA")()
        else:
            op = hip("MojoPagedPrefillSWA")(global_window_size=glob, local_window_size=local)
        keys = sum(visible(c + i, glob, local) for ql, c in zip(q_lens, cached) for i in range(ql))
        flops = 4.0 * HQ * D * keys
        t = _time(lambda: op(q, k, v, cu_q, table, cu_total_seq_lens=cu_kv, max_q_len=max(q_lens), max_total_seq_len=max(kv)))
        out[name] = _mfma(t, flops)
    if "gqa_1x16384" in out and "swa_1x16384_local4095" in out:
        out["swa_local4095_tflops_vs_gqa"] = out["swa_1x16384_local4095"]["tflops"] / out["gqa_1x16384"]["tflops"]
    return out


if __name__ == "__main__":
    dev = torch.device("cuda", 0)
    print(json.dumps({"paged_decode_swa": bench_decode(dev), "paged_prefill_swa": bench_prefill(dev)}))
