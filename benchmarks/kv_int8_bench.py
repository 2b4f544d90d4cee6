"""int8 paged KV cache benchmark (standalone; not part of bench.py): python benchmarks/kv_int8_bench.py

Decode (graph replay, sustained): B 64, 32 query / 8 kv heads, head_dim 128, pages of 16, bf16 queries, at ctx 1024 / 4096 /
16384 and ragged 2048-4096, plus 64 / 8 heads at ctx 4096 — `MojoPagedDecodeGQAWithKVDequant` next to `MojoPagedDecodeGQA`
on the same lengths, the two legs alternated in the same process, five medians per leg (their spread is reported).
Store (HIP events): 64 decode tokens and 8192 prefill tokens, next to `MojoStorePagedKVCache`.
Prefill (HIP events): 1 x 16384 and 4 x 2048 on 2048 cached, next to `MojoPagedPrefillGQA`; the gather's byte estimate is
three int8-cache-sizes of the gathered pages at 8 TB/s.  Bytes are ALGORITHMIC.  One JSON object."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.extras import _paged, _time, _time_graph, _want, hip  # noqa: E402

HKV, D, PAGE = 8, 128, 16
HBM_PEAK = 8.0e12
LEGS = 5


def quantize(cache):
    """Per-channel amax / 127 (clamp 1e-5), scales stored as bf16 — the reference tests' recipe, on the device."""
    f = cache.float()
    scale = (f.abs().amax(dim=(0, 2)) / 127).clamp(min=1e-5)
    q = torch.round(f / scale[None, :, None, :]).clamp(-128, 127).to(torch.int8)
    return q, scale.to(torch.bfloat16)


def bench_decode(device):
    out = {}
    b = 64
    g = torch.Generator().manual_seed(20260716)
    cases = (("ctx1024", 32, [1024] * b), ("ctx4096", 32, [4096] * b), ("ctx16384", 32, [16384] * b),
             ("ragged_2048_4096", 32, torch.randint(2048, 4097, (b,), generator=g).tolist()), ("hq64_ctx4096", 64, [4096] * b))
    for name, hq, lens_l in cases:
        if not _want(name):
            continue
        k, v, table = _paged(device, lens_l, HKV, D, PAGE)
        k8, ks = quantize(k)
        v8, vs = quantize(v)
        q = torch.randn(b, hq, D, device=device, dtype=torch.bfloat16)
        lens = torch.tensor(lens_l, dtype=torch.int32, device=device)
        hint = max(lens_l)
        op16, op8 = hip("MojoPagedDecodeGQA")(), hip("MojoPagedDecodeGQAWithKVDequant")()
        f16 = lambda: op16(q, k, v, lens, table, max_total_seq_len=hint)  # noqa: E731
        f8 = lambda: op8(q, None, k8, ks, v8, vs, lens, table, max_total_seq_len=hint)  # noqa: E731
        t16, t8 = [], []
        for _ in range(LEGS):                                  # alternated legs
            t16.append(_time_graph(f16))
            t8.append(_time_graph(f8))
        tokens = sum(lens_l)
        other = 2 * b * hq * D * 2 + 4 * b * (table.shape[1] + 1)
        bytes16 = tokens * HKV * D * 2 * 2 + other
        bytes8 = tokens * HKV * D * 2 * 1 + 2 * HKV * D * 2 + other
        m16, m8 = statistics.median(t16), statistics.median(t8)
        out[name] = {
            "bf16": {"us": m16 * 1e6, "us_legs": [t * 1e6 for t in t16], "spread_us": (max(t16) - min(t16)) * 1e6,
                     "tokens_per_s": b / m16, "bytes": bytes16, "frac_of_hbm_peak": bytes16 / m16 / HBM_PEAK},
            "int8": {"us": m8 * 1e6, "us_legs": [t * 1e6 for t in t8], "spread_us": (max(t8) - min(t8)) * 1e6,
                     "tokens_per_s": b / m8, "bytes": bytes8, "frac_of_hbm_peak": bytes8 / m8 / HBM_PEAK},
            "int8_over_bf16_time": m8 / m16, "bytes_predict": bytes8 / bytes16,
            "faster_by_more_than_the_spread": (m16 - m8) > max(max(t16) - min(t16), max(t8) - min(t8)),
        }
        del k, v, k8, v8
        torch.cuda.empty_cache()
    return out


def bench_store(device):
    out = {}
    cu = lambda l: torch.tensor([0] + list(torch.tensor(l).cumsum(0).tolist()), dtype=torch.int32, device=device)  # noqa: E731
    for name, q_lens, ctx in (("decode_64_tokens", None, [4095] * 64), ("prefill_8192_tokens", [2048] * 4, [0] * 4)):
        if not _want(name):
            continue
        end = [c + (1 if q_lens is None else q_lens[i]) for i, c in enumerate(ctx)]
        k, v, table = _paged(device, end, HKV, D, PAGE)
        k8, v8 = torch.zeros_like(k, dtype=torch.int8), torch.zeros_like(v, dtype=torch.int8)
        tokens = len(ctx) if q_lens is None else sum(q_lens)
        ks = torch.randn(tokens, HKV, D, device=device, dtype=torch.bfloat16)
        vs = torch.randn(tokens, HKV, D, device=device, dtype=torch.bfloat16)
        scale = (torch.rand(HKV, D, device=device) * 0.05 + 0.01).to(torch.bfloat16)
        ctx_t = torch.tensor(ctx, dtype=torch.int32, device=device)
        cu_q = None if q_lens is None else cu(q_lens)
        op16, op8 = hip("MojoStorePagedKVCache")(), hip("MojoStorePagedKVCacheC8")()
        t16 = _time(lambda: op16(ks, vs, k, v, table, cu_q, ctx_t))
        t8 = _time(lambda: op8(ks, vs, k8, v8, scale, scale, table, cu_q, ctx_t))
        n = tokens * HKV * D * 2
        out[name] = {"bf16": {"us": t16 * 1e6, "bytes": n * 4, "GB/s": n * 4 / t16 / 1e9},
                     "int8": {"us": t8 * 1e6, "bytes": n * 3, "GB/s": n * 3 / t8 / 1e9}}
    return out


def bench_prefill(device):
    out = {}
    hq = 32
    cu = lambda l: torch.tensor([0] + list(torch.tensor(l).cumsum(0).tolist()), dtype=torch.int32, device=device)  # noqa: E731
    for name, q_lens, cached in (("1x16384", [16384], [0]), ("4x2048_cached2048", [2048] * 4, [2048] * 4)):
        if not _want(name):
            continue
        kv = [a + c for a, c in zip(q_lens, cached)]
        k, v, table = _paged(device, kv, HKV, D, PAGE)
        k8, ks = quantize(k)
        v8, vs = quantize(v)
        q = torch.randn(sum(q_lens), hq, D, device=device, dtype=torch.bfloat16)
        cu_q, cu_kv = cu(q_lens), cu(kv)
        op16, op8 = hip("MojoPagedPrefillGQA")(), hip("MojoPagedPrefillGQAWithKVDequant")()
        kw = dict(cu_total_seq_lens=cu_kv, max_q_len=max(q_lens), max_total_seq_len=max(kv))
        t16, t8 = [], []
        for _ in range(3):
            t16.append(_time(lambda: op16(q, k, v, cu_q, table, **kw)))
            t8.append(_time(lambda: op8(q, None, k8, ks, v8, vs, cu_q, table, **kw)))
        m16, m8 = statistics.median(t16), statistics.median(t8)
        gather_bytes = 3 * sum(kv) * HKV * D * 2
        out[name] = {"bf16_us": m16 * 1e6, "int8_us": m8 * 1e6, "overhead_us": (m8 - m16) * 1e6,
                     "gather_bytes": gather_bytes, "gather_estimate_us": gather_bytes / HBM_PEAK * 1e6,
                     "overhead_over_estimate": (m8 - m16) / (gather_bytes / HBM_PEAK)}
    return out


if __name__ == "__main__":
    dev = torch.device("cuda", 0)
    print(json.dumps({"paged_decode_kv_int8": bench_decode(dev), "store_paged_kv_c8": bench_store(dev),
                      "paged_prefill_kv_int8": bench_prefill(dev)}))
