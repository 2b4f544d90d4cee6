"""int8-compute paged prefill benchmark (standalone; not part of bench.py):
python -m benchmarks.sage_prefill_bench [--out profiles/sage_prefill_bench.json]

`MojoPagedPrefillSageGQA` next to `MojoPagedPrefillGQAWithKVDequant` (the dequantising gather + the bf16 kernel) and
`MojoPagedPrefillGQA` (bf16 caches) on the same lengths: 2 x 1024 (16 / 4 heads, pages of 32), 2 x 512 on 1024 cached keys (8 / 1
heads, pages of 128) and one prompt of 8192 (32 / 8 heads, pages of 16), head_dim 128.  HIP events; the three legs alternated in
one process, five medians per leg (WARM: back-to-back calls, the caches hold what the previous call left) and the median of five
single calls that each follow a 1 GiB fill (COLD: nothing of the operands in the caches).  MFMA work is ALGORITHMIC: causal
multiply-adds of Q.K^T and P.V; the int8 op computes Q.K^T twice.  One JSON object."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.extras import _paged, _time, hip  # noqa: E402

D, LEGS = 128, 5
CASES = (("2x1024", [1024, 1024], [0, 0], 16, 4, 32), ("2x512_cached1024", [512, 512], [1024, 1024], 8, 1, 128),
         ("1x8192", [8192], [0], 32, 8, 16))


def _cold(fn, spoil):
    times = []
    for _ in range(LEGS):
        spoil.fill_(1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    return statistics.median(times)


def bench(device):
    out = {}
    spoil = torch.empty(1 << 30, dtype=torch.uint8, device=device)
    cu = lambda l: torch.tensor([0] + torch.tensor(l).cumsum(0).tolist(), dtype=torch.int32, device=device)  # noqa: E731
    for name, q_lens, cached, hq, hkv, page in CASES:
        kv = [a + c for a, c in zip(q_lens, cached)]
        k, v, table = _paged(device, kv, hkv, D, page)
        q = torch.randn(sum(q_lens), hq, D, device=device, dtype=torch.bfloat16)
        # per-channel int8 cache of the kv8 route (bf16 scales), per-token K / per-channel V / per-token Q of the int8-compute op
        kc_scale = (k.float().abs().amax(dim=(0, 2)) / 127).clamp(min=1e-5)
        vc_scale = (v.float().abs().amax(dim=(0, 2)) / 127).clamp(min=1e-5)
        k8c = torch.round(k.float() / kc_scale[None, :, None, :]).clamp(-127, 127).to(torch.int8)
        v8 = torch.round(v.float() / vc_scale[None, :, None, :]).clamp(-127, 127).to(torch.int8)
        kt_scale = (k.float().abs().amax(dim=-1) / 127).clamp(min=1e-5)
        k8t = torch.round(k.float() / kt_scale[..., None]).clamp(-127, 127).to(torch.int8)
        q_scale = (q.float().abs().amax(dim=-1) / 127).clamp(min=1e-5)
        q8 = torch.round(q.float() / q_scale[..., None]).clamp(-127, 127).to(torch.int8)
        q_scale_t = q_scale.T.contiguous()
        kc_scale16, vc_scale16 = kc_scale.bfloat16(), vc_scale.bfloat16()
        cu_q, cu_kv = cu(q_lens), cu(kv)
        kw = dict(cu_total_seq_lens=cu_kv, max_q_len=max(q_lens), max_total_seq_len=max(kv))
        sage, kv8, bf16 = hip("MojoPagedPrefillSageGQA")(), hip("MojoPagedPrefillGQAWithKVDequant")(), hip("MojoPagedPrefillGQA")()
        legs = {"sage_int8": lambda: sage(q8, q_scale_t, k8t, kt_scale, v8, vc_scale, cu_q, table, **kw),
                "kv8_dequant": lambda: kv8(q, None, k8c, kc_scale16, v8, vc_scale16, cu_q, table, **kw),
                "bf16": lambda: bf16(q, k, v, cu_q, table, **kw)}
        warm = {leg: [] for leg in legs}
        for _ in range(LEGS):                                  # alternated legs
            for leg, fn in legs.items():
                warm[leg].append(_time(fn))
        macs = sum(2 * hq * D * (a * c + a * (a + 1) // 2) for a, c in zip(q_lens, cached))       # Q.K^T + P.V, causal
        res = {"causal_macs": macs}
        for leg, fn in legs.items():
            m = statistics.median(warm[leg])
            res[leg] = {"warm_us": m * 1e6, "warm_us_legs": [t * 1e6 for t in warm[leg]],
                        "warm_spread_us": (max(warm[leg]) - min(warm[leg])) * 1e6, "cold_us": _cold(fn, spoil) * 1e6,
                        "algorithmic_tmacs_per_s": macs * (1.5 if leg == "sage_int8" else 1.0) / m / 1e12}
        res["sage_over_bf16_time"] = res["sage_int8"]["warm_us"] / res["bf16"]["warm_us"]
        res["sage_over_kv8_time"] = res["sage_int8"]["warm_us"] / res["kv8_dequant"]["warm_us"]
        out[name] = res
        del k, v, k8c, k8t, v8
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ns = ap.parse_args()
    line = json.dumps({"sage_prefill": bench(torch.device("cuda", 0))})
    if ns.out:
        os.makedirs(os.path.dirname(os.path.abspath(ns.out)), exist_ok=True)
        with open(ns.out, "w") as f:
            f.write(line + "\n")
    print(line)
