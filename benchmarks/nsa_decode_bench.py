"""Native-sparse-attention decode benchmark (standalone; not part of bench.py):
python -m benchmarks.nsa_decode_bench [--out profiles/nsa_decode_bench.json]

`MojoPagedDecodeNSA` next to this project's `MojoPagedDecodeGQA` with ``Hq = Hkv = H`` on the same caches, lengths and pages: the
dense step reads the same K / V bytes.  Two cases, head_dim 128, 16 heads, pages of 64, ``cr 4, bs 64, nsel 16, ws 512``:
B 64 at ctx 4096 (planned: the fused form) and B 2 at ctx 32768 (planned: the split form).  HIP events; the two legs
alternated in one process, five medians per leg, the median of the five reported with their spread.  ``kv_GB/s`` is K + V of
the walked keys over the step time.  One JSON object."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.extras import _paged, _time, hip  # noqa: E402
from mojo_opset_amd.backends.hip import lib as L  # noqa: E402

H, D, PAGE, LEGS = 16, 128, 64, 5
CFG = dict(compress_ratio=4, block_size=64, num_selected_blocks=16, window_size=512)
CASES = (("B64_ctx4096", 64, 4096), ("B2_ctx32768", 2, 32768))


def bench(device):
    out = {}
    for name, batch, ctx in CASES:
        k, v, table = _paged(device, [ctx] * batch, H, D, PAGE)
        q = torch.randn(batch, H, D, device=device, dtype=torch.bfloat16)
        lens = torch.full((batch,), ctx, dtype=torch.int32, device=device)
        nsa = hip("MojoPagedDecodeNSA")(H, D, **CFG).to(device)
        with torch.no_grad():
            nsa.gate_proj.data = (torch.randn(H, D, 3, device=device) * D ** -0.5).bfloat16()
        dense = hip("MojoPagedDecodeGQA")()
        legs = {"nsa": lambda: nsa(q, k, v, lens, table), "dense_gqa": lambda: dense(q, k, v, lens, table, max_total_seq_len=ctx)}
        forms, times = {}, {leg: [] for leg in legs}
        for leg, fn in legs.items():
            fn()
            forms[leg] = L.last_launch()
        for _ in range(LEGS):                                  # alternated legs
            for leg, fn in legs.items():
                times[leg].append(_time(fn))
        kv_bytes = 2 * batch * H * ctx * D * 2
        res = {"kv_bytes": kv_bytes}
        for leg in legs:
            m = statistics.median(times[leg])
            res[leg] = {"us": m * 1e6, "us_legs": [t * 1e6 for t in times[leg]],
                        "spread_us": (max(times[leg]) - min(times[leg])) * 1e6, "kv_GB/s": kv_bytes / m / 1e9, "form": forms[leg]}
        res["nsa_over_dense_time"] = res["nsa"]["us"] / res["dense_gqa"]["us"]
        out[name] = res
        del k, v
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ns = ap.parse_args()
    line = json.dumps({"nsa_decode": bench(torch.device("cuda", 0))})
    if ns.out:
        os.makedirs(os.path.dirname(os.path.abspath(ns.out)), exist_ok=True)
        with open(ns.out, "w") as f:
            f.write(line + "\n")
    print(line)
