"""Native-sparse-attention prefill benchmark (standalone; not part of bench.py):
python -m benchmarks.nsa_prefill_bench [--out profiles/nsa_prefill_bench.json]

`MojoPagedPrefillNSA` next to this project's `MojoPagedPrefillGQA` with ``Hq = Hkv = H`` on the same caches: the dense causal
prefill over the same bytes.  bf16, 16 heads, head_dim 128, pages of 64, ``cr 4, bs 64, nsel 16, ws 512``; one long prompt
(B 1 x 8192) and one batch of chunks (B 8 x q 512 over kv 4096).  HIP events; the two legs alternated in one process, five
medians per leg, the median of the five reported with their spread.  One JSON object."""
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
CASES = (("B1_q8192_kv8192", 1, 8192, 8192), ("B8_q512_kv4096", 8, 512, 4096))


def bench(device):
    out = {}
    for name, batch, q_len, kv_len in CASES:
        k, v, table = _paged(device, [kv_len] * batch, H, D, PAGE)
        q = torch.randn(batch * q_len, H, D, device=device, dtype=torch.bfloat16)
        cu_q = torch.arange(batch + 1, dtype=torch.int32, device=device) * q_len
        cu_kv = torch.arange(batch + 1, dtype=torch.int32, device=device) * kv_len
        nsa = hip("MojoPagedPrefillNSA")(H, D, **CFG).to(device)
        with torch.no_grad():
            nsa.gate_proj.data = (torch.randn(H, D, 3, device=device) * D ** -0.5).bfloat16()
        dense = hip("MojoPagedPrefillGQA")()
        legs = {"nsa": lambda: nsa(q, k, v, cu_q, table, cu_total_seq_lens=cu_kv),
                "dense_gqa": lambda: dense(q, k, v, cu_q, table, cu_total_seq_lens=cu_kv, max_q_len=q_len, max_total_seq_len=kv_len)}
        forms, times = {}, {leg: [] for leg in legs}
        for leg, fn in legs.items():
            fn()
            forms[leg] = L.last_launch()
        for _ in range(LEGS):                                  # alternated legs
            for leg, fn in legs.items():
                times[leg].append(_time(fn))
        res = {"dense_flops": 4 * batch * H * D * (q_len * kv_len - q_len * q_len / 2)}
        for leg in legs:
            m = statistics.median(times[leg])
            res[leg] = {"us": m * 1e6, "us_legs": [t * 1e6 for t in times[leg]],
                        "spread_us": (max(times[leg]) - min(times[leg])) * 1e6, "form": forms[leg]}
        res["nsa_over_dense_time"] = res["nsa"]["us"] / res["dense_gqa"]["us"]
        out[name] = res
        del k, v
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ns = ap.parse_args()
    line = json.dumps({"nsa_prefill": bench(torch.device("cuda", 0))})
    if ns.out:
        os.makedirs(os.path.dirname(os.path.abspath(ns.out)), exist_ok=True)
        with open(ns.out, "w") as f:
            f.write(line + "\n")
    print(line)
