"""Packed var-len attention over contiguous K/V (`MojoSWA`) benchmark (standalone; not part of bench.py):
python benchmarks/swa_packed_bench.py

A first prefill (no cached prefix), 32 query / 8 kv heads, head_dim 128, bf16, HIP events: 1 x 16384, 4 x 2048 and the 16
ragged sequences of benchmarks/extras.py (512 .. 1024 tokens), each without a window and with one (local 4095 for the long
sequence, global 4 / local 1023 for the short ones).  Per shape, in one process:

  linear          `MojoSWA` on contiguous K/V
  linear_fused    `MojoSWA` on K/V views of a fused [T, (Hq + 2 Hkv) * D] QKV buffer (read in place)
  paged           `MojoPagedPrefillGQA` / `MojoPagedPrefillSWA` on the same tokens in pages of 16 — the yardstick: its code is
                  the parent commit's
  store+paged     `MojoStorePagedKVCache` and then that paged op: the path `MojoSWA` replaces

Every figure is the median of 5 timed regions after warm-up (min and max beside it); FLOPs are ALGORITHMIC and count only the
keys a row can see.  ``linear_minus_paged_us`` against ``paged_spread_us`` (the paged op's own min-to-max in this run) says
whether a difference is inside the yardstick's noise.  One JSON object."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.extras import _mfma, _time, _want, hip  # noqa: E402
from benchmarks.swa_bench import visible  # noqa: E402

HQ, HKV, D, PAGE = 32, 8, 128, 16


def shapes():
    g = torch.Generator().manual_seed(20260716)
    ragged = torch.randint(512, 1025, (16,), generator=g).tolist()
    return {"1x16384": ([16384], (None, 4095)), "4x2048": ([2048] * 4, (4, 1023)), "16_ragged_512_1024": (ragged, (4, 1023))}


def bench(device):
    out = {}
    store = hip("MojoStorePagedKVCache")()
    for shape, (lens, window) in shapes().items():
        tokens = sum(lens)
        fused = torch.randn(tokens, (HQ + 2 * HKV) * D, device=device, dtype=torch.bfloat16)
        q = fused[:, : HQ * D].reshape(tokens, HQ, D).contiguous()
        k_view = fused[:, HQ * D: (HQ + HKV) * D].view(tokens, HKV, D)
        v_view = fused[:, (HQ + HKV) * D:].view(tokens, HKV, D)
        k, v = k_view.contiguous(), v_view.contiguous()
        cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device=device)
        ctx0 = torch.zeros(len(lens), dtype=torch.int32, device=device)
        need = [(n + PAGE - 1) // PAGE for n in lens]
        total = sum(need) + 4
        kc = torch.zeros(total, HKV, PAGE, D, device=device, dtype=torch.bfloat16)
        vc = torch.zeros_like(kc)
        perm = torch.randperm(total, dtype=torch.int32)
        table = torch.full((len(lens), max(need)), -1, dtype=torch.int32)
        at = 0
        for b, n in enumerate(need):
            table[b, :n] = perm[at: at + n]
            at += n
        table = table.to(device)
        store(k, v, kc, vc, table, cu, ctx0)                       # the same tokens, paged
        hints = dict(max_q_len=max(lens), max_total_seq_len=max(lens))
        for glob, local in ((None, None), window):
            name = shape + ("" if local is None else f"_g{glob or 0}_l{local}")
            if not _want(name):
                continue
            kw = dict(global_window_size=glob, local_window_size=local)
            linear = hip("MojoSWA")(**kw)
            paged = hip("MojoPagedPrefillGQA")() if local is None else hip("MojoPagedPrefillSWA")(**kw)
            flops = 4.0 * HQ * D * sum(visible(i, glob, local) for n in lens for i in range(n))
            legs = {
                "linear": lambda: linear(q, k, v, cu, cu, **hints),
                "linear_fused": lambda: linear(q, k_view, v_view, cu, cu, **hints),
                "paged": lambda: paged(q, kc, vc, cu, table, cu_total_seq_lens=cu, **hints),
                "store+paged": lambda: (store(k, v, kc, vc, table, cu, ctx0),
                                        paged(q, kc, vc, cu, table, cu_total_seq_lens=cu, **hints)),
            }
            assert torch.equal(legs["linear"](), legs["paged"]()) and torch.equal(legs["linear_fused"](), legs["paged"]())
            res = {leg: _mfma(_time(fn), flops) for leg, fn in legs.items()}
            res["linear_minus_paged_us"] = res["linear"]["us"] - res["paged"]["us"]
            res["paged_spread_us"] = res["paged"]["us_max"] - res["paged"]["us_min"]
            res["linear_within_paged_spread"] = res["linear_minus_paged_us"] <= res["paged_spread_us"]
            res["store+paged_over_linear"] = res["store+paged"]["us"] / res["linear"]["us"]
            out[name] = res
        del fused, q, k, v, kc, vc
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    print(json.dumps({"swa_packed": bench(torch.device("cuda", 0))}))
