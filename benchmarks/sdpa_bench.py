"""Bidirectional attention with an optional mask (`MojoSdpa`) benchmark (standalone; not part of bench.py):
python benchmarks/sdpa_bench.py

bf16, HIP events.  Legs:

  dit_self_8192 / dit_self_32760   DiT self-attention: 1 x 40 heads x head_dim 128, token-major views ([B,S,H,D] memory seen
                                   as [B,H,S,D]), no mask
  dit_cross_32760x512              the same rows against 512 text keys
  t5_512                           a T5-like encoder step: 64 heads, head_dim 64, S 512, bf16 bias [1,64,512,512], scale 1
  gqa_32_8_16384                   32 query / 8 kv heads, head_dim 128, S 16384, no mask

Yardsticks, in the same process:

  causal   the causal `MojoSWA` on the same tokens (self-attention legs): its kernel code is the parent commit's.  Compared on
           EXECUTED FLOPs — the key tiles a block walks times its rows — because the causal walk stops at the diagonal.
  torch    `torch.nn.functional.scaled_dot_product_attention` on the device with the same arguments: what the reference's own
           class runs.

Every figure is the median of 5 timed regions after warm-up (min and max beside it).  ``sdpa_rate_floor`` is the causal rate
less that yardstick's own min-to-max spread; ``sdpa_at_least_causal_rate`` says whether `MojoSdpa` reaches it.  One JSON object."""
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.extras import _mfma, _time, _want, hip  # noqa: E402

KEYS = 64                                                  # keys per tile of the prefill kernel


def executed_flops(hq, hkv, d, sq, sk, causal):
    """4 * Hq * D * (rows x keys of the tiles walked): a block of 128 / G positions walks every tile up to its last row's
    diagonal (causal) or all of them."""
    qpb = 128 // (hq // hkv)
    cells = 0
    for lo in range(0, sq, qpb):
        rows = min(qpb, sq - lo)
        keys = min(sk, sk - sq + lo + rows) if causal else sk
        cells += rows * (-(-keys // KEYS) * KEYS)
    return 4.0 * hq * d * cells


def token_major(b, s, h, d, device):
    return torch.randn(b, s, h, d, device=device, dtype=torch.bfloat16).transpose(1, 2)


def leg(name, hq, hkv, d, sq, sk, device, bias=False, scale=None, causal_yardstick=False, iters=10):
    q, k, v = token_major(1, sq, hq, d, device), token_major(1, sk, hkv, d, device), token_major(1, sk, hkv, d, device)
    mask = torch.randn(1, hq, sq, sk, device=device, dtype=torch.bfloat16) if bias else None
    gqa = hq != hkv
    op = hip("MojoSdpa")(scale=scale, enable_gqa=gqa)
    flops = executed_flops(hq, hkv, d, sq, sk, causal=False)
    res = {"shape": dict(hq=hq, hkv=hkv, d=d, sq=sq, sk=sk, mask="bf16 bias" if bias else None, scale=scale),
           "sdpa": _mfma(_time(lambda: op(q, k, v, mask), iters=iters), flops)}
    try:
        fn = lambda: F.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=scale, enable_gqa=gqa)   # noqa: E731
        got, want = op(q, k, v, mask), fn()
        res["max_abs_diff_vs_torch"] = float((got.float() - want.float()).abs().max())
        res["torch"] = _mfma(_time(fn, iters=iters), flops)
        res["sdpa_over_torch_time"] = res["sdpa"]["us"] / res["torch"]["us"]
    except Exception as exc:                               # (recorded, not hidden: a leg the library cannot run)
        res["torch"] = {"error": f"{type(exc).__name__}: {exc}"[:300]}
    if causal_yardstick:
        swa = hip("MojoSWA")()
        qp, kp, vp = (t.transpose(1, 2)[0] for t in (q, k, v))          # the same memory as packed [T,H,D]
        cu = torch.tensor([0, sq], dtype=torch.int32, device=device)
        c_flops = executed_flops(hq, hkv, d, sq, sk, causal=True)
        res["causal"] = _mfma(_time(lambda: swa(qp, kp, vp, cu, cu, max_q_len=sq, max_total_seq_len=sk), iters=iters), c_flops)
        spread = (res["causal"]["us_max"] - res["causal"]["us_min"]) / res["causal"]["us"]
        res["sdpa_rate_floor"] = res["causal"]["tflops"] * (1.0 - spread)
        res["sdpa_at_least_causal_rate"] = res["sdpa"]["tflops"] >= res["sdpa_rate_floor"]
    return res


def bench(device):
    legs = {
        "dit_self_8192": dict(hq=40, hkv=40, d=128, sq=8192, sk=8192, causal_yardstick=True),
        "dit_self_32760": dict(hq=40, hkv=40, d=128, sq=32760, sk=32760, causal_yardstick=True, iters=3),
        "dit_cross_32760x512": dict(hq=40, hkv=40, d=128, sq=32760, sk=512),
        "t5_512": dict(hq=64, hkv=64, d=64, sq=512, sk=512, bias=True, scale=1.0),
        "gqa_32_8_16384": dict(hq=32, hkv=8, d=128, sq=16384, sk=16384, causal_yardstick=True, iters=5),
    }
    out = {}
    for name, kw in legs.items():
        if _want(name):
            out[name] = leg(name, device=device, **kw)
            torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    print(json.dumps({"sdpa": bench(torch.device("cuda", 0))}))
