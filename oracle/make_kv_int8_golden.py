"""Write tests/golden/paged_kv_int8_store.pt, _decode.pt and _prefill.pt: reference outputs of the int8 paged KV cache
ops (authoring machine only).

Usage: python oracle/make_kv_int8_golden.py [reference root]   (default: MOJO_REFERENCE_ROOT, else /root/reference; nothing else reads it)

The outputs come from the reference's own `MojoStorePagedKVCacheC8.forward`
(`mojo_opset/experimental/operators/kv_cache.py:109-184`), `MojoPagedDecodeGQAWithKVDequant.forward` and
`MojoPagedPrefillGQAWithKVDequant.forward` (`experimental/operators/attention.py:461-800`), called on CPU.  Each case
records the constructor keywords, the inputs and the output; tests/test_kv_int8_golden.py pins oracle/kv_int8.py
to them bit for bit and tests/test_hip_kv_int8.py runs the hip backend on them.
"""
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.kv_int8 import quantize_kv_cache  # noqa: E402  (the reference tests' recipe, test_attention_quant.py:46-67)
from oracle.paged import cu  # noqa: E402


def paged_inputs(g, batch, hq, hkv, d, kv_lens, page, q_rows):
    need = [max((n + page - 1) // page, 0) for n in kv_lens]
    width = max(max(need), 1)
    total = max(sum(need), 1)
    k8, ks = quantize_kv_cache(torch.randn(total, hkv, page, d, generator=g))
    v8, vs = quantize_kv_cache(torch.randn(total, hkv, page, d, generator=g))
    table = torch.full((batch, width), -1, dtype=torch.int32)
    free = torch.randperm(total, generator=g, dtype=torch.int32)
    at = 0
    for b, n in enumerate(need):
        table[b, :n] = free[at: at + n]
        at += n
    q = torch.randn(q_rows, hq, d, generator=g).to(torch.bfloat16)
    return q, k8, ks, v8, vs, table


# (kind, layout, compute dtype, page, hq, hkv, d, kv_lens, q_lens)
ATTN_CASES = [
    ("decode", "AABB", torch.bfloat16, 16, 4, 4, 64, [100, 0, 33], None),            # group 1, a zero-length row
    ("decode", "ABAB", torch.bfloat16, 32, 4, 2, 96, [70, 1], None),                 # group 2
    ("decode", "AABB", torch.bfloat16, 128, 4, 1, 128, [130, 128], None),            # group 4
    ("decode", "ABAB", torch.bfloat16, 16, 8, 1, 64, [49, 16, 300], None),           # group 8
    ("decode", "ABAB", torch.int8, 16, 4, 2, 64, [40, 17], None),                    # compute_dtype=int8 (golden only)
    ("prefill", "AABB", torch.bfloat16, 16, 2, 2, 64, [50, 0, 20], [50, 0, 20]),     # group 1, an empty sequence
    ("prefill", "ABAB", torch.bfloat16, 32, 4, 2, 96, [70, 30], [70, 30]),
    ("prefill", "AABB", torch.bfloat16, 128, 4, 1, 128, [140], [140]),
    ("prefill", "ABAB", torch.bfloat16, 16, 8, 1, 64, [100, 37], [64, 37]),
    ("prefill", "AABB", torch.bfloat16, 16, 4, 1, 64, [300], [40]),                  # chunked prefill on a cached prefix
    ("prefill", "AABB", torch.int8, 16, 4, 2, 64, [40, 33], [20, 33]),               # compute_dtype=int8 (golden only)
]

# (state dtype, scale dtype, page, heads, d, context_kv_lens, q_lens | None = decode mode, plan form?)
STORE_CASES = [
    (torch.bfloat16, torch.bfloat16, 16, 2, 64, [0, 0], [20, 3], True),
    (torch.bfloat16, torch.float32, 16, 2, 64, [5, -1, 30], [4, 0, 2], False),       # a context_kv_lens = -1 row, a q_len = 0 row
    (torch.bfloat16, torch.float32, 32, 2, 96, [31, -1, 64], None, False),           # decode mode, legacy arguments
    (torch.bfloat16, torch.bfloat16, 128, 1, 128, [127, 3], None, True),             # decode mode, plan
    (torch.float16, torch.float16, 16, 2, 64, [15, 40], [33, 7], False),
    (torch.bfloat16, torch.bfloat16, 16, 2, 64, [5, -1, 30], [4, 0, 2], True),
]


def main(reference_root):
    sys.path.insert(0, reference_root)
    from mojo_opset.core.operators.kv_cache import build_paged_kv_chunk_metadata
    from mojo_opset.experimental.operators import attention as ref_attn
    from mojo_opset.experimental.operators import kv_cache as ref_kv

    g = torch.Generator().manual_seed(2027)
    files = {"store": [], "decode": [], "prefill": []}
    for kind, layout, compute, page, hq, hkv, d, kv_lens, q_lens in ATTN_CASES:
        batch = len(kv_lens)
        rows = batch if kind == "decode" else sum(q_lens)
        q, k8, ks, v8, vs, table = paged_inputs(g, batch, hq, hkv, d, kv_lens, page, rows)
        ctor = {"is_causal": True, "gqa_layout": layout, "query_dtype": torch.bfloat16, "context_dtype": torch.int8,
                "compute_dtype": compute}
        me = types.SimpleNamespace(**ctor, qmax=127, qmin=-128)
        if kind == "decode":
            args, kwargs = (q, None, k8, ks, v8, vs, torch.tensor(kv_lens, dtype=torch.int32), table), {}
            out = ref_attn.MojoPagedDecodeGQAWithKVDequant.forward(me, *args)
            op = "MojoPagedDecodeGQAWithKVDequant"
        else:
            args, kwargs = (q, None, k8, ks, v8, vs, cu(q_lens), table), {"cu_total_seq_lens": cu(kv_lens)}
            out = ref_attn.MojoPagedPrefillGQAWithKVDequant.forward(me, *args, **kwargs)
            op = "MojoPagedPrefillGQAWithKVDequant"
        files[kind].append({"op": op, "ctor": {"kwargs": ctor}, "state": {}, "args": args, "kwargs": kwargs, "out": out})

    for sdt, scdt, page, heads, d, ctx, q_lens, as_plan in STORE_CASES:
        batch = len(ctx)
        tokens = batch if q_lens is None else sum(q_lens)
        end = [c + (1 if q_lens is None else q_lens[i]) for i, c in enumerate(ctx)]
        need = [max((e + page - 1) // page, 1) for e in end]
        total = sum(need) + 1
        table = torch.full((batch, max(need)), -1, dtype=torch.int32)
        free = torch.randperm(total, generator=g, dtype=torch.int32)
        at = 0
        for b, n in enumerate(need):
            table[b, :n] = free[at: at + n]
            at += n
        ks_ = torch.randn(tokens, heads, d, generator=g).to(sdt)
        vs_ = torch.randn(tokens, heads, d, generator=g).to(sdt)
        # scales of both signs, as the reference test draws them (randn), kept away from 0
        kscale = torch.randn(heads, d, generator=g)
        vscale = torch.randn(heads, d, generator=g)
        kscale = (kscale.sign() * kscale.abs().clamp(min=0.02)).to(scdt)
        vscale = (vscale.sign() * vscale.abs().clamp(min=0.02)).to(scdt)
        kc = torch.randint(-128, 128, (total, heads, page, d), generator=g, dtype=torch.int8)
        vc = torch.randint(-128, 128, (total, heads, page, d), generator=g, dtype=torch.int8)
        ctx_t = torch.tensor(ctx, dtype=torch.int32)
        cu_q = None if q_lens is None else cu(q_lens)
        if as_plan:
            args, kwargs = (ks_, vs_, kc, vc, kscale, vscale), {"chunk_metadata": build_paged_kv_chunk_metadata(table, cu_q, ctx_t, page)}
        else:
            args, kwargs = (ks_, vs_, kc, vc, kscale, vscale, table, cu_q, ctx_t), {}
        out = ref_kv.MojoStorePagedKVCacheC8.forward(types.SimpleNamespace(), *[a.clone() if isinstance(a, torch.Tensor) else a for a in args],
                                                     **kwargs)
        files["store"].append({"op": "MojoStorePagedKVCacheC8", "ctor": {"kwargs": {}}, "state": {}, "args": args, "kwargs": kwargs,
                               "out": tuple(out)})
    for name, cases in files.items():
        path = os.path.join(ROOT, "tests", "golden", f"paged_kv_int8_{name}.pt")
        torch.save({"cases": cases}, path)
        print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MOJO_REFERENCE_ROOT", "/root/reference"))
