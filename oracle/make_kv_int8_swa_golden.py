"""Write tests/golden/paged_kv_int8_swa_decode.pt and _prefill.pt: reference outputs of sliding-window attention over the
int8 paged KV cache (authoring machine only).

Usage: python oracle/make_kv_int8_swa_golden.py [reference root]   (default: MOJO_REFERENCE_ROOT, else /root/reference; nothing else reads it)

The outputs come from the reference's own `MojoPagedDecodeSWAWithKVDequant.forward` and
`MojoPagedPrefillSWAWithKVDequant.forward` (`experimental/operators/attention.py:803-1151`), called on CPU.  Each case
records the constructor keywords, the inputs and the output; tests/test_kv_int8_swa_golden.py pins
oracle/kv_int8_swa.py to them bit for bit and tests/test_hip_kv_int8_swa.py runs the hip backend on them.  Two files:
all twelve cases in one exceed the size bound of a committed file.
"""
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.make_kv_int8_golden import paged_inputs  # noqa: E402
from oracle.paged import cu  # noqa: E402

BF16, INT8 = torch.bfloat16, torch.int8

# (layout, compute dtype, page, hq, hkv, d, kv_lens, global window, local window)
DECODE_CASES = [
    ("AABB", BF16, 16, 4, 4, 64, [100, 0, 33], 4, 31),             # group 1, a zero-length row
    ("ABAB", BF16, 32, 4, 2, 96, [70, 1], None, 15),               # group 2, local only
    ("AABB", BF16, 128, 4, 1, 128, [300, 128], 20, None),          # group 4, global only
    ("ABAB", BF16, 16, 8, 1, 64, [49, 16, 300], 4, 255),           # group 8, the reference's windows
    ("AABB", BF16, 16, 4, 2, 128, [257, 40], 40, 0),               # local_window_size = 0: the query's own key
    ("ABAB", INT8, 16, 4, 2, 64, [40, 17], 4, 7),                  # compute_dtype=int8 (golden only)
]
# (layout, compute dtype, page, hq, hkv, d, kv_lens, q_lens, global window, local window)
PREFILL_CASES = [
    ("AABB", BF16, 16, 2, 2, 64, [50, 0, 20], [50, 0, 20], 4, 15),     # group 1, an empty sequence
    ("ABAB", BF16, 32, 4, 2, 96, [70, 30], [70, 30], None, 31),
    ("AABB", BF16, 128, 4, 1, 128, [140], [140], 20, None),
    ("ABAB", BF16, 16, 8, 1, 64, [100, 37], [64, 37], 4, 255),
    ("AABB", BF16, 16, 4, 1, 64, [300], [40], 4, 63),                  # chunked prefill on a cached prefix
    ("AABB", INT8, 16, 4, 2, 64, [40, 33], [20, 33], 4, 7),            # compute_dtype=int8 (golden only)
]


def main(reference_root):
    sys.path.insert(0, reference_root)
    from mojo_opset.experimental.operators import attention as ref_attn

    g = torch.Generator().manual_seed(2028)
    files = {"decode": [], "prefill": []}
    for kind, cases in (("decode", DECODE_CASES), ("prefill", PREFILL_CASES)):
        for case in cases:
            layout, compute, page, hq, hkv, d, kv_lens = case[:7]
            q_lens = case[7] if kind == "prefill" else None
            glob, local = case[-2:]
            batch = len(kv_lens)
            rows = batch if kind == "decode" else sum(q_lens)
            q, k8, ks, v8, vs, table = paged_inputs(g, batch, hq, hkv, d, kv_lens, page, rows)
            ctor = {"is_causal": True, "gqa_layout": layout, "global_window_size": glob, "local_window_size": local,
                    "query_dtype": BF16, "context_dtype": INT8, "compute_dtype": compute}
            me = types.SimpleNamespace(**ctor, gqa_interleave=layout == "ABAB", qmax=127, qmin=-128)
            if kind == "decode":
                args, kwargs = (q, None, k8, ks, v8, vs, torch.tensor(kv_lens, dtype=torch.int32), table), {}
                out = ref_attn.MojoPagedDecodeSWAWithKVDequant.forward(me, *args)
                op = "MojoPagedDecodeSWAWithKVDequant"
            else:
                args, kwargs = (q, None, k8, ks, v8, vs, cu(q_lens), table), {"cu_total_seq_lens": cu(kv_lens)}
                out = ref_attn.MojoPagedPrefillSWAWithKVDequant.forward(me, *args, **kwargs)
                op = "MojoPagedPrefillSWAWithKVDequant"
            assert not torch.isnan(out.float()).any(), case
            files[kind].append({"op": op, "ctor": {"kwargs": ctor}, "state": {}, "args": args, "kwargs": kwargs, "out": out})
    for name, cases in files.items():
        path = os.path.join(ROOT, "tests", "golden", f"paged_kv_int8_swa_{name}.pt")
        torch.save({"cases": cases}, path)
        print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MOJO_REFERENCE_ROOT", "/root/reference"))
