"""Write tests/golden/swa_packed.pt: reference outputs of `MojoSWA` (authoring machine only; pytest does not collect this
file).

Usage: python tests/make_swa_packed_golden.py <reference root>   (or MOJO_REFERENCE_ROOT; nothing else reads it)

The outputs come from the reference's own `MojoSWA.forward` (`mojo_opset/core/operators/attention.py:774-835`), called on
CPU.  Each case records the constructor keywords, the inputs and the output — tensors and scalars only;
tests/test_swa_packed_golden.py pins tests/swa_packed_golden.py to them bit for bit and tests/test_hip_swa_packed.py checks
the hip backend against them at the reference's bound (2e-2).  Every sequence has ``q_len >= 1`` and ``kv_len >= q_len``: the
reference is undefined otherwise.  The queries fill ``[0, cu_q_lens[-1])`` exactly (the reference leaves other rows
uninitialised); the keys may start behind ``lead`` unused tokens and end before ``tail`` more.
"""
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [
    # (layout, local, global, hq, hkv, d, dtype, [(q_len, kv_len)], lead, tail) — short: the file stays far below 1 MiB.
    # Sequence starts in K/V fall off every multiple of 4, 16 and 64; kv_len == q_len sits next to cached prefixes.
    ("AABB", None, None, 4, 1, 64, torch.bfloat16, [(21, 21), (5, 38), (1, 1)], 0, 0),
    ("ABAB", None, None, 8, 1, 64, torch.float16, [(17, 17), (3, 18), (9, 35)], 5, 3),
    ("AABB", None, 4, 2, 1, 64, torch.bfloat16, [(20, 20), (2, 9), (34, 34)], 1, 0),
    ("ABAB", 5, None, 4, 2, 64, torch.float16, [(25, 25), (4, 38)], 0, 7),
    ("AABB", 5, 4, 1, 1, 128, torch.bfloat16, [(24, 24), (17, 17), (3, 40)], 3, 1),
    ("ABAB", 0, None, 4, 1, 64, torch.bfloat16, [(20, 20), (2, 13)], 0, 0),
    ("AABB", 17, 8, 2, 1, 96, torch.float16, [(20, 45), (1, 1), (29, 29)], 2, 0),
    ("ABAB", 63, 4, 2, 1, 64, torch.bfloat16, [(66, 66), (3, 70)], 0, 0),
    ("AABB", 7, 3, 2, 2, 96, torch.bfloat16, [(29, 29), (2, 40)], 6, 2),
    ("ABAB", None, None, 2, 1, 128, torch.float16, [(33, 33), (10, 31)], 0, 0),
]


def packed_inputs(g, hq, hkv, d, lens, lead, tail, dtype):
    cu_q, cu_kv = [0], [lead]
    for q_len, kv_len in lens:
        cu_q.append(cu_q[-1] + q_len)
        cu_kv.append(cu_kv[-1] + kv_len)
    q = torch.randn(cu_q[-1], hq, d, generator=g).to(dtype)
    k = torch.randn(cu_kv[-1] + tail, hkv, d, generator=g).to(dtype)
    v = torch.randn(cu_kv[-1] + tail, hkv, d, generator=g).to(dtype)
    return q, k, v, torch.tensor(cu_q, dtype=torch.int32), torch.tensor(cu_kv, dtype=torch.int32)


def main(reference_root):
    sys.path.insert(0, reference_root)
    from mojo_opset.core.operators import attention as ref

    g = torch.Generator().manual_seed(2028)
    cases = []
    for layout, local, glob, hq, hkv, d, dtype, lens, lead, tail in CASES:
        assert all(q_len >= 1 and kv_len >= q_len for q_len, kv_len in lens)
        args = packed_inputs(g, hq, hkv, d, lens, lead, tail, dtype)
        ctor = {"is_causal": True, "gqa_layout": layout, "global_window_size": glob, "local_window_size": local}
        me = types.SimpleNamespace(**ctor, gqa_interleave=layout == "ABAB")
        out = ref.MojoSWA.forward(me, *args)
        assert not bool(torch.isnan(out.float()).any())
        cases.append({"op": "MojoSWA", "ctor": {"kwargs": ctor}, "state": {}, "args": args, "kwargs": {}, "out": out})
    path = os.path.join(ROOT, "tests", "golden", "swa_packed.pt")
    torch.save({"cases": cases}, path)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MOJO_REFERENCE_ROOT")
    if not root:
        sys.exit(__doc__)
    main(root)
