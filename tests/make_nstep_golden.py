"""Write tests/golden/paged_nstep_swa.pt: reference outputs of `MojoPagedDecodeNstepSWA` (authoring machine only; pytest
does not collect this file).

Usage: python tests/make_nstep_golden.py <reference root>   (or MOJO_REFERENCE_ROOT; nothing else reads it)

The outputs come from the reference's own `MojoPagedDecodeNstepSWA.forward`
(`mojo_opset/experimental/operators/attention.py:1185-1259`), called on CPU.  Each case records the constructor keywords,
the inputs and the output — tensors and scalars only; tests/test_nstep_golden.py pins tests/nstep_golden.py to them bit for
bit and tests/test_hip_nstep_swa.py checks the hip backend against them at the reference's bound (2e-2).  Every row has
``len == 0`` or ``len >= S``: the reference returns NaN for a row shorter than its steps.
"""
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [
    # (layout, local, global, page, steps, hq, hkv, d, dtype, kv_lens) — short rows: the file stays far below 1 MiB
    ("AABB", None, None, 16, 4, 8, 2, 64, torch.bfloat16, [37, 0, 4]),
    ("ABAB", None, None, 16, 3, 8, 1, 64, torch.float16, [33, 3, 18]),
    ("AABB", None, 4, 16, 2, 4, 2, 64, torch.bfloat16, [20, 2, 0]),
    ("ABAB", 5, None, 32, 4, 6, 2, 64, torch.float16, [49, 4, 70]),
    ("AABB", 5, 4, 16, 3, 2, 2, 128, torch.bfloat16, [48, 17, 3]),
    ("ABAB", 0, None, 16, 2, 4, 1, 64, torch.bfloat16, [40, 2]),
    ("AABB", 17, 8, 16, 1, 4, 2, 64, torch.float16, [40, 0, 1]),
    ("ABAB", 255, 4, 16, 4, 8, 1, 64, torch.bfloat16, [300]),
    ("AABB", 7, 3, 16, 2, 4, 4, 96, torch.bfloat16, [29, 2]),          # a geometry of the composed route
]


def paged_inputs(g, hq, hkv, d, kv_lens, page, dtype, steps):
    need = [max((n + page - 1) // page, 0) for n in kv_lens]
    total = sum(need)
    k = torch.randn(total, hkv, page, d, generator=g).to(dtype)
    v = torch.randn(total, hkv, page, d, generator=g).to(dtype)
    table = torch.full((len(kv_lens), max(max(need), 1)), -1, dtype=torch.int32)
    free = torch.randperm(total, generator=g, dtype=torch.int32)
    at = 0
    for b, n in enumerate(need):
        table[b, :n] = free[at: at + n]
        at += n
    q = torch.randn(len(kv_lens), steps, hq, d, generator=g).to(dtype)
    return q, k, v, table


def main(reference_root):
    sys.path.insert(0, reference_root)
    from mojo_opset.experimental.operators import attention as ref

    g = torch.Generator().manual_seed(2027)
    cases = []
    for layout, local, glob, page, steps, hq, hkv, d, dtype, kv_lens in CASES:
        assert all(n == 0 or n >= steps for n in kv_lens)
        q, k, v, table = paged_inputs(g, hq, hkv, d, kv_lens, page, dtype, steps)
        ctor = {"is_causal": True, "gqa_layout": layout, "global_window_size": glob, "local_window_size": local}
        me = types.SimpleNamespace(**ctor, gqa_interleave=layout == "ABAB")
        args = (q, k, v, torch.tensor(kv_lens, dtype=torch.int32), table)
        out = ref.MojoPagedDecodeNstepSWA.forward(me, *args)
        assert not bool(torch.isnan(out.float()).any())
        cases.append({"op": "MojoPagedDecodeNstepSWA", "ctor": {"kwargs": ctor}, "state": {}, "args": args, "kwargs": {},
                      "out": out})
    path = os.path.join(ROOT, "tests", "golden", "paged_nstep_swa.pt")
    torch.save({"cases": cases}, path)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MOJO_REFERENCE_ROOT")
    if not root:
        sys.exit(__doc__)
    main(root)
