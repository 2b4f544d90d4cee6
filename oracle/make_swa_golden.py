"""Write tests/golden/paged_swa.pt (decode) and paged_swa_prefill.pt: reference outputs of the sliding-window pair (authoring machine only).

Usage: python oracle/make_swa_golden.py [reference root]   (default: MOJO_REFERENCE_ROOT, else /root/reference; nothing else reads it)

The outputs come from the reference's own `MojoPagedDecodeSWA.forward` / `MojoPagedPrefillSWA.forward`
(`mojo_opset/core/operators/attention.py:561-741`), called on CPU.  Each case records the constructor keywords, the
inputs and the output; tests/test_swa_golden.py pins oracle/swa.py to them bit for bit and tests/test_hip_swa.py
checks the hip backend against them at the reference's bound (2e-2).
"""
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.paged import cu  # noqa: E402


def paged_inputs(g, batch, hq, hkv, d, kv_lens, page, dtype, q_rows):
    """Random K/V pools (no spare page) and shuffled tables padded with -1; ``q_rows`` query rows."""
    need = [max((n + page - 1) // page, 0) for n in kv_lens]
    width = max(max(need), 1)
    total = sum(need)
    k = torch.randn(total, hkv, page, d, generator=g).to(dtype)
    v = torch.randn(total, hkv, page, d, generator=g).to(dtype)
    table = torch.full((batch, width), -1, dtype=torch.int32)
    free = torch.randperm(total, generator=g, dtype=torch.int32)
    at = 0
    for b, n in enumerate(need):
        table[b, :n] = free[at: at + n]
        at += n
    q = torch.randn(q_rows, hq, d, generator=g).to(dtype)
    return q, k, v, table


CASES = [
    # (kind, layout, local, global, page, hq, hkv, d, dtype, kv_lens, q_lens).  Sized to keep the file under 1 MiB: one
    # Mistral-like (4, 1023) decode case, the rest short (prefill at (4, 1023): tests/test_hip_swa.py); pages of 1024 tokens (256 KiB of K/V per page at the smallest head)
    # are exercised by tests/test_hip_swa.py against oracle/swa.py instead.
    ("decode", "AABB", 1023, 4, 16, 4, 1, 64, torch.bfloat16, [1060, 0], None),
    ("decode", "ABAB", 255, 4, 32, 4, 2, 64, torch.bfloat16, [262, 1], None),
    ("decode", "AABB", 0, None, 16, 2, 1, 128, torch.float16, [40, 17], None),
    ("decode", "ABAB", 17, None, 16, 4, 2, 96, torch.bfloat16, [40, 18, 0], None),
    ("decode", "AABB", None, 8, 128, 8, 1, 64, torch.bfloat16, [130], None),
    ("decode", "AABB", 5000, 4, 16, 2, 1, 64, torch.bfloat16, [70, 33], None),
    ("prefill", "ABAB", 255, 4, 32, 4, 2, 64, torch.bfloat16, [262, 0, 20], [20, 5, 20]),
    ("prefill", "AABB", 0, None, 16, 1, 1, 96, torch.float16, [70], [70]),
    ("prefill", "ABAB", 17, None, 16, 4, 2, 128, torch.bfloat16, [50, 30], [20, 30]),
    ("prefill", "AABB", None, 8, 16, 8, 1, 64, torch.bfloat16, [100], [64]),
    ("prefill", "AABB", 5000, 4, 16, 2, 1, 64, torch.bfloat16, [100, 37], [70, 37]),
    # chunked prefill on a cached prefix: the window of the first rows starts inside the cache
    ("prefill", "AABB", 255, 4, 16, 4, 1, 64, torch.bfloat16, [300], [40]),
]


def main(reference_root):
    sys.path.insert(0, reference_root)
    from mojo_opset.core.operators import attention as ref

    g = torch.Generator().manual_seed(2026)
    cases = []
    for kind, layout, local, glob, page, hq, hkv, d, dtype, kv_lens, q_lens in CASES:
        batch = len(kv_lens)
        rows = batch if kind == "decode" else sum(q_lens)
        q, k, v, table = paged_inputs(g, batch, hq, hkv, d, kv_lens, page, dtype, rows)
        ctor = {"is_causal": True, "gqa_layout": layout, "global_window_size": glob, "local_window_size": local}
        me = types.SimpleNamespace(**ctor, gqa_interleave=layout == "ABAB")
        if kind == "decode":
            lens = torch.tensor(kv_lens, dtype=torch.int32)
            args, kwargs = (q, k, v, lens, table), {}
            out = ref.MojoPagedDecodeSWA.forward(me, *args)
            op = "MojoPagedDecodeSWA"
        else:
            cu_q, cu_kv = cu(q_lens), cu(kv_lens)
            args, kwargs = (q, k, v, cu_q, table), {"cu_total_seq_lens": cu_kv}
            out = ref.MojoPagedPrefillSWA.forward(me, *args, **kwargs)
            # the reference leaves rows of sequences without keys uninitialised (torch.empty_like); both backends zero them
            for b in range(batch):
                if kv_lens[b] <= 0:
                    out[int(cu_q[b]): int(cu_q[b + 1])] = 0
            op = "MojoPagedPrefillSWA"
        cases.append({"op": op, "ctor": {"kwargs": ctor}, "state": {}, "args": args, "kwargs": kwargs, "out": out})
    # two files, each under the 1 MiB bound of a committed file
    for name, kind in (("paged_swa", "MojoPagedDecodeSWA"), ("paged_swa_prefill", "MojoPagedPrefillSWA")):
        path = os.path.join(ROOT, "tests", "golden", name + ".pt")
        mine = [c for c in cases if c["op"] == kind]
        torch.save({"cases": mine}, path)
        print(path, os.path.getsize(path), "bytes,", len(mine), "cases")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MOJO_REFERENCE_ROOT", "/root/reference"))
