"""Write tests/golden/vision_tower.pt: reference outputs of the vision-tower ops (authoring machine only; pytest does not
collect this file).

Usage: python tests/make_vision_tower_golden.py <reference root>   (or MOJO_REFERENCE_ROOT; nothing else reads it)

The outputs come from the reference's own classes, constructed and called on CPU: `mojo_opset/core/operators/attention.py`
MojoSWA with ``is_causal=False`` (recorded under the name this repository gives those semantics, MojoPackedSdpa),
`core/operators/position_embedding.py` MojoVisionRotaryEmbedding2D, MojoApplyVisionRoPE2D and MojoMRoPE,
`experimental/operators/position_embedding.py` MojoMRoPEInplace.  Each case records the constructor keywords, the inputs, the
outputs and the instance's ``extra_repr()`` -- tensors, scalars and strings only; tests/test_vision_tower_golden.py pins
tests/vision_tower_golden.py to them bit for bit.  The cases are small (the file stays under 256 KiB): the GPU tests compute
their goldens from the pinned classes at the shapes they need.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32

PACKED = [
    # (gqa_layout, Hq, Hkv, D, dtype, q lens, kv lens, first K/V row, softmax_scale)
    ("AABB", 2, 1, 64, BF16, [5, 0, 9, 3], [9, 4, 9, 20], 0, None),         # ragged, q_len != kv_len, an empty-query sequence
    ("ABAB", 4, 2, 64, F16, [4, 7, 0, 2], [2, 7, 3, 9], 2, 0.2),            # kv_len < q_len, cu_total_seq_lens[0] > 0
    ("AABB", 2, 2, 96, BF16, [6, 1], [11, 1], 0, None),
    ("ABAB", 8, 1, 128, BF16, [3, 5], [5, 3], 0, None),
]
VISION_GRIDS = [
    # (grids, rope_dim, adapooling_factor): the three grids of the reference's vision test, and one with pooling factor 2
    (((4, 4),), 64, 1), (((8, 6),), 64, 1), (((8, 8), (4, 6)), 64, 1), (((4, 6), (2, 4), (4, 4)), 8, 2),
]
VISION_APPLY = [
    # (T, q heads, k heads, D, dtype, table dtype)
    (5, 3, 2, 8, BF16, F32), (4, 2, 2, 72, F16, F32), (3, 1, 1, 2, F32, F32), (4, 2, 1, 16, BF16, BF16),
]
MROPE = [
    # (T, q heads, k heads, head_dim, sections, interleaved, dtype, table dtype, 3-D tables)
    (3, 4, 2, 32, [4, 6, 6], False, BF16, F32, True),      # chunked
    (3, 4, 2, 32, [6, 5, 5], True, F16, F32, True),        # interleaved
    (2, 2, 1, 48, [4, 6, 6], False, BF16, F32, True),      # partial rotation: a pass-through tail of 16
    (3, 2, 2, 12, [1, 1, 2], True, F32, F32, True),
    (2, 2, 1, 32, [4, 6, 6], False, BF16, F32, False),     # merged [T, half] tables
    (2, 2, 1, 32, [4, 6, 6], True, BF16, BF16, True),      # 16-bit tables
]


def record(cls, name, ctor, args, kwargs=None, **extra):
    op = cls(**ctor)
    recorded = tuple(a.clone() if isinstance(a, torch.Tensor) else a for a in args)
    with torch.no_grad():
        out = op.forward(*args, **(kwargs or {}))
    return {"op": name, "ctor": {"kwargs": ctor}, "state": {}, "args": recorded, "kwargs": kwargs or {}, "out": out,
            "repr": op.extra_repr(), **extra}


def cumulative(lens, first=0):
    return torch.tensor([first] + [first + sum(lens[:i + 1]) for i in range(len(lens))], dtype=torch.int32)


def main(reference_root):
    sys.path.insert(0, reference_root)
    from mojo_opset.core.operators import attention as ref_attn
    from mojo_opset.core.operators import position_embedding as ref_pos
    from mojo_opset.experimental.operators import position_embedding as ref_exp

    g = torch.Generator().manual_seed(2033)
    cases = []
    for layout, hq, hkv, dim, dtype, q_lens, kv_lens, first, scale in PACKED:
        q = torch.randn(sum(q_lens), hq, dim, generator=g).to(dtype)
        k = torch.randn(first + sum(kv_lens) + 3, hkv, dim, generator=g).to(dtype)
        v = torch.randn(first + sum(kv_lens) + 3, hkv, dim, generator=g).to(dtype)
        case = record(ref_attn.MojoSWA, "MojoPackedSdpa", {"is_causal": False, "gqa_layout": layout},
                      (q, k, v, cumulative(q_lens), cumulative(kv_lens, first), scale))
        case["reference_repr"] = case["repr"]                # MojoSWA's; the op of this repository has its own constructor
        case["ctor"] = {"kwargs": {"gqa_layout": layout}}
        del case["repr"]
        cases.append(case)
    for grids, rope_dim, pool in VISION_GRIDS:
        cases.append(record(ref_pos.MojoVisionRotaryEmbedding2D, "MojoVisionRotaryEmbedding2D",
                            {"rope_theta": 10000.0, "rope_dim": rope_dim, "adapooling_factor": pool},
                            (torch.tensor(grids, dtype=torch.int32),)))
    for tokens, nq, nk, dim, dtype, tdtype in VISION_APPLY:
        q = torch.randn(tokens, nq, dim, generator=g).to(dtype)
        k = torch.randn(tokens, nk, dim, generator=g).to(dtype)
        angle = torch.rand(tokens, dim, generator=g) * 6.0
        cases.append(record(ref_pos.MojoApplyVisionRoPE2D, "MojoApplyVisionRoPE2D", {}, (q, k, angle.cos().to(tdtype), angle.sin().to(tdtype))))
    for tokens, hq, hk, hd, sec, inter, dtype, tdtype, three in MROPE:
        half = sum(sec)
        angle = torch.rand(*((3, tokens, half) if three else (tokens, half)), generator=g) * 6.0
        cos, sin = angle.cos().to(tdtype), angle.sin().to(tdtype)
        forms = [(ref_pos.MojoMRoPE, "MojoMRoPE", {}), (ref_exp.MojoMRoPEInplace, "MojoMRoPEInplace", {"inplace": True})]
        if not cases or cases[-1]["op"] != "MojoMRoPEInplace":   # the out-of-place form of the serving class: once
            forms.append((ref_exp.MojoMRoPEInplace, "MojoMRoPEInplace", {"inplace": False}))
        for cls, name, ctor in forms:
            q = torch.randn(tokens, hq * hd, generator=g).to(dtype)
            k = torch.randn(tokens, hk * hd, generator=g).to(dtype)
            cases.append(record(cls, name, ctor, (q, k, cos, sin, list(sec), inter, hd)))
    path = os.path.join(ROOT, "tests", "golden", "vision_tower.pt")
    torch.save({"cases": cases}, path, _use_new_zipfile_serialization=False)   # (the zip form spends 64-byte padding and a
                                                                                 #  directory entry per tensor: a third of this file)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MOJO_REFERENCE_ROOT")
    if not root:
        sys.exit(__doc__)
    main(root)
