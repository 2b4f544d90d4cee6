"""Write tests/golden/dit_block.pt: reference outputs of the DiT block ops (authoring machine only; pytest does not collect
this file).

Usage: python tests/make_dit_block_golden.py <reference root>   (or MOJO_REFERENCE_ROOT; nothing else reads it)

The outputs come from the reference's own classes (`mojo_opset/core/operators/normalization.py` MojoLayerNorm and
MojoResidualAddLayerNorm, `activation.py` MojoGelu and MojoSilu, `experimental/operators/position_embedding.py` MojoGridRoPE),
constructed and called on CPU.  Each case records the constructor keywords, the parameters, the inputs, the outputs and the
instance's ``extra_repr()`` -- tensors, scalars and strings only; tests/test_dit_block_golden.py pins tests/dit_block_golden.py
to them bit for bit.  The cases are small (the file stays under 256 KiB): the GPU tests compute their goldens from the pinned
classes at the shapes they need.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32

LAYERNORM = [
    # (rows shape, dim, dtype, eps, elementwise_affine)
    ((3,), 40, BF16, 1e-5, True), ((2, 2), 40, F16, 1e-6, False), ((2,), 1000, F32, 1e-5, True), ((2,), 24, F32, 1e-6, False),
    ((2,), 1, BF16, 1e-5, True), ((3,), 7, F16, 1e-5, True), ((1,), 2, BF16, 1e-6, False),
]
RESIDUAL_LAYERNORM = [
    # (rows shape, dim, dtype, eps, norm_pos)
    ((3,), 40, BF16, 1e-5, "pre"), ((2, 2), 40, F16, 1e-6, "post"), ((2,), 1000, F32, 1e-5, "pre"), ((2,), 7, BF16, 1e-5, "post"),
    ((2,), 1, F16, 1e-5, "pre"),
]
GRID_ROPE = [
    # (grids per sample, padding behind the largest, heads, head_dim, dtype, one shared frequency tensor)
    ([(1, 2, 3), (1, 2, 3)], 2, 2, 8, BF16, True), ([(2, 2, 2), (1, 1, 1), (1, 3, 2)], 0, 3, 4, F16, False),
    ([(1, 1, 5)], 1, 2, 2, BF16, True), ([(2, 1, 2), (1, 2, 1)], 3, 1, 16, F32, False),
]


def activation_inputs(dtype):
    """Every 16th bit pattern of a 16-bit type (all exponents, both signs, zeros, infinities, NaNs), or 2048 random fp32
    values and the edge values the GPU test names."""
    if dtype == F32:
        g = torch.Generator().manual_seed(77)
        edge = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 88.0, -88.0, 1e4, -1e4], dtype=F32)
        return torch.cat([torch.randn(2048, generator=g) * 3, edge])
    return torch.arange(0, 1 << 16, 16, dtype=torch.int32).to(torch.int16).view(dtype)


def grid_frequencies(cells, head_dim):
    """Unit phases [cells, 1, head_dim / 2], complex64: the construction of the reference's own test."""
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, head_dim, 2, dtype=F32) / head_dim))
    angle = torch.arange(cells, dtype=F32)[:, None] * inv_freq[None, :]
    return torch.complex(angle.cos()[:, None, :], angle.sin()[:, None, :])


def record(cls, name, ctor, state, args, **extra):
    op = cls(**ctor)
    with torch.no_grad():
        for k, v in state.items():
            getattr(op, k).copy_(v)
        out = op.forward(*args)
    return {"op": name, "ctor": {"kwargs": ctor}, "state": state, "args": args, "kwargs": {}, "out": out,
            "repr": op.extra_repr(), **extra}


def main(reference_root):
    sys.path.insert(0, reference_root)
    from mojo_opset.core.operators import activation as ref_act
    from mojo_opset.core.operators import normalization as ref_norm
    from mojo_opset.experimental.operators import position_embedding as ref_pos

    g = torch.Generator().manual_seed(2032)
    cases = []
    for lead, dim, dtype, eps, affine in LAYERNORM:
        x = (torch.randn(*lead, dim, generator=g) * 2 + 0.5).to(dtype)
        state = {"weight": torch.randn(dim, generator=g).to(dtype), "bias": torch.randn(dim, generator=g).to(dtype)} if affine else {}
        cases.append(record(ref_norm.MojoLayerNorm, "MojoLayerNorm", {"norm_size": dim, "eps": eps, "elementwise_affine": affine, "dtype": dtype},
                            state, (x,)))
    for lead, dim, dtype, eps, pos in RESIDUAL_LAYERNORM:
        x = (torch.randn(*lead, dim, generator=g) * 2 + 0.5).to(dtype)
        r = torch.randn(*lead, dim, generator=g).to(dtype)
        state = {"weight": torch.randn(dim, generator=g).to(dtype), "bias": torch.randn(dim, generator=g).to(dtype)}
        cases.append(record(ref_norm.MojoResidualAddLayerNorm, "MojoResidualAddLayerNorm",
                            {"norm_size": dim, "eps": eps, "norm_pos": pos, "dtype": dtype}, state, (x, r)))
    for name, cls in (("MojoGelu", ref_act.MojoGelu), ("MojoSilu", ref_act.MojoSilu)):
        for dtype in (BF16, F16, F32):
            cases.append(record(cls, name, {}, {}, (activation_inputs(dtype),)))
    for grids, pad, heads, dim, dtype, shared in GRID_ROPE:
        cells = [f * h * w for f, h, w in grids]
        tokens = max(cells) + pad
        x = torch.randn(len(grids), tokens, heads, dim, generator=g).to(dtype)
        one = grid_frequencies(max(cells), dim)
        freqs = [one] * len(grids) if shared else [grid_frequencies(c, dim) for c in cells]
        cases.append(record(ref_pos.MojoGridRoPE, "MojoGridRoPE", {}, {}, (x, torch.tensor(grids, dtype=torch.int32), freqs),
                            shared=shared))
    path = os.path.join(ROOT, "tests", "golden", "dit_block.pt")
    torch.save({"cases": cases}, path)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MOJO_REFERENCE_ROOT")
    if not root:
        sys.exit(__doc__)
    main(root)
