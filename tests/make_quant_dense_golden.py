"""Write tests/golden/quant_dense.pt: reference outputs of the dense W8A8 quantiser ops, `QUANT_DENSE_OPS` (authoring machine
only; pytest does not collect this file).

Usage: python tests/make_quant_dense_golden.py <reference root>   (or MOJO_REFERENCE_ROOT; nothing else reads it)

The outputs come from the reference's own torch classes (`mojo_opset/core/operators/quantize.py`, `normalization.py`),
constructed and called on CPU.  Each case records the constructor keywords, the parameters, the inputs and the outputs —
tensors and scalars only; tests/test_quant_dense_golden.py pins tests/quant_dense_golden.py to them bit for bit and
tests/test_hip_quant_dense.py runs the hip backend on them.  Shapes are small: the reference's grouped static cases, rows of
128, 257 and 1000, the reference's four `dequant_swiglu_quant_cases` plus one with an empty expert and one with
``activate_left``, a bias and no activation scale.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16, F16, F32, I8, F8 = torch.bfloat16, torch.float16, torch.float32, torch.int8, torch.float8_e4m3fn

# (shape, dtype, quant dtype, symmetric, smooth scale?)
NORM_CASES = [
    ((1, 128), BF16, I8, True, False),
    ((7, 257), F16, I8, False, True),
    ((2, 1000), F32, F8, True, True),
    ((2, 3, 128), BF16, I8, True, True),
    ((3, 257), BF16, F8, True, False),
]
# (shape, scale shape, dtype, quant dtype)
STATIC_CASES = [
    ((2, 4, 128), (4, 128), BF16, I8),
    ((5, 2, 16, 32), (16, 32), F16, I8),
    ((7, 257), (257,), F32, F8),
    ((2, 1000), (1000,), BF16, F8),
]
# (shape, scale shape, input dtype, output dtype)
DEQUANT_CASES = [
    ((2, 4, 128), (4, 128), I8, BF16),
    ((5, 2, 16, 32), (16, 32), I8, F32),
    ((7, 257), (7, 1), I8, F16),
    ((2, 1000), (1000,), F8, F32),
    ((3, 2, 128), (3, 2, 1), F8, BF16),
]
# (tokens, hidden, token_count, activate_left, bias: None | "flat" | "grouped", activation scale?)
SWIGLU_CASES = [
    (12, 64, [4, 3, 5], False, None, True),
    (20, 128, [6, 4, 7, 3], False, None, True),
    (24, 256, [5, 8, 4, 7], False, None, True),
    (30, 512, [6, 3, 8, 5, 8], False, None, True),
    (12, 64, [4, 0, 8], False, "grouped", True),
    (20, 128, [6, 4, 7, 3], True, "flat", False),
    (9, 257, None, True, None, True),
]


def main(reference_root):
    sys.path.insert(0, reference_root)
    from mojo_opset.core.operators import normalization as ref_norm
    from mojo_opset.core.operators import quantize as ref_quant

    def torch_impl(cls):
        return cls._registry.get("torch")

    g = torch.Generator().manual_seed(2029)
    cases = []

    def record(name, ref_cls, kwargs, state, args, call_kwargs=None):
        op = ref_cls(**kwargs)
        with torch.no_grad():
            for k, v in state.items():
                getattr(op, k).copy_(v)
            out = op(*args, **(call_kwargs or {}))
        out = tuple(o.detach().clone() for o in out) if isinstance(out, tuple) else out.detach().clone()
        cases.append({"op": name, "ctor": {"kwargs": kwargs}, "state": state, "args": args, "kwargs": call_kwargs or {}, "out": out})

    def affine(dim):
        return {"weight": torch.randn(dim, generator=g), "bias": torch.randn(dim, generator=g)}

    for shape, dtype, qd, symmetric, smooth in NORM_CASES:
        dim = shape[-1]
        x = torch.randn(shape, generator=g).to(dtype)
        sm = (torch.rand(dim, generator=g) + 0.5) if smooth else None
        common = {"norm_size": dim, "eps": 1e-5, "quant_dtype": qd, "symmetric": symmetric}
        record("MojoRMSNormQuant", torch_impl(ref_norm.MojoRMSNormQuant), dict(common), {"weight": torch.randn(dim, generator=g)}, (x, sm))
        record("MojoLayerNormQuant", torch_impl(ref_norm.MojoLayerNormQuant), dict(common), affine(dim), (x, sm))
        for pos in ("pre", "post"):
            r = torch.randn(shape, generator=g).to(dtype)
            record("MojoResidualAddLayerNormQuant", torch_impl(ref_norm.MojoResidualAddLayerNormQuant), dict(common, norm_pos=pos),
                   affine(dim), (x, r, sm))
    x = torch.randn(3, 128, generator=g).to(BF16)
    plain = {"norm_size": 128, "elementwise_affine": False}
    record("MojoLayerNormQuant", torch_impl(ref_norm.MojoLayerNormQuant), dict(plain), {}, (x, None))
    record("MojoResidualAddLayerNormQuant", torch_impl(ref_norm.MojoResidualAddLayerNormQuant), dict(plain, norm_pos="post"), {},
           (x, torch.randn(3, 128, generator=g).to(BF16), torch.rand(128, generator=g) + 0.5))

    for shape, scale_shape, dtype, qd in STATIC_CASES:
        x = torch.randn(shape, generator=g).to(dtype)
        lead = tuple(range(len(shape) - len(scale_shape)))
        scale = (x.float().abs().amax(dim=lead) / (127 if qd == I8 else 448)).clamp(min=1e-10)
        record("MojoStaticQuant", torch_impl(ref_quant.MojoStaticQuant), {"input_size": scale_shape, "quant_dtype": qd}, {"scale": scale}, (x,))

    for shape, scale_shape, in_dtype, out_dtype in DEQUANT_CASES:
        if in_dtype == I8:
            q = torch.randint(-128, 128, shape, generator=g, dtype=torch.int32).to(I8)
        else:
            q = (torch.randn(shape, generator=g) * 150).clamp(-448, 448).to(F8)
        scale = torch.rand(scale_shape, generator=g) * 0.05 + 1e-3
        record("MojoDequant", torch_impl(ref_quant.MojoDequant), {"output_dtype": out_dtype}, {}, (q, scale))

    for tokens, hidden, counts, left, bias_kind, with_act in SWIGLU_CASES:
        experts = len(counts) if counts is not None else 1
        x = torch.randint(-1024, 1024, (tokens, 2 * hidden), generator=g, dtype=torch.int32)
        act = torch.rand(tokens, generator=g) if with_act else None
        bias = {None: None, "flat": torch.randn(2 * hidden, generator=g), "grouped": torch.randn(experts, 2 * hidden, generator=g)}[bias_kind]
        state = {"weight_scale": torch.rand(experts, 2 * hidden, generator=g) * 0.01, "quant_scale": torch.rand(experts, hidden, generator=g)}
        token_count = None if counts is None else torch.tensor(counts, dtype=torch.int64)
        record("MojoDequantSwiGLUQuant", torch_impl(ref_quant.MojoDequantSwiGLUQuant),
               {"expert_num": experts, "hidden_size": hidden, "activate_left": left, "quant_mode": 1}, state, (x, act, bias, None, token_count))

    path = os.path.join(ROOT, "tests", "golden", "quant_dense.pt")
    torch.save({"cases": cases}, path)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MOJO_REFERENCE_ROOT")
    if not root:
        sys.exit(__doc__)
    main(root)
