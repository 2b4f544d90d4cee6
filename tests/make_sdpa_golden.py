"""Write tests/golden/sdpa.pt: reference outputs of `MojoSdpa` (authoring machine only; pytest does not collect this file).

Usage: python tests/make_sdpa_golden.py <reference root>   (or MOJO_REFERENCE_ROOT; nothing else reads it)

The outputs come from the reference's own `MojoSdpa.forward` (`mojo_opset/core/operators/attention.py:466-501`), called on CPU.
Each case records the constructor keywords, the inputs and the output — tensors and scalars only;
tests/test_sdpa_golden.py pins tests/sdpa_golden.py to them bit for bit and tests/test_hip_sdpa.py checks the hip backend
against them at the project's attention bound (2e-2).  Every row of every mask keeps at least one key visible: the reference
is NaN or unspecified otherwise.
"""
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [
    # (scale, enable_gqa, B, Hq, Hkv, Sq, Sk, D, dtype, mask form, token-major views) — short: the file stays below 1 MiB.
    # Sk falls on and off the 64-key tile, Sq < Sk, Sq == Sk and Sq > Sk (cross-attention) all occur, B is 1 and 3.
    (None, False, 1, 2, 2, 33, 33, 64, torch.bfloat16, None, True),
    (None, True, 3, 8, 1, 9, 65, 64, torch.float16, None, False),
    (0.25, True, 1, 4, 2, 40, 12, 96, torch.bfloat16, None, True),
    (None, True, 1, 4, 1, 21, 63, 128, torch.float16, "bool_2d", False),
    (None, False, 3, 2, 2, 12, 70, 64, torch.bfloat16, "bool_b1", False),
    (None, False, 3, 2, 2, 9, 64, 128, torch.bfloat16, "key_padding", True),
    (None, False, 1, 1, 1, 70, 70, 96, torch.float16, "block", False),
    (1.0, False, 1, 4, 4, 24, 24, 64, torch.bfloat16, "bias", False),
    (1.0, False, 1, 2, 2, 19, 40, 64, torch.float16, "bias_fp32", False),
    (None, True, 1, 2, 1, 16, 130, 128, torch.bfloat16, "bias_inf", False),
    (None, False, 3, 1, 1, 5, 1, 64, torch.float16, None, False),
]


def block_mask(sq, sk, block=32):
    """Block-diagonal plus causal blocks: query block i sees key blocks 0 .. i (the boolean block mask of the reference's tests)."""
    return (torch.arange(sq)[:, None] // block) >= (torch.arange(sk)[None, :] // block)


def make_mask(g, form, b, hq, sq, sk, dtype):
    if form is None:
        return None
    if form == "block":
        return block_mask(sq, sk)
    if form in ("bias", "bias_fp32", "bias_inf"):
        bias = torch.randn(1, hq, sq, sk, generator=g).to(torch.float32 if form == "bias_fp32" else dtype)
        if form == "bias_inf":
            hide = torch.rand(1, hq, sq, sk, generator=g) < 0.3
            hide[..., 0] = False
            bias = bias.masked_fill(hide, float("-inf"))
        return bias
    shape = {"bool_2d": (sq, sk), "bool_b1": (b, 1, sq, sk), "key_padding": (b, 1, 1, sk)}[form]
    m = torch.rand(shape, generator=g) < 0.6
    m[..., torch.randint(0, sk, (1,), generator=g).item()] = True      # one visible key in every row
    return m


def sdpa_inputs(g, b, hq, hkv, sq, sk, d, dtype, token_major):
    if token_major:                                        # [B,S,H,D] memory seen as [B,H,S,D]
        q = torch.randn(b, sq, hq, d, generator=g).to(dtype).transpose(1, 2)
        k = torch.randn(b, sk, hkv, d, generator=g).to(dtype).transpose(1, 2)
        v = torch.randn(b, sk, hkv, d, generator=g).to(dtype).transpose(1, 2)
    else:
        q = torch.randn(b, hq, sq, d, generator=g).to(dtype)
        k = torch.randn(b, hkv, sk, d, generator=g).to(dtype)
        v = torch.randn(b, hkv, sk, d, generator=g).to(dtype)
    return q, k, v


def main(reference_root):
    sys.path.insert(0, reference_root)
    from mojo_opset.core.operators import attention as ref

    g = torch.Generator().manual_seed(2031)
    cases = []
    for scale, gqa, b, hq, hkv, sq, sk, d, dtype, form, token_major in CASES:
        q, k, v = sdpa_inputs(g, b, hq, hkv, sq, sk, d, dtype, token_major)
        mask = make_mask(g, form, b, hq, sq, sk, dtype)
        ctor = {"scale": scale, "enable_gqa": gqa}
        out = ref.MojoSdpa.forward(types.SimpleNamespace(**ctor), q, k, v, mask)
        assert bool(torch.isfinite(out.float()).all())
        cases.append({"op": "MojoSdpa", "ctor": {"kwargs": ctor}, "state": {}, "args": (q, k, v, mask), "kwargs": {},
                      "out": out, "mask_form": form or "none"})
    path = os.path.join(ROOT, "tests", "golden", "sdpa.pt")
    torch.save({"cases": cases}, path)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MOJO_REFERENCE_ROOT")
    if not root:
        sys.exit(__doc__)
    main(root)
