"""Write tests/golden/short_conv.pt: reference outputs of the short-convolution ops (authoring machine only; pytest does not
collect this file).

Usage: python tests/make_short_conv_golden.py <reference root>   (or MOJO_REFERENCE_ROOT; nothing else reads it)

The outputs come from the reference's own code, called on CPU: `mojo_opset/core/operators/convolution.py`
MojoCausalConv1dUpdateState (its ``forward``, which also rewrites ``conv_state``) and `mojo_opset/core/functions/convolution.py`
MojoCausalConv1dFunction.forward.  Each case records the arguments, the output and the state after the call - tensors, scalars and
strings only; tests/test_short_conv_golden.py pins tests/short_conv_golden.py to them (states bit for bit, outputs inside the
stated bound: a CPU ``conv1d`` chooses its own summation order).

A function case with ``initial_state`` and ``output_final_state`` also records ``state_by_update_op``: per sequence, the state
the reference's UPDATE-STATE op leaves on the same concatenation (``conv_state = initial_state``, ``hidden_states = x_seq``).  It is
what `MojoCausalConv1d` returns here; the reference's function drops the initial state when a sequence is shorter than ``W - 1``.
(A sequence of length 0 leaves the state as it was: the update op's own ``conv1d`` refuses an input shorter than its kernel.)

The three reference test shapes are recorded once each, in different dtypes; everything else is 8 channels wide, so the file
stays under 256 KiB.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
NAMES = {BF16: "bf16", F16: "fp16", F32: "fp32"}
PACKED = [1, 2, 3, 17, 0, 40]


def tensors(g, dtype, *shapes):
    return [torch.randn(*s, generator=g).to(dtype) for s in shapes]


def coded(g, dtype, shape):
    """An input of a large case: multiples of 1/64 in [-2, 2), exact in every dtype, stored as int8 codes (half the bytes of a
    16-bit tensor); `short_conv_golden.case_args` rebuilds it."""
    codes = torch.randint(-128, 128, shape, generator=g, dtype=torch.int8)
    return codes, (codes.float() / 64).to(dtype)


def update_cases(g):
    """(label, B, T, D, W, S, dtype, bias, activation)"""
    out = [("ref-2x64x128-w3", 2, 64, 128, 3, 3, BF16, True, "silu"), ("ref-1x32x32-w4", 1, 32, 32, 4, 4, F32, True, "silu")]
    small = [(2, 1, 1), (2, 2, 5), (3, 2, 1), (3, 3, 2), (3, 3, 3), (4, 3, 1), (4, 4, 4), (4, 4, 1), (4, 7, 3), (4, 7, 7), (4, 7, 9)]
    acts = [None, "silu", "swish"]
    n = 0
    for dtype in (BF16, F16, F32):
        for width, state, seq in (small if dtype == BF16 else small[0:1] + small[3:4] + small[5:6] + small[8:9] + small[10:11]):
            out.append((f"w{width}-s{state}-t{seq}-{NAMES[dtype]}", 2, seq, 8, width, state, dtype, n % 2 == 0, acts[n % 3]))
            n += 1
    return out


def main(reference_root):
    sys.path.insert(0, reference_root)
    from mojo_opset.core.functions.convolution import MojoCausalConv1dFunction
    from mojo_opset.core.operators import convolution as ref_ops

    update_cls = ref_ops.MojoCausalConv1dUpdateState
    update = update_cls.forward                                     # the reference's own body, unbound: no backend dispatch

    def run_update(hidden, state, weight, bias, activation):
        state = state.clone()
        with torch.no_grad():
            out = update(None, hidden, state, weight, bias, activation)
        return out, state

    g = torch.Generator().manual_seed(2042)
    cases = []
    for label, batch, seq, dim, width, state_len, dtype, with_bias, act in update_cases(g):
        hidden, state, weight = tensors(g, dtype, (batch, dim, seq), (batch, dim, state_len), (dim, width))
        codes = None
        if hidden.numel() > 4096:
            codes, hidden = coded(g, dtype, hidden.shape)
        bias = tensors(g, dtype, (dim,))[0] if with_bias else None
        out, after = run_update(hidden, state, weight, bias, act)
        cases.append({"op": "MojoCausalConv1dUpdateState", "label": label, "kwargs": {}, "out": out, "state_after": after,
                      "args": (hidden if codes is None else None, state, weight, bias, act), "arg0_codes": codes, "arg0_dtype": NAMES[dtype]})

    def function_case(label, x, weight, **kw):
        # the reference's function raises on a sequence of length 0 (its conv1d refuses an empty input): such a case is recorded
        # from a call WITHOUT the empty sequences - the tokens and the other sequences' states are the same - and the rows of the
        # recorded final state are listed in ``final_state_rows``
        ref_kw, rows = {k: v for k, v in kw.items() if k != "codes"}, None
        if kw.get("cu_seqlens") is not None:
            cu = kw["cu_seqlens"]
            rows = [n for n in range(cu.numel() - 1) if int(cu[n + 1]) > int(cu[n])]
            ref_kw["cu_seqlens"] = torch.cat([cu[:1], cu[1:][rows]])
            if kw.get("initial_state") is not None:
                ref_kw["initial_state"] = kw["initial_state"][rows]
        with torch.no_grad():
            out, final = MojoCausalConv1dFunction.forward(
                type("Ctx", (), {"save_for_backward": lambda self, *a: None})(), x, weight, ref_kw.get("bias"), ref_kw.get("residual"),
                ref_kw.get("initial_state"), ref_kw.get("output_final_state", False), ref_kw.get("activation"), ref_kw.get("cu_seqlens"))
        codes = kw.pop("codes", None)
        case = {"op": "MojoCausalConv1d", "label": label, "args": (x if codes is None else None, weight), "kwargs": kw, "out": out,
                "final_state": final, "arg0_codes": codes, "arg0_dtype": NAMES[x.dtype]}
        if rows is not None:
            case["final_state_rows"] = rows
        init = kw.get("initial_state")
        if init is not None and kw.get("output_final_state"):
            cu = kw.get("cu_seqlens")
            spans = [(b, 0, x.shape[1]) for b in range(x.shape[0])] if cu is None else \
                [(0, int(cu[n]), int(cu[n + 1])) for n in range(cu.numel() - 1)]
            rows = []
            for n, (row, bos, eos) in enumerate(spans):
                if eos == bos:
                    rows.append(init[n].clone())
                else:
                    rows.append(run_update(x[row, bos:eos].transpose(0, 1).unsqueeze(0).contiguous(), init[n:n + 1], weight, None, None)[1][0])
            case["state_by_update_op"] = torch.stack(rows)
        cases.append(case)

    weight, bias = tensors(g, F16, (128, 4), (128,))
    codes, x = coded(g, F16, (2, 128, 128))
    function_case("ref-2x128x128-w4", x, weight, bias=bias, activation="silu", output_final_state=True, codes=codes)
    cu = torch.tensor([0] + torch.tensor(PACKED).cumsum(0).tolist())
    n = 0
    for dtype in (BF16, F16, F32):
        for width in (2, 3, 4):
            name = f"w{width}-{NAMES[dtype]}"
            x, res, weight, bias, init = tensors(g, dtype, (2, 9, 8), (2, 9, 8), (8, width), (8,), (2, 8, width - 1))
            act = [None, "silu", "swish"][n % 3]
            function_case(f"residual-{name}", x, weight, bias=bias if n % 2 else None, residual=res, activation=act,
                          output_final_state=True)
            function_case(f"state-{name}", x, weight, bias=bias, initial_state=init, output_final_state=True, activation=act)
            # T = 1: shorter than W - 1 for W = 3 and 4 (the deviation), equal to it for W = 2
            function_case(f"state-t1-{name}", x[:, :1].contiguous(), weight, initial_state=init, output_final_state=True)
            if width == 4:
                function_case(f"no-state-t1-{name}", x[:, :1].contiguous(), weight, output_final_state=True)
            if n % 3 != (0, 1, 2)[(F32, F16, BF16).index(dtype)]:    # the packed batch once per dtype and once per width
                n += 1
                continue
            packed, pres, pinit = tensors(g, dtype, (1, sum(PACKED), 8), (1, sum(PACKED), 8), (len(PACKED), 8, width - 1))
            function_case(f"packed-{name}", packed, weight, bias=bias, output_final_state=True, activation=act,
                          cu_seqlens=cu.to(torch.int32 if n % 2 else torch.int64))
            function_case(f"packed-state-{name}", packed, weight, bias=bias, residual=pres, initial_state=pinit,
                          output_final_state=True, activation=act, cu_seqlens=cu.to(torch.int64 if n % 2 else torch.int32))
            n += 1
    path = os.path.join(ROOT, "tests", "golden", "short_conv.pt")
    torch.save({"cases": cases}, path, _use_new_zipfile_serialization=False)   # (the zip form pads every tensor to 64 bytes)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MOJO_REFERENCE_ROOT")
    if not root:
        sys.exit(__doc__)
    main(root)
