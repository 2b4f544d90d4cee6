"""Torch goldens of the short-convolution ops (`SHORT_CONV_OPS`): `MojoCausalConv1dUpdateState` and `MojoCausalConv1d`.

Importing this module registers a ``Torch<Op>`` class as the ``torch`` backend of each API class.

The goldens state the ONE arithmetic every backend of these ops follows, in elementwise torch calls only (a CPU ``conv1d``
chooses its own summation order and, in 16 bits, its own intermediate roundings, so it cannot be a bit-level golden):

    acc = bias as fp32 (or +0.0)
    acc = acc + w[k] * x[oldest + k]        k = 0 .. W - 1, the product and the sum two fp32 roundings (two torch calls)
    y   = silu(acc) when asked              evaluated in fp64 on the fp32 accumulator and rounded to fp32
    out = storage(y)                        one rounding
    out = storage(out + residual)           `MojoCausalConv1d` only: the residual meets the ROUNDED value, as in the reference

Beside the result, `conv_detail` reports the fp32 pre-activation, an fp64 evaluation of the same sum and the magnitude
``sum_k |w[k] * x[..]| + |bias|`` per output, which the bounds of tests/test_short_conv_golden.py are stated in.

The states are copies: the new state of the update op is the last ``S`` columns of ``cat(conv_state, hidden_states)``, and the
final state of `MojoCausalConv1d` is the last ``W - 1`` columns of ``cat(initial_state or zeros, x_seq)`` - for a sequence shorter
than ``W - 1`` under an ``initial_state`` a deliberate deviation from the reference, which drops the initial state there
(`reference_final_state` restates its rule)."""
import torch

from mojo_opset_amd.core.operators import convolution as _conv

_CPU = ["rocm", "cpu"]
_DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def case_args(case):
    """Clones of the positional arguments of a recorded case (tests/make_short_conv_golden.py); the first argument of a large case
    is stored as int8 codes, multiples of 1/64."""
    args = [a.clone() if isinstance(a, torch.Tensor) else a for a in case["args"]]
    if case.get("arg0_codes") is not None:
        args[0] = (case["arg0_codes"].float() / 64).to(_DTYPES[case["arg0_dtype"]])
    return args


def silu_of_fp32(pre):
    """SiLU of an fp32 tensor, evaluated in fp64 and rounded to fp32."""
    wide = pre.double()
    return (wide * torch.sigmoid(wide)).float()


def conv_detail(cat, weight, bias, outputs, silu):
    """``cat [..., D, L]`` (state or zeros, then the inputs, storage dtype), ``outputs`` = T: the last T positions of ``cat`` are
    convolved, each with the ``W - 1`` columns before it.  Returns a dict: ``pre`` (fp32 accumulator), ``y`` (fp32 after the
    activation), ``out`` (storage), ``exact`` (fp64 evaluation of the sum, before the activation), ``mag`` (fp64)."""
    width = weight.shape[1]
    first = cat.shape[-1] - outputs - (width - 1)
    assert first >= 0
    x32, w32 = cat.float(), weight.float()
    pre = (bias.float() if bias is not None else torch.zeros(weight.shape[0])).unsqueeze(-1).expand(*cat.shape[:-1], outputs).clone()
    exact = pre.double()
    mag = exact.abs()
    for k in range(width):
        window = x32[..., first + k:first + k + outputs]
        tap = w32[:, k].unsqueeze(-1)
        product = tap * window                              # one fp32 rounding
        pre = pre + product                                 # another
        wide = tap.double() * window.double()
        exact = exact + wide
        mag = mag + wide.abs()
    y = silu_of_fp32(pre) if silu else pre
    return {"pre": pre, "y": y, "out": y.to(cat.dtype), "exact": exact, "mag": mag}


def update_state_detail(hidden_states, conv_state, weight, bias=None, activation=None):
    """`conv_detail` of the update op plus ``state``: the new ``conv_state`` (the argument is not written)."""
    what = "TorchCausalConv1dUpdateState"
    silu = _conv.use_silu(what, activation)
    _conv.check_update_state_call(what, hidden_states, conv_state, weight, bias)
    cat = torch.cat([conv_state, hidden_states], dim=-1)
    detail = conv_detail(cat, weight, bias, hidden_states.shape[-1], silu)
    detail["state"] = cat[..., cat.shape[-1] - conv_state.shape[-1]:].clone()
    return detail


def conv1d_detail(x, weight, bias=None, residual=None, initial_state=None, activation=None, cu_seqlens=None):
    """`conv_detail` of `MojoCausalConv1d` in ``[B, T, D]`` layout (``out`` includes the residual; ``conv_out`` is the value
    before it) plus ``final_state [B or N, D, W - 1]``.  A token outside every sequence of ``cu_seqlens`` gets zeros."""
    what = "TorchCausalConv1d"
    silu = _conv.use_silu(what, activation)
    width, sequences = _conv.check_conv1d_call(what, x, weight, bias, residual, initial_state, cu_seqlens)
    dim = x.shape[2]
    if cu_seqlens is None:
        bounds = [(b, 0, x.shape[1]) for b in range(x.shape[0])]
    else:
        total = x.shape[1]
        cu = [min(max(int(v), 0), total) for v in cu_seqlens.tolist()]
        bounds = [(0, cu[n], max(cu[n], cu[n + 1])) for n in range(sequences)]
    keys = ("pre", "y", "exact", "mag")
    full = {k: torch.zeros(x.shape, dtype=torch.float64 if k in ("exact", "mag") else torch.float32) for k in keys}
    conv_out = torch.zeros_like(x)
    final = torch.zeros(sequences, dim, width - 1, dtype=x.dtype)
    for n, (row, bos, eos) in enumerate(bounds):
        state = initial_state[n] if initial_state is not None else torch.zeros(dim, width - 1, dtype=x.dtype)
        cat = torch.cat([state, x[row, bos:eos].transpose(0, 1)], dim=-1)
        final[n] = cat[:, cat.shape[-1] - (width - 1):]
        if eos > bos:
            detail = conv_detail(cat, weight, bias, eos - bos, silu)
            for k in keys:
                full[k][row, bos:eos] = detail[k].transpose(0, 1)
            conv_out[row, bos:eos] = detail["out"].transpose(0, 1)
    full["conv_out"] = conv_out
    full["out"] = conv_out if residual is None else (conv_out.float() + residual.float()).to(x.dtype)
    full["final_state"] = final
    return full


def reference_final_state(x_seq, width):
    """The reference's rule for ONE sequence ``[T, D]``: the last ``W - 1`` inputs, zero-padded in front; the initial state never
    enters.  Agrees with the golden whenever ``T >= W - 1`` or no initial state is given."""
    cols = x_seq.transpose(0, 1)
    short = width - 1 - cols.shape[-1]
    return torch.nn.functional.pad(cols, (short, 0)) if short > 0 else cols[:, cols.shape[-1] - (width - 1):]


class TorchCausalConv1dUpdateState(_conv.MojoCausalConv1dUpdateState):
    supported_platforms_list = _CPU

    def forward(self, hidden_states, conv_state, weight, bias=None, activation=None):
        detail = update_state_detail(hidden_states, conv_state, weight, bias, activation)
        conv_state.copy_(detail["state"])
        return detail["out"]


class TorchCausalConv1d(_conv.MojoCausalConv1d):
    supported_platforms_list = _CPU

    def forward(self, x, weight, bias=None, residual=None, initial_state=None, output_final_state=False, activation=None,
                cu_seqlens=None):
        detail = conv1d_detail(x, weight, bias, residual, initial_state, activation, cu_seqlens)
        return detail["out"], (detail["final_state"] if output_final_state else None)


GOLDENS = {"MojoCausalConv1dUpdateState": TorchCausalConv1dUpdateState, "MojoCausalConv1d": TorchCausalConv1d}
