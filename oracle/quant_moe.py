"""Torch goldens of the W8A8 MoE ops (`MojoMoEDynamicQuant`, `MojoQuantExperts`, `MojoQuantMoE`).

Importing this module registers ``TorchMoEDynamicQuant`` / ``TorchQuantExperts`` / ``TorchQuantMoE`` as the ``torch``
backends of the three API classes.

Semantics and rounding points restate `mojo_opset/core/operators/quantize.py:208-244` (the quantiser) and
`mojo_opset/core/operators/moe.py:566-664` (the experts):

* quantiser: ``y = x.float() * inv_smooth_scale[expert of the row]``; ``scale = amax|y|.clamp(1e-12) / 127``, ``1.0`` where
  that is below ``1e-6``; ``q = round(y / scale)`` clamped to [-128, 127]; the counts are validated on the host (non-negative,
  summing to the row count);
* quant-linear: ``acc.float() * weight_scale * input_scale`` in THAT order — the bf16 weight scale is promoted to fp32 by
  the product, the result is rounded once, to the activation dtype.  With group scales each K group's partial sum is scaled
  by its own weight scale and by the input scale, and the groups are summed in fp32.  int4 weights are two signed nibbles
  per byte along the OUTPUT dimension, low nibble = even row;
* between the projections: fc1's rounded output back to fp32, ``silu(gate) * up`` with the gate the FIRST half, fp32 into the
  second quantiser; fc2's output in the activation dtype.

``acc`` in the reference is an ``[m, N, K]`` int32 product summed in fp32 along K.  ``exact_int=True`` takes it from an exact
integer matrix product instead (fp64 matmul of the int8 values): the same bits whenever ``sum_k |x_k| |w_k| < 2**24`` for
every output — then every partial fp32 sum of the reference is an integer below 2**24, exact in any order.  The form asserts
that bound on its inputs (``dot_bound``).  `tests/golden/quant_moe.pt` pins both forms bit for bit.

``TorchQuantMoE`` chains the ``torch`` backends of gating, dispatch and combine (`oracle/torch_golden.py`, which the package
imports with this module) around
``TorchQuantExperts`` through `MojoMoE.compose_forward`.
"""
import torch
import torch.nn.functional as F

from mojo_opset_amd.core.operators import moe as _moe
from mojo_opset_amd.core.operators import quantize as _quant

_CPU = ["rocm", "cpu"]

EXACT_BOUND = 2 ** 24


def unpack_int4(weight: torch.Tensor) -> torch.Tensor:
    """int8 ``[N / 2, K]`` holding two signed nibbles per byte -> int8 ``[N, K]``: row 2i is the low nibble of packed row i,
    row 2i + 1 the high nibble (moe.py:566-573)."""
    assert weight.ndim == 2
    out = torch.empty(weight.shape[0] * 2, weight.shape[1], dtype=torch.int8, device=weight.device)
    out[0::2] = weight & 0x0F
    out[1::2] = (weight >> 4) & 0x0F
    return torch.where(out >= 8, out - 16, out)


def pack_int4(weight: torch.Tensor) -> torch.Tensor:
    """The inverse of `unpack_int4` for values in [-8, 7]: ``[..., N, K]`` -> ``[..., N / 2, K]``."""
    u = weight.to(torch.uint8) & 0x0F
    return (u[..., 0::2, :] | (u[..., 1::2, :] << 4)).to(torch.int8)


def dot_bound(x8: torch.Tensor, w8: torch.Tensor) -> int:
    """max over outputs of ``sum_k |x_k| |w_k|`` for ``x8 [m, K]`` against ``w8 [N, K]`` (exact, fp64)."""
    if x8.shape[0] == 0:
        return 0
    return int((x8.double().abs() @ w8.double().abs().T).max().item())


def int_dot(x8: torch.Tensor, w8: torch.Tensor, exact_int: bool) -> torch.Tensor:
    """fp32 ``[m, N]``: the reference's ``(x.int()[:, None, :] * w.int()[None, :, :]).float().sum(-1)``, or the exact integer
    product where the bound makes them the same bits."""
    if exact_int:
        bound = dot_bound(x8, w8)
        assert bound < EXACT_BOUND, f"exact_int: sum |x||w| reaches {bound} >= 2**24, the reference's fp32 sum is not exact"
        return (x8.double() @ w8.double().T).float()
    return torch.mul(x8.int().unsqueeze(-2), w8.int().unsqueeze(-3)).float().sum(dim=-1)


def quant_linear(x8, x_scale, weight, weight_scale, out_dtype, weight_dtype=torch.int8, group_size=-1, exact_int=False):
    """One expert's projection (moe.py:575-600)."""
    if weight_dtype == "int4":
        weight = unpack_int4(weight)
    assert x_scale.ndim == 2 and x_scale.shape[1] == 1
    if group_size > 0:
        parts = [int_dot(xg, wg, exact_int) for xg, wg in zip(torch.split(x8, group_size, dim=-1), torch.split(weight, group_size, dim=-1))]
        out = (torch.stack(parts, dim=-1) * weight_scale * x_scale.unsqueeze(-1)).sum(-1)
    else:
        out = int_dot(x8, weight, exact_int) * weight_scale * x_scale
    return out.to(out_dtype)


def moe_dynamic_quant(x, inv_smooth_scale, token_count, q_max=127, q_min=-128):
    """The quantiser's arithmetic without its host-side validation (quantize.py:237-244)."""
    y = x.float() * inv_smooth_scale.float().repeat_interleave(token_count, dim=0)
    scale = y.abs().amax(dim=-1, keepdim=True).clamp(min=1e-12) / q_max
    scale = torch.where(scale < 1e-6, 1.0, scale)
    return torch.clamp(torch.round(y / scale), q_min, q_max).to(torch.int8), scale


class TorchMoEDynamicQuant(_quant.MojoMoEDynamicQuant):
    supported_platforms_list = _CPU

    def forward(self, input: torch.Tensor, token_count: torch.Tensor):
        self.check_call_contract(input, token_count)
        if torch.any(token_count < 0):
            raise ValueError("token_count must be non-negative.")
        rows = input.reshape(-1, input.shape[-1]).size(0)
        if int(token_count.sum().item()) != rows:
            raise ValueError(f"token_count sum must equal flattened row count {rows}, got {token_count.sum().item()}.")
        return moe_dynamic_quant(input, self.inv_smooth_scale, token_count, self.q_max, self.q_min)


class TorchQuantExperts(_moe.MojoQuantExperts):
    supported_platforms_list = _CPU
    exact_int = False          # set on an instance: `acc` from the exact integer product (module docstring)

    def stages(self, sorted_hidden_states: torch.Tensor, tokens_per_expert: torch.Tensor):
        """Every intermediate of the forward, for the tests that feed a later stage the golden's own input:
        ``x8, x_scale, fc1 (activation dtype), activated (fp32), smoothed (fp32, times the second smooth scale), y8, y_scale, out``."""
        dtype = sorted_hidden_states.dtype
        x8, x_scale = self.up_proj_quantize(sorted_hidden_states, tokens_per_expert)
        counts = tokens_per_expert.tolist()
        fc1 = []
        for e, (xq, xs) in enumerate(zip(torch.split(x8, counts, dim=0), torch.split(x_scale, counts, dim=0))):
            if xq.shape[0] == 0:
                fc1.append(torch.empty(0, 2 * self.intermediate_size, dtype=dtype))
                continue
            fc1.append(quant_linear(xq, xs, self.up_proj_weight[e], self.up_proj_weight_scale[e], dtype, self.up_weight_dtype,
                                    self.up_quant_group_size, self.exact_int))
        fc1 = torch.cat(fc1, dim=0)
        gate, up = fc1.float().chunk(2, dim=-1)
        activated = F.silu(gate) * up
        y8, y_scale = self.down_proj_quantize(activated, tokens_per_expert)
        smoothed = activated * self.down_proj_quantize.inv_smooth_scale.float().repeat_interleave(tokens_per_expert, dim=0)
        out = []
        for e, (yq, ys) in enumerate(zip(torch.split(y8, counts, dim=0), torch.split(y_scale, counts, dim=0))):
            if yq.shape[0] == 0:
                out.append(torch.empty(0, self.hidden_size, dtype=dtype))
                continue
            out.append(quant_linear(yq, ys, self.down_proj_weight[e], self.down_proj_weight_scale[e], dtype, self.down_weight_dtype,
                                    self.down_quant_group_size, self.exact_int))
        return x8, x_scale, fc1, activated, smoothed, y8, y_scale, torch.cat(out, dim=0)

    def forward(self, sorted_hidden_states: torch.Tensor, tokens_per_expert: torch.Tensor):
        return self.stages(sorted_hidden_states, tokens_per_expert)[-1]


class TorchQuantMoE(_moe.MojoQuantMoE):
    supported_platforms_list = _CPU

    def forward(self, hidden_states: torch.Tensor) -> torch.Tensor:
        return _moe.MojoMoE.compose_forward(self, hidden_states)
