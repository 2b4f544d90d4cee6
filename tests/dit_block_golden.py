"""Torch goldens of the DiT block ops (`DIT_BLOCK_OPS`): LayerNorm, residual-add LayerNorm, GELU, SiLU, grid RoPE.

Importing this module registers a ``Torch<Op>`` class as the ``torch`` backend of each API class.

The reference's classes (`mojo_opset/core/operators/normalization.py:19-68`, `:365-432`, `activation.py:6-35`,
`experimental/operators/position_embedding.py:80-118`) are thin calls into torch, so the goldens are the same library calls on
the same arguments: the only way to the same bits on the CPU.  `tests/golden/dit_block.pt` pins every class here bit for bit
(tests/make_dit_block_golden.py records it from the reference).

torch's CPU kernels for fp16 GELU / SiLU are not the same on every host (one evaluates in fp32 and rounds, another takes a
native half-precision route: gelu(+inf) is NaN on the first and +inf on the second).  The recording is the first kind, so the
goldens spell that out for fp16 -- convert, evaluate in fp32, round once -- which is bit for bit what the recording host's
kernel does and does not depend on the host the tests run on.

The ``*_fp64`` functions are the formulas themselves in double precision: what the GPU tests count storage ulps against.
"""
import math

import torch
import torch.nn.functional as F

from mojo_opset_amd.core.operators import activation as _act
from mojo_opset_amd.core.operators import normalization as _norm
from mojo_opset_amd.core.operators import position_embedding as _pos

_CPU = ["rocm", "cpu"]


class TorchLayerNorm(_norm.MojoLayerNorm):
    supported_platforms_list = _CPU

    def forward(self, hidden_state):
        return F.layer_norm(hidden_state, (hidden_state.shape[-1],), self.weight, self.bias, self.variance_epsilon)


class TorchResidualAddLayerNorm(_norm.MojoResidualAddLayerNorm):
    supported_platforms_list = _CPU

    def forward(self, hidden_state, residual):
        summed = hidden_state + residual                       # rounded to the input dtype: the norm sees the rounded sum
        normed = F.layer_norm(summed, (summed.shape[-1],), self.weight, self.bias, self.variance_epsilon)
        return (normed, summed) if self.norm_pos == "pre" else (normed, normed)


class TorchGelu(_act.MojoGelu):
    supported_platforms_list = _CPU

    def forward(self, x):
        if x.dtype == torch.float16:                           # (module docstring: host-independent form of the fp16 kernel)
            return F.gelu(x.float()).to(x.dtype)
        return F.gelu(x)                                       # approximate="none": the erf form


class TorchSilu(_act.MojoSilu):
    supported_platforms_list = _CPU

    def forward(self, x):
        if x.dtype == torch.float16:
            return F.silu(x.float()).to(x.dtype)
        return F.silu(x)


class TorchGridRoPE(_pos.MojoGridRoPE):
    supported_platforms_list = _CPU

    def forward(self, x, grid_sizes, freqs_list):
        self.check_shape_contract(x, grid_sizes, freqs_list)
        out = x.clone()                                        # the padding tokens: unchanged
        for i, (f, h, w) in enumerate(grid_sizes.tolist()):
            cells = f * h * w
            pairs = x[i, :cells].float().unflatten(-1, (-1, 2)).contiguous()
            turned = torch.view_as_complex(pairs) * freqs_list[i]            # [cells, N, D/2] x [cells, 1, D/2], complex64
            out[i, :cells] = torch.view_as_real(turned).flatten(-2).to(x.dtype)
        return out


GOLDENS = {"MojoLayerNorm": TorchLayerNorm, "MojoResidualAddLayerNorm": TorchResidualAddLayerNorm, "MojoGelu": TorchGelu,
           "MojoSilu": TorchSilu, "MojoGridRoPE": TorchGridRoPE}


def layernorm_fp64(x, weight=None, bias=None, eps=1e-5):
    """mean, biased variance as the mean of squared deviations, (x - mean) / sqrt(var + eps) * w + b, all in fp64."""
    x = x.double()
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + eps)
    if weight is not None:
        y = y * weight.double() + bias.double()
    return y


def gelu_fp64(x):
    """x * Phi(x) with Phi through erfc, which fp64 evaluates without cancellation down to where the product underflows."""
    x = x.double()
    return x * 0.5 * torch.special.erfc(-x * math.sqrt(0.5))


def silu_fp64(x):
    """x * sigmoid(x); for x < 0 as x * e^x / (1 + e^x), which does not overflow."""
    x = x.double()
    e = torch.exp(-x.abs())
    return torch.where(x >= 0, x / (1 + e), x * (e / (1 + e)))


def grid_rope_fp64(x, grid_sizes, freqs_list):
    out = x.double().clone()
    for i, (f, h, w) in enumerate(grid_sizes.tolist()):
        cells = f * h * w
        z = torch.view_as_complex(x[i, :cells].double().unflatten(-1, (-1, 2)).contiguous()) * freqs_list[i].to(torch.complex128)
        out[i, :cells] = torch.view_as_real(z).flatten(-2)
    return out


def ulp_distance(got, want_fp64):
    """Distance in units of the last place of ``got``'s dtype between ``got`` and ``want_fp64`` rounded once to that dtype
    (int64, same shape).  Both finite; the count is over the ordered bit patterns, so it is exact across exponent steps and
    through the subnormals, and +0 / -0 are zero apart."""
    want = want_fp64.to(got.dtype)
    bits = {torch.float32: (torch.int32, 31), torch.float16: (torch.int16, 15), torch.bfloat16: (torch.int16, 15)}[got.dtype]

    def ordered(t):
        raw = t.contiguous().view(bits[0]).to(torch.int64)
        mag = raw & ((1 << bits[1]) - 1)
        return torch.where(raw < 0, -mag, mag)

    return (ordered(got) - ordered(want)).abs()
