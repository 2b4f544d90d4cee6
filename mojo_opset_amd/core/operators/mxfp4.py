"""API classes of the MXFP4 ops (`MXFP4_OPS`): the OCP microscaling fp4 quantiser and the block-scaled a4w4 product.  The
reference has no class for either.

The format (the contract of both ops).  A row of ``K`` elements, ``K % 32 == 0``, is stored as

* ``K / 2`` bytes of data: element ``2j`` in bits 0-3 of byte ``j``, element ``2j + 1`` in bits 4-7;
* ``K / 32`` scale bytes, one per block of 32 consecutive elements.

A nibble is a sign bit and an E2M1 code: the magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6.  A scale byte ``e`` (E8M0) means
``2 ** (e - 127)``; ``0xFF`` is the format's NaN and outside the contract of the product.  ``uint8`` is the canonical storage.

Quantising one block, every step exact::

    amax = max |x|
    e    = clamp(floor(log2(amax)) - 2, -127, 127)        # scale byte e + 127; amax == 0: byte 0
    q    = round_to_grid(x * 2 ** -e)                      # nearest, ties to the even code; saturate at +-6; keep the sign, also of 0

(the ties: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4).  A block that holds Inf or NaN gets the
scale byte ``0xFF`` and zero nibbles.

``forward`` of the two classes is the golden: the quantiser by these rules in fp64, the product as
``dequantize(input) @ dequantize(weight).T`` in fp32, rounded once."""
from typing import Tuple

import torch

from ..operator import MojoOperator

BLOCK = 32
E2M1_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
SCALE_NAN = 0xFF
OUTPUT_DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def mxfp4_quantize(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``x [M, K]`` (any float dtype, ``K % 32 == 0``) -> ``(data uint8 [M, K/2], scale uint8 [M, K/32])`` by the rules above."""
    if x.dim() != 2 or x.shape[1] % BLOCK != 0 or x.shape[1] == 0:
        raise ValueError(f"mxfp4_quantize: x [M, K] with K a positive multiple of {BLOCK} expected, got {tuple(x.shape)}")
    m, k = x.shape
    xb = x.detach().to(torch.float64).reshape(m, k // BLOCK, BLOCK)
    finite = torch.isfinite(xb).all(dim=-1)
    amax = torch.where(finite, xb.abs().amax(dim=-1), torch.ones((), dtype=torch.float64, device=x.device))
    _, exponent = torch.frexp(amax)                               # amax = mantissa * 2 ** exponent, mantissa in [0.5, 1)
    e = torch.where(amax > 0, (exponent - 3).clamp(-127, 127), torch.full_like(exponent, -127))
    a = torch.ldexp(xb.abs(), -e.unsqueeze(-1))                   # exact: a power of two within fp64's range
    code = ((a > 0.25).to(torch.uint8) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) + (a >= 3.5) + (a > 5.0)).to(torch.uint8)
    nibble = code | (torch.signbit(xb).to(torch.uint8) << 3)
    nibble = torch.where(finite.unsqueeze(-1), nibble, torch.zeros_like(nibble)).reshape(m, k)
    data = nibble[:, 0::2] | (nibble[:, 1::2] << 4)
    scale = torch.where(finite, (e + 127).to(torch.uint8), torch.full_like(e, SCALE_NAN, dtype=torch.uint8))
    return data.contiguous(), scale.contiguous()


def mxfp4_dequantize(data: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """The inverse: ``(data uint8 [M, K/2], scale uint8 [M, K/32])`` -> fp32 ``[M, K]`` (a scale byte 0xFF gives NaN).  Exact but
    for products below fp32's range (a scale byte under 3 with the smallest magnitudes)."""
    data, scale = as_bytes(data), as_bytes(scale)
    if data.dim() != 2 or scale.dim() != 2 or data.shape[0] != scale.shape[0] or data.shape[1] != scale.shape[1] * (BLOCK // 2):
        raise ValueError(f"mxfp4_dequantize: data [M, K/2] and scale [M, K/32] expected, got {tuple(data.shape)} and "
                         f"{tuple(scale.shape)}")
    grid = torch.tensor(E2M1_GRID + tuple(-v for v in E2M1_GRID), dtype=torch.float32, device=data.device)
    nibble = torch.stack((data & 0xF, data >> 4), dim=-1).reshape(data.shape[0], -1)
    value = grid[nibble.long()].reshape(data.shape[0], -1, BLOCK)
    factor = torch.ldexp(torch.ones((), dtype=torch.float64, device=data.device), scale.to(torch.int32) - 127)
    factor = torch.where(scale == SCALE_NAN, torch.full_like(factor, float("nan")), factor)
    return (value.double() * factor.unsqueeze(-1)).to(torch.float32).reshape(data.shape[0], -1)


def as_bytes(t: torch.Tensor) -> torch.Tensor:
    """uint8 as it is; ``float4_e2m1fn_x2`` / ``float8_e8m0fnu`` (where this torch has them) by view."""
    return t if t.dtype == torch.uint8 else t.view(torch.uint8)


def check_quant_call(what: str, x: torch.Tensor) -> Tuple[int, int]:
    if x.dim() != 2 or x.shape[1] % BLOCK != 0 or x.shape[1] == 0:
        raise ValueError(f"{what}: x [M, K] with K a positive multiple of {BLOCK} expected, got {tuple(x.shape)}")
    if x.dtype not in (torch.bfloat16, torch.float16):
        raise NotImplementedError(f"{what}: bf16 or fp16 input expected, got {x.dtype}")
    if x.stride(1) != 1 and x.shape[1] > 1:
        raise NotImplementedError(f"{what}: rows must be dense (rows by a stride), got strides {x.stride()}")
    return x.shape[0], x.shape[1]


class MojoMXFP4Quant(MojoOperator):
    """forward(x bf16 / fp16 [M, K], rows by a stride) -> (data uint8 [M, K/2], scale uint8 [M, K/32])."""

    def forward(self, x: torch.Tensor):
        check_quant_call("MojoMXFP4Quant", x)
        return mxfp4_quantize(x)


class MojoMXFP4Gemm(MojoOperator):
    """forward(input [M, K/2], input_scale [M, K/32]) -> [M, N] in ``output_dtype`` (bf16, fp16 or fp32): the product of the
    dequantised operands with fp32 accumulation, rounded once.  Buffers: ``weight`` uint8 ``[N, K/2]`` and ``weight_scale`` uint8
    ``[N, K/32]`` (the K-contiguous layout only: blocks run along K)."""

    def __init__(self, in_features: int, out_features: int, output_dtype: torch.dtype = torch.bfloat16, **kwargs):
        super().__init__(**kwargs)
        if in_features <= 0 or in_features % BLOCK != 0:
            raise ValueError(f"MojoMXFP4Gemm: in_features must be a positive multiple of {BLOCK}, got {in_features}")
        if output_dtype not in OUTPUT_DTYPES:
            raise NotImplementedError(f"MojoMXFP4Gemm: output_dtype {output_dtype}; {OUTPUT_DTYPES} are supported")
        self.in_features = in_features
        self.out_features = out_features
        self.output_dtype = output_dtype
        factory = {**self.tensor_factory_kwargs, "dtype": torch.uint8}
        self.register_buffer("weight", torch.zeros((out_features, in_features // 2), **factory))
        self.register_buffer("weight_scale", torch.full((out_features, in_features // BLOCK), 127, **factory))

    def check_call_contract(self, input: torch.Tensor, input_scale: torch.Tensor) -> Tuple[int, int, int]:
        """Returns ``(M, K, N)``."""
        what, k, n = type(self).__name__, self.in_features, self.out_features
        if tuple(self.weight.shape) != (n, k // 2) or tuple(self.weight_scale.shape) != (n, k // BLOCK):
            raise ValueError(f"{what}: weight [{n}, {k // 2}] and weight_scale [{n}, {k // BLOCK}] expected, got "
                             f"{tuple(self.weight.shape)} and {tuple(self.weight_scale.shape)}")
        if input.dim() != 2 or input.shape[1] != k // 2 or tuple(input_scale.shape) != (input.shape[0], k // BLOCK):
            raise ValueError(f"{what}: input [M, {k // 2}] and input_scale [M, {k // BLOCK}] expected, got {tuple(input.shape)} "
                             f"and {tuple(input_scale.shape)}")
        return input.shape[0], k, n

    def extra_repr(self) -> str:
        return f"in_features={self.in_features}, out_features={self.out_features}, output_dtype={self.output_dtype}"

    def forward(self, input: torch.Tensor, input_scale: torch.Tensor) -> torch.Tensor:
        self.check_call_contract(input, input_scale)
        a = mxfp4_dequantize(input, input_scale)
        w = mxfp4_dequantize(self.weight, self.weight_scale)
        return (a @ w.T).to(self.output_dtype)
