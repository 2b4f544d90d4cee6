"""API classes of the MXFP4 ops (`MXFP4_OPS`): the OCP microscaling fp4 quantiser and the block-scaled a4w4 product, and of the
MXFP4 MoE experts (`MXFP4_MOE_OPS`): the grouped product, the SwiGLU re-quantiser between the two expert GEMMs and the experts
operator.  The reference has no class for any of them.

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

``forward`` of the classes is the golden: the quantiser by these rules in fp64, the product as
``dequantize(input) @ dequantize(weight).T`` in fp32, rounded once; the grouped classes are written with the same two functions."""
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


def swiglu_mxfp4_quantize(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``x [M, 2I]`` = ``[gate | up]`` -> ``mxfp4_quantize(silu(gate) * up)``, ``silu`` and the multiply in fp32."""
    inter = x.shape[1] // 2
    return mxfp4_quantize(torch.nn.functional.silu(x[:, :inter].float()) * x[:, inter:].float())


class MojoMXFP4GroupGemm(MojoOperator):
    """forward(input uint8 [M, K/2], input_scale uint8 [M, K/32], group_list int32 [G]): the a4w4 product over ragged row groups.

    ``group_list`` holds ROW COUNTS (as `MojoGroupGemm`): group ``g`` owns the next ``group_list[g]`` rows and multiplies them by
    ``weight[g]``.  Rows ``[sum(group_list), M)`` of every output are zeros (data bytes 0 and scale byte 0 in the fused form).
    Buffers: ``weight`` uint8 ``[G, N, K/2]`` and ``weight_scale`` uint8 ``[G, N, K/32]``.

    ``swiglu_quant=False``: returns ``[M, N]`` in ``output_dtype``, per group ``dequantize(a) @ dequantize(w[g]).T`` accumulated in
    fp32 and rounded once.  ``swiglu_quant=True`` (``N = 2I``, ``I % 32 == 0``, weight rows ``[gate | up]`` as in `MojoExperts`):
    returns ``(data uint8 [M, I/2], scale uint8 [M, I/32]) = mxfp4_quantize(silu(gate) * up)`` of the UNROUNDED fp32 products,
    ``silu`` and the multiply in fp32; ``output_dtype`` is ignored.

    Raises NotImplementedError for ``[G, K, N]`` weights (only the K-contiguous layout exists: blocks run along K) and for mixed
    fp8 x fp4 operands."""

    def __init__(self, num_groups: int, in_features: int, out_features: int, output_dtype: torch.dtype = torch.bfloat16,
                 swiglu_quant: bool = False, **kwargs):
        super().__init__(**kwargs)
        what = "MojoMXFP4GroupGemm"
        if num_groups <= 0 or in_features <= 0 or in_features % BLOCK != 0:
            raise ValueError(f"{what}: num_groups must be positive and in_features a positive multiple of {BLOCK}, got "
                             f"{num_groups} and {in_features}")
        if swiglu_quant and (out_features <= 0 or out_features % (2 * BLOCK) != 0):
            raise ValueError(f"{what}: swiglu_quant wants out_features = 2 I with I a multiple of {BLOCK}, got {out_features}")
        if output_dtype not in OUTPUT_DTYPES:
            raise NotImplementedError(f"{what}: output_dtype {output_dtype}; {OUTPUT_DTYPES} are supported")
        self.num_groups, self.in_features, self.out_features = num_groups, in_features, out_features
        self.output_dtype, self.swiglu_quant = output_dtype, swiglu_quant
        factory = {**self.tensor_factory_kwargs, "dtype": torch.uint8}
        self.register_buffer("weight", torch.zeros((num_groups, out_features, in_features // 2), **factory))
        self.register_buffer("weight_scale", torch.full((num_groups, out_features, in_features // BLOCK), 127, **factory))

    def check_call_contract(self, input: torch.Tensor, input_scale: torch.Tensor, group_list: torch.Tensor) -> Tuple[int, int, int]:
        """Returns ``(M, K, N)``."""
        return check_group_call(type(self).__name__, input, input_scale, self.weight, self.weight_scale, group_list,
                                self.in_features, self.out_features)

    def extra_repr(self) -> str:
        return (f"num_groups={self.num_groups}, in_features={self.in_features}, out_features={self.out_features}, "
                f"output_dtype={self.output_dtype}, swiglu_quant={self.swiglu_quant}")

    def forward(self, input: torch.Tensor, input_scale: torch.Tensor, group_list: torch.Tensor):
        self.check_call_contract(input, input_scale, group_list)
        fc = grouped_product(input, input_scale, self.weight, self.weight_scale, group_list)
        return swiglu_mxfp4_quantize(fc) if self.swiglu_quant else fc.to(self.output_dtype)


def check_group_call(what, input, input_scale, weight, weight_scale, group_list, k, n) -> Tuple[int, int, int]:
    groups = weight.shape[0] if weight.dim() == 3 else -1
    if tuple(weight.shape) != (groups, n, k // 2) or tuple(weight_scale.shape) != (groups, n, k // BLOCK):
        if weight.dim() == 3 and (tuple(weight.shape[1:]) in ((k, n // 2), (k // 2, n)) or tuple(weight_scale.shape[1:]) == (k // BLOCK, n)):
            raise NotImplementedError(f"{what}: [G, K, N] weights; only the K-contiguous [G, N, K/2] layout is supported")
        raise ValueError(f"{what}: weight [G, {n}, {k // 2}] and weight_scale [G, {n}, {k // BLOCK}] expected, got "
                         f"{tuple(weight.shape)} and {tuple(weight_scale.shape)}")
    if input.dim() != 2 or input.shape[1] != k // 2 or tuple(input_scale.shape) != (input.shape[0], k // BLOCK):
        raise ValueError(f"{what}: input [M, {k // 2}] and input_scale [M, {k // BLOCK}] expected, got {tuple(input.shape)} and "
                         f"{tuple(input_scale.shape)}")
    if group_list.dtype != torch.int32:
        raise NotImplementedError(f"{what}: group_list must be int32 row counts, got {group_list.dtype}")
    if tuple(group_list.shape) != (groups,):
        raise ValueError(f"{what}: group_list [{groups}] expected, got {tuple(group_list.shape)}")
    return input.shape[0], k, n


def grouped_product(input, input_scale, weight, weight_scale, group_list) -> torch.Tensor:
    """fp32 ``[M, N]``: per group the product of the dequantised operands; rows past ``sum(group_list)`` zeros."""
    a = mxfp4_dequantize(input, input_scale)
    out = torch.zeros((a.shape[0], weight.shape[1]), dtype=torch.float32, device=a.device)
    begin = 0
    for g, count in enumerate(group_list.clamp_min(0).tolist()):
        end = min(begin + count, a.shape[0])
        if end > begin:
            out[begin:end] = a[begin:end] @ mxfp4_dequantize(weight[g], weight_scale[g]).T
        begin = end
    return out


def check_swiglu_quant_call(what: str, x: torch.Tensor) -> Tuple[int, int]:
    """Returns ``(M, I)``."""
    if x.dim() != 2 or x.shape[1] == 0 or x.shape[1] % (2 * BLOCK) != 0:
        raise ValueError(f"{what}: x [M, 2I] with I a positive multiple of {BLOCK} expected, got {tuple(x.shape)}")
    if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise NotImplementedError(f"{what}: fp32, bf16 or fp16 input expected, got {x.dtype}")
    if x.stride(1) != 1:
        raise NotImplementedError(f"{what}: rows must be dense (rows by a stride), got strides {x.stride()}")
    return x.shape[0], x.shape[1] // 2


class MojoMXFP4SwiGLUQuant(MojoOperator):
    """forward(x [M, 2I] fp32 / bf16 / fp16, rows by a stride) -> (data uint8 [M, I/2], scale uint8 [M, I/32]) =
    ``mxfp4_quantize(silu(x[:, :I].float()) * x[:, I:].float())``: the stage between the two expert GEMMs as a stand-alone op.
    Raises NotImplementedError for gpt-oss's clamped / biased / interleaved SwiGLU (plain ``[gate | up]`` halves only)."""

    def forward(self, x: torch.Tensor):
        check_swiglu_quant_call("MojoMXFP4SwiGLUQuant", x)
        return swiglu_mxfp4_quantize(x)


class MojoMXFP4Experts(MojoOperator):
    """forward(sorted_hidden_states bf16 / fp16 [M, hidden], tokens_per_expert int32 [E]) -> [M, hidden]: MXFP4 experts, the
    arguments of `MojoExperts`.  The chain: `MojoMXFP4Quant` of the rows, fc1 as `MojoMXFP4GroupGemm(swiglu_quant=True)` against
    ``up_proj_weight`` (rows ``[gate | up]``), fc2 as `MojoMXFP4GroupGemm` against ``down_proj_weight`` with the input's dtype as
    ``output_dtype``.  Buffers (uint8): ``up_proj_weight [E, 2I, hidden/2]``, ``up_proj_weight_scale [E, 2I, hidden/32]``,
    ``down_proj_weight [E, hidden, I/2]``, ``down_proj_weight_scale [E, hidden, I/32]``.

    Raises NotImplementedError for any activation but ``"swiglu"`` (also gpt-oss's clamped / biased / interleaved form), for mixed
    fp8 x fp4 operands and for ``[G, K, N]`` weights.  There is no `MojoMXFP4MoE` layer class."""

    def __init__(self, num_experts: int, hidden_size: int, intermediate_size: int, activation: str = "swiglu", **kwargs):
        super().__init__(**kwargs)
        if activation != "swiglu":
            raise NotImplementedError(f"MojoMXFP4Experts: Activation {activation} is not supported.")
        if num_experts <= 0 or hidden_size <= 0 or hidden_size % BLOCK != 0 or intermediate_size <= 0 or intermediate_size % BLOCK != 0:
            raise ValueError(f"MojoMXFP4Experts: hidden_size and intermediate_size must be positive multiples of {BLOCK}, got "
                             f"{hidden_size} and {intermediate_size}")
        self.activation = activation
        self.num_experts, self.hidden_size, self.intermediate_size = num_experts, hidden_size, intermediate_size
        factory = {**self.tensor_factory_kwargs, "dtype": torch.uint8}
        e, h, i = num_experts, hidden_size, intermediate_size
        self.register_buffer("up_proj_weight", torch.zeros((e, 2 * i, h // 2), **factory))
        self.register_buffer("up_proj_weight_scale", torch.full((e, 2 * i, h // BLOCK), 127, **factory))
        self.register_buffer("down_proj_weight", torch.zeros((e, h, i // 2), **factory))
        self.register_buffer("down_proj_weight_scale", torch.full((e, h, i // BLOCK), 127, **factory))

    def check_call_contract(self, sorted_hidden_states: torch.Tensor, tokens_per_expert: torch.Tensor) -> None:
        what = type(self).__name__
        if sorted_hidden_states.dim() != 2 or sorted_hidden_states.shape[1] != self.hidden_size:
            raise ValueError(f"{what}: sorted_hidden_states [M, {self.hidden_size}] expected, got {tuple(sorted_hidden_states.shape)}")
        check_quant_call(what, sorted_hidden_states)

    def extra_repr(self) -> str:
        return f"num_experts={self.num_experts}, hidden_size={self.hidden_size}, intermediate_size={self.intermediate_size}"

    def forward(self, sorted_hidden_states: torch.Tensor, tokens_per_expert: torch.Tensor) -> torch.Tensor:
        self.check_call_contract(sorted_hidden_states, tokens_per_expert)
        h, i = self.hidden_size, self.intermediate_size
        a, sa = mxfp4_quantize(sorted_hidden_states)
        check_group_call("MojoMXFP4Experts fc1", a, sa, self.up_proj_weight, self.up_proj_weight_scale, tokens_per_expert, h, 2 * i)
        y, sy = swiglu_mxfp4_quantize(grouped_product(a, sa, self.up_proj_weight, self.up_proj_weight_scale, tokens_per_expert))
        check_group_call("MojoMXFP4Experts fc2", y, sy, self.down_proj_weight, self.down_proj_weight_scale, tokens_per_expert, i, h)
        out = grouped_product(y, sy, self.down_proj_weight, self.down_proj_weight_scale, tokens_per_expert)
        return out.to(sorted_hidden_states.dtype)
