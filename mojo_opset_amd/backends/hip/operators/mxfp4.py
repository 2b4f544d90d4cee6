"""HIP<Op> classes of the MXFP4 ops (`MXFP4_OPS`): `MojoMXFP4Quant` and `MojoMXFP4Gemm` on csrc/mxfp4_gemm.hip, and
of the MXFP4 MoE experts (`MXFP4_MOE_OPS`) on csrc/mxfp4_group_gemm.hip.
The quantiser is one streaming launch; the product runs on ``v_mfma_scale_f32_16x16x128_f8f6f4`` with fp4 operands and both
block scales applied by the instruction, in a tile form (``M > 32``) or a weight-streaming skinny form with a fixed-order
split-K merge (``M <= 32``), planned from the shapes alone.  Everything outside the envelope raises on the host, before any
device work."""
import torch

from ....core.operators.mxfp4 import (BLOCK, MojoMXFP4Experts, MojoMXFP4Gemm, MojoMXFP4GroupGemm, MojoMXFP4Quant,
                                      MojoMXFP4SwiGLUQuant, as_bytes, check_group_call, check_quant_call, check_swiglu_quant_call)
from .. import lib as L

__all__ = ["HIPMXFP4Quant", "HIPMXFP4Gemm", "HIPMXFP4GroupGemm", "HIPMXFP4SwiGLUQuant", "HIPMXFP4Experts", "SKINNY_MAX_M"]

SKINNY_MAX_M = 32                      # rows up to which the product takes the skinny form (csrc/mxfp4_gemm.hip: MX_SKINNY_MAX_M)
_BYTE_VIEWS = tuple(getattr(torch, name) for name in ("float4_e2m1fn_x2", "float8_e8m0fnu") if hasattr(torch, name))


def _bytes(what: str, name: str, t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.uint8 and t.dtype not in _BYTE_VIEWS:
        raise NotImplementedError(f"{what}: {name} is {t.dtype}; uint8 (or float4_e2m1fn_x2 / float8_e8m0fnu by view) expected")
    return as_bytes(t).contiguous()


def _on_device(what: str, *tensors) -> None:
    if not all(t.is_cuda for t in tensors):
        raise NotImplementedError(f"{what}: CPU tensors; the hip backend has no CPU path (the core class is the golden)")


def _quantize(what: str, x: torch.Tensor):
    m, k = check_quant_call(what, x)
    _on_device(what, x)
    if (m > 1 and x.stride(0) % 8 != 0) or x.data_ptr() % 16 != 0:
        x = x.contiguous()
    data = torch.empty((m, k // 2), dtype=torch.uint8, device=x.device)
    scale = torch.empty((m, k // BLOCK), dtype=torch.uint8, device=x.device)
    if m == 0:
        return data, scale
    L.check(L.load().mojo_hip_mxfp4_quant(L.ptr(x), L.ptr(data), L.ptr(scale), m, k, x.stride(0) if m > 1 else k,
                                          L.dtype_code(x.dtype), L.stream_of(x)), what)
    return data, scale


def _group_gemm(what, input, input_scale, weight, weight_scale, group_list, k, n, swiglu_quant, output_dtype):
    """The grouped product of one call: every refusal first, then the workspace and ONE library call.  Returns ``[M, N]``, or
    ``(data, scale)`` with ``swiglu_quant``."""
    m, k, n = check_group_call(what, input, input_scale, weight, weight_scale, group_list, k, n)
    if n <= 0 or n % 16 != 0:
        raise NotImplementedError(f"{what}: out_features {n}; multiples of 16 are supported")
    if swiglu_quant and n % (2 * BLOCK) != 0:
        raise ValueError(f"{what}: swiglu_quant wants out_features = 2 I with I a multiple of {BLOCK}, got {n}")
    _on_device(what, input, input_scale, weight, weight_scale, group_list)
    a, sa = _bytes(what, "input", input), _bytes(what, "input_scale", input_scale)
    w, sw = _bytes(what, "weight", weight), _bytes(what, "weight_scale", weight_scale)
    counts, groups = group_list.contiguous(), weight.shape[0]
    if swiglu_quant:
        out = torch.empty((m, n // 4), dtype=torch.uint8, device=a.device)
        out_scale = torch.empty((m, n // (2 * BLOCK)), dtype=torch.uint8, device=a.device)
    else:
        out, out_scale = torch.empty((m, n), dtype=output_dtype, device=a.device), None
    if m > 0:
        lib = L.load()
        ws = torch.empty(lib.mojo_hip_mxfp4_group_gemm_workspace_bytes(m, k, n, groups, int(swiglu_quant)), dtype=torch.uint8,
                         device=a.device)
        L.check(lib.mojo_hip_mxfp4_group_gemm(L.ptr(a), L.ptr(sa), L.ptr(w), L.ptr(sw), L.ptr(out), L.ptr(out_scale), L.ptr(counts),
                                              m, k, n, groups, int(swiglu_quant), L.dtype_code(output_dtype), L.ptr(ws), ws.numel(),
                                              L.stream_of(a)), what)
    return (out, out_scale) if swiglu_quant else out


class HIPMXFP4Quant(MojoMXFP4Quant):
    """One launch: four lanes share a block of 32 elements, each reads one 16-byte vector, the block's largest magnitude is a
    two-step lane exchange, every lane writes its four data bytes and the first the scale byte.  Bit-identical to the core
    golden.  Rows are read by their stride when it is a multiple of 16 bytes, anything else is made dense first.  No host
    sync, capture-safe.  Tag ``mxfp4_quant``."""
    supported_platforms_list = ["rocm"]

    def forward(self, x: torch.Tensor):
        return _quantize("HIPMXFP4Quant", x)


class HIPMXFP4Gemm(MojoMXFP4Gemm):
    """``N % 16 == 0``, any ``M >= 1``, ``K % 32 == 0``; uint8 operands (``float4_e2m1fn_x2`` data and ``float8_e8m0fnu`` scales by
    view).  No atomics: two calls give the same bits.  No host sync, capture-safe.  `mojo_hip_last_launch()` names the form taken:
    ``mxfp4_gemm:tile128`` or ``mxfp4_gemm:skinny:mg<1|2>:splitk<S>``."""
    supported_platforms_list = ["rocm"]

    def forward(self, input: torch.Tensor, input_scale: torch.Tensor) -> torch.Tensor:
        what = "HIPMXFP4Gemm"
        m, k, n = self.check_call_contract(input, input_scale)
        if n <= 0 or n % 16 != 0:
            raise NotImplementedError(f"{what}: out_features {n}; multiples of 16 are supported")
        _on_device(what, input, input_scale, self.weight, self.weight_scale)
        a, sa = _bytes(what, "input", input), _bytes(what, "input_scale", input_scale)
        w, sw = _bytes(what, "weight", self.weight), _bytes(what, "weight_scale", self.weight_scale)
        out = torch.empty((m, n), dtype=self.output_dtype, device=a.device)
        if m == 0:
            return out
        lib = L.load()
        ws = torch.empty(lib.mojo_hip_mxfp4_gemm_workspace_bytes(m, k, n), dtype=torch.uint8, device=a.device)
        L.check(lib.mojo_hip_mxfp4_gemm(L.ptr(a), L.ptr(sa), L.ptr(w), L.ptr(sw), L.ptr(out), m, k, n,
                                        L.dtype_code(self.output_dtype), L.ptr(ws), ws.numel(), L.stream_of(a)), what)
        return out


class HIPMXFP4GroupGemm(MojoMXFP4GroupGemm):
    """``N % 16 == 0``, up to 1024 groups, int32 row counts on the device that are never read on the host.  A plan kernel deals every
    group on its own: more than 32 rows to 128-row tiles, 1..32 rows to the weight-streaming skinny form with a fixed-order
    split-K merge; with ``swiglu_quant`` the product's epilogue writes fp4 data and scale bytes directly (the ``[M, 2I]`` product
    never reaches memory).  No atomics: two calls give the same bits.  No host sync, capture-safe.  `mojo_hip_last_launch()`:
    ``mxfp4_group_gemm:<plain|swiglu>:splitk<S>``."""
    supported_platforms_list = ["rocm"]

    def forward(self, input: torch.Tensor, input_scale: torch.Tensor, group_list: torch.Tensor):
        return _group_gemm("HIPMXFP4GroupGemm", input, input_scale, self.weight, self.weight_scale, group_list, self.in_features,
                           self.out_features, self.swiglu_quant, self.output_dtype)


class HIPMXFP4SwiGLUQuant(MojoMXFP4SwiGLUQuant):
    """One streaming launch, the fused epilogue over a stored ``x``: eight lanes share a block, each reads four gate and four up
    values.  Rows are read by their stride when it is a multiple of 16 bytes, anything else is made dense first.  Tag
    ``mxfp4_swiglu_quant``."""
    supported_platforms_list = ["rocm"]

    def forward(self, x: torch.Tensor):
        what = "HIPMXFP4SwiGLUQuant"
        m, inter = check_swiglu_quant_call(what, x)
        _on_device(what, x)
        if (m > 1 and x.stride(0) * x.element_size() % 16 != 0) or x.data_ptr() % 16 != 0:
            x = x.contiguous()
        data = torch.empty((m, inter // 2), dtype=torch.uint8, device=x.device)
        scale = torch.empty((m, inter // BLOCK), dtype=torch.uint8, device=x.device)
        if m > 0:
            L.check(L.load().mojo_hip_mxfp4_swiglu_quant(L.ptr(x), L.ptr(data), L.ptr(scale), m, inter,
                                                         x.stride(0) if m > 1 else 2 * inter, L.dtype_code(x.dtype),
                                                         L.stream_of(x)), what)
        return data, scale


class HIPMXFP4Experts(MojoMXFP4Experts):
    """Three library calls and no host sync: the row quantiser, fc1 with the fused SwiGLU quantiser, fc2.  ``tokens_per_expert``
    stays on the device and is not validated: rows at or past its sum come back as zeros."""
    supported_platforms_list = ["rocm"]

    def forward(self, sorted_hidden_states: torch.Tensor, tokens_per_expert: torch.Tensor) -> torch.Tensor:
        what = "HIPMXFP4Experts"
        self.check_call_contract(sorted_hidden_states, tokens_per_expert)
        h, i = self.hidden_size, self.intermediate_size
        buffers = (self.up_proj_weight, self.up_proj_weight_scale, self.down_proj_weight, self.down_proj_weight_scale)
        _on_device(what, sorted_hidden_states, tokens_per_expert, *buffers)
        a, sa = _quantize(what, sorted_hidden_states)
        y, sy = _group_gemm(what, a, sa, buffers[0], buffers[1], tokens_per_expert, h, 2 * i, True, sorted_hidden_states.dtype)
        return _group_gemm(what, y, sy, buffers[2], buffers[3], tokens_per_expert, i, h, False, sorted_hidden_states.dtype)
