"""`MojoMXFP4Quant` / `MojoMXFP4Gemm` (`MXFP4_OPS`): the core goldens against the fp64 models of tests/mxfp4_golden.py without a GPU,
and `HIPMXFP4Quant` / `HIPMXFP4Gemm` (csrc/mxfp4_gemm.hip) against the same models on one.

Exact inputs: scale bytes from {126, 127, 128} make every product a multiple of 1/16 with partial sums below 2^24 such units at
K <= 1024, so the fp32 result is exact in any summation order and must equal the fp64 model bit for bit.  Wide scales (derived, not
measured): ``|out - ref64| <= (K/32 + S + 2) 2^-23 sum_k |a_k b_k|``, one truncation of the running sum per block and per merge of
``S`` K-splits.  Largest ``max |err| / bound`` measured on an MI355X: see DESIGN §4.32."""
import sys
import types

import pytest
import torch

import mojo_opset_amd as mo
from mojo_opset_amd.backends.hip import lib as L
from mojo_opset_amd.backends.hip.operators.mxfp4 import SKINNY_MAX_M, HIPMXFP4Gemm, HIPMXFP4Quant
from mojo_opset_amd.core.operators.mxfp4 import mxfp4_dequantize, mxfp4_quantize
from mxfp4_golden import TIE_CODES, dequant_model64, gemm_model64, operand, quant_input, quant_model64

gpu = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]


class TorchMXFP4Quant(mo.MojoMXFP4Quant):
    """The core class's golden ``forward`` as the ``torch`` backend."""
    supported_platforms_list = ["rocm", "cpu"]


class TorchMXFP4Gemm(mo.MojoMXFP4Gemm):
    supported_platforms_list = ["rocm", "cpu"]


def gemm_op(cls, w, sw, output_dtype, device="cpu"):
    op = cls(w.shape[1] * 2, w.shape[0], output_dtype)
    op.weight, op.weight_scale = w.to(device), sw.to(device)
    return op


def split_of(tag):
    return int(tag.rsplit("splitk", 1)[1]) if "splitk" in tag else 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_quantiser_golden_against_the_fp64_model(dtype):
    x = quant_input(3, 4128, dtype)
    data, scale = TorchMXFP4Quant()(x)
    want_data, want_scale = quant_model64(x)
    assert torch.equal(data, want_data) and torch.equal(scale, want_scale)
    assert data.dtype == scale.dtype == torch.uint8 and data.shape == (3, 2064) and scale.shape == (3, 129)
    codes = torch.stack((data[0, :7] & 0xF, data[0, :7] >> 4), -1).reshape(-1)
    assert codes.tolist() == list(TIE_CODES) + [8 + c for c in TIE_CODES]     # the ties of block 0, both signs
    assert scale[0, :10].tolist()[2:] == [127, 0, 0 if dtype == torch.bfloat16 else 110, 252 if dtype == torch.bfloat16 else 140,
                                          255, 255, 255, 255]
    assert int(data[0, 32] & 0xF) == 7 and int(data[0, 32] >> 4) == 15 and int(data[0, 33] & 0xF) == 7   # 7.75, -7, 6.5 saturate
    assert data[0, 48:64].tolist() == [0x80, 0, 0x80] + [0] * 13              # the zero block keeps its signs
    assert not data[0, 96:160].any()                                          # Inf / NaN blocks: zero nibbles
    grid = mxfp4_dequantize(*operand(5, 160, 120, 134, 1)).to(dtype)          # values on the grid survive the round trip
    assert torch.equal(mxfp4_dequantize(*mxfp4_quantize(grid)), grid.float())


@pytest.mark.parametrize("m,n,k", [(5, 16, 32), (33, 48, 544)])
def test_gemm_golden_against_the_fp64_model_on_exact_inputs(m, n, k):
    (a, sa), (w, sw) = operand(m, k, 126, 128, 2), operand(n, k, 126, 128, 3)
    assert torch.equal(mxfp4_dequantize(a, sa).double(), dequant_model64(a, sa))
    want = gemm_model64(a, sa, w, sw)[0]
    assert torch.equal(gemm_op(TorchMXFP4Gemm, w, sw, torch.float32)(a, sa).double(), want)
    assert torch.equal(gemm_op(TorchMXFP4Gemm, w, sw, torch.bfloat16)(a, sa), want.to(torch.bfloat16))


def test_sets_constructor_and_plugin():
    names = ("MojoMXFP4Quant", "MojoMXFP4Gemm")
    assert mo.MXFP4_OPS == mo.core.MXFP4_OPS == mo.core.operators.MXFP4_OPS == names
    assert not set(names) & set(mo.__all__) and not set(names) & set(mo.BEYOND_SURVEY_OPS)
    op = TorchMXFP4Gemm(64, 16)
    assert op.output_dtype == torch.bfloat16 and op.weight.shape == (16, 32) and op.weight_scale.shape == (16, 2)
    assert op.weight.dtype == op.weight_scale.dtype == torch.uint8 and "in_features=64" in repr(op)
    from mojo_opset_amd import plugin

    ref = types.ModuleType("stand_in_mxfp4_reference")
    cores = {n: type(n, (mo.core.MojoOperator,), {"forward": lambda self, *a, **k: None}) for n in names}
    vars(ref).update(cores)
    sys.modules[ref.__name__] = ref
    try:
        made = plugin.rebase_hip_backend(ref, platforms=["rocm", "cpu"])
    finally:
        del sys.modules[ref.__name__]
    for name, hip in zip(names, (HIPMXFP4Quant, HIPMXFP4Gemm)):
        assert issubclass(made[name], cores[name]) and made[name].forward is hip.forward


@pytest.mark.parametrize("name,error", [("K 48", ValueError), ("scale shape", ValueError), ("N 24", NotImplementedError),
                                        ("int8 input", NotImplementedError), ("CPU tensors", NotImplementedError),
                                        ("fp32 quant", NotImplementedError), ("quant K 40", ValueError)])
def test_refusals_come_before_any_device_work(name, error):
    """CPU tensors throughout: a refusal that came behind the first device step would be the loader's `MojoHipError` instead."""
    with pytest.raises(error):
        if "quant" in name:
            HIPMXFP4Quant()(torch.zeros(2, 40 if name == "quant K 40" else 64, dtype=torch.float32 if name == "fp32 quant" else torch.bfloat16))
        else:
            op = HIPMXFP4Gemm(48 if name == "K 48" else 64, 24 if name == "N 24" else 16)
            a = torch.zeros(2, 32, dtype=torch.int8 if name == "int8 input" else torch.uint8)
            op(a, torch.zeros(2, 3 if name == "scale shape" else 2, dtype=torch.uint8))


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [1, 3, 257])
@pytest.mark.parametrize("k", [32, 160, 4128])
def test_hip_quantiser_is_bit_identical_to_the_golden(m, k, dtype):
    x = quant_input(m, k, dtype)
    want_data, want_scale = mxfp4_quantize(x)
    data, scale = HIPMXFP4Quant()(x.cuda())
    assert L.last_launch() == "mxfp4_quant"
    assert torch.equal(data.cpu(), want_data) and torch.equal(scale.cpu(), want_scale)
    wide = torch.zeros(m, k + 64, dtype=dtype, device="cuda")                 # the same rows by a stride
    wide[:, 8:k + 8] = x.cuda()
    data, scale = HIPMXFP4Quant()(wide[:, 8:k + 8])
    assert torch.equal(data.cpu(), want_data) and torch.equal(scale.cpu(), want_scale)


@gpu
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("m", [1, 16, 17, 33, 128, 257])
def test_hip_gemm_is_exact_on_exact_inputs(m, out_dtype):
    for k in (32, 128, 160, 544, 1024):
        a, sa = operand(m, k, 126, 128, 4)
        for n in (16, 48, 272):
            w, sw = operand(n, k, 126, 128, 5)
            got = gemm_op(HIPMXFP4Gemm, w, sw, out_dtype, "cuda")(a.cuda(), sa.cuda())
            assert L.last_launch().startswith("mxfp4_gemm:skinny" if m <= SKINNY_MAX_M else "mxfp4_gemm:tile128")
            want = gemm_model64(a, sa, w, sw)[0]
            assert got.dtype == out_dtype and torch.equal(got.cpu(), want.to(out_dtype)), (m, n, k)


@gpu
@pytest.mark.parametrize("m", [8, 192])
def test_hip_gemm_with_wide_scales_is_within_the_derived_bound(m):
    k, n = 2880, 320
    (a, sa), (w, sw) = operand(m, k, 107, 147, 6), operand(n, k, 107, 147, 7)
    got = gemm_op(HIPMXFP4Gemm, w, sw, torch.float32, "cuda")(a.cuda(), sa.cuda())
    want, magnitude = gemm_model64(a, sa, w, sw)
    ratio = float(((got.cpu().double() - want).abs() / ((k // 32 + split_of(L.last_launch()) + 2) * 2.0 ** -23 * magnitude)).max())
    print(f"{L.last_launch()}: max |err| / bound = {ratio:.4f}")
    assert ratio <= 1.0


@gpu
@pytest.mark.parametrize("m", [8, 192])
def test_hip_quant_then_gemm_end_to_end_repeatable_and_capturable(m):
    k, n = 2880, 320
    gen = torch.Generator().manual_seed(8 + m)
    x, wx = (torch.randn(rows, k, generator=gen).to(torch.bfloat16) for rows in (m, n))
    w, sw = mxfp4_quantize(wx)
    quant, gemm = HIPMXFP4Quant(), gemm_op(HIPMXFP4Gemm, w, sw, torch.bfloat16, "cuda")
    xd = x.cuda()
    got = gemm(*quant(xd))
    a, sa = TorchMXFP4Quant()(x)
    golden = gemm_op(TorchMXFP4Gemm, w, sw, torch.bfloat16)(a, sa)
    want, magnitude = gemm_model64(a, sa, w, sw)
    bound = (k // 32 + split_of(L.last_launch()) + 2) * 2.0 ** -23 * magnitude
    for out in (got.cpu(), golden):               # the kernel and the golden: the same bound + one rounding to bf16 (u = 2^-8)
        assert bool(((out.double() - want).abs() <= bound + 2.0 ** -8 * (want.abs() + bound)).all())
    assert torch.equal(gemm(*quant(xd)), got)
    graph, static = torch.cuda.CUDAGraph(), None
    with torch.cuda.graph(graph):
        static = gemm(*quant(xd))
    for _ in range(3):
        static.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static, got)
