"""`MXFP4_MOE_OPS` (`MojoMXFP4GroupGemm`, `MojoMXFP4SwiGLUQuant`, `MojoMXFP4Experts`): the core goldens against the fp64 models of
tests/mxfp4_golden.py without a GPU, and the HIP classes (csrc/mxfp4_group_gemm.hip) against them on one.

Exact inputs are those of tests/test_hip_mxfp4.py (scale bytes from {126, 127, 128}, K <= 1024: the fp32 product is exact in any
order), so the grouped product must equal the fp64 model bit for bit, and in the fused stage only the device's `exp` separates the
kernel from the golden.  The stage's criterion is the project's quantiser criterion per byte (`check_stage`).  The count lists put a
group on every boundary of the dealing (empty, 1, 16, 17, 32, 33, 128, 129, 257 rows; an empty first and last group; slack rows)
and send groups to both forms within one call.  Figures measured on an MI355X: DESIGN §4.33."""
import functools
import sys
import types

import pytest
import torch

import mojo_opset_amd as mo
from mojo_opset_amd.backends.hip import lib as L
from mojo_opset_amd.backends.hip.operators.mxfp4 import HIPMXFP4Experts, HIPMXFP4GroupGemm, HIPMXFP4SwiGLUQuant
from mojo_opset_amd.core.operators.mxfp4 import mxfp4_quantize
from mxfp4_golden import gemm_model64, operand, quant_model64

gpu = pytest.mark.gpu
COUNTS = {"boundaries": ((0, 1, 16, 17, 32, 33, 0, 128, 129, 0), 3), "large": ((257, 4), 0)}     # (row counts, slack rows)
EXPERT_COUNTS, HIDDEN, INTER = (5, 0, 40, 17), 160, 96


class TorchMXFP4GroupGemm(mo.MojoMXFP4GroupGemm):
    """The core class's golden ``forward`` as the ``torch`` backend."""
    supported_platforms_list = ["rocm", "cpu"]


class TorchMXFP4SwiGLUQuant(mo.MojoMXFP4SwiGLUQuant):
    supported_platforms_list = ["rocm", "cpu"]


class TorchMXFP4Experts(mo.MojoMXFP4Experts):
    supported_platforms_list = ["rocm", "cpu"]


def group_op(cls, w, sw, groups, device="cpu", **kwargs):
    op = cls(groups, w.shape[1] * 2, w.shape[0] // groups, **kwargs)
    op.weight, op.weight_scale = (t.reshape(groups, -1, t.shape[1]).to(device) for t in (w, sw))
    return op


@functools.lru_cache(maxsize=None)
def grouped_case(counts, slack, k, n, lo=126, hi=128):
    """``(a, sa, w, sw, product, magnitude)``: operands and the fp64 model per group, zeros in the slack rows."""
    m = sum(counts) + slack
    (a, sa), (w, sw) = operand(m, k, lo, hi, 11), operand(len(counts) * n, k, lo, hi, 12)
    want, magnitude, begin = torch.zeros(m, n, dtype=torch.float64), torch.zeros(m, n, dtype=torch.float64), 0
    for g, count in enumerate(counts):
        rows = slice(begin, begin + count)
        if count:
            want[rows], magnitude[rows] = gemm_model64(a[rows], sa[rows], w[g * n:(g + 1) * n], sw[g * n:(g + 1) * n])
        begin += count
    return a, sa, w, sw, want, magnitude


@functools.lru_cache(maxsize=None)
def stage_case(counts, slack, k, inter):
    """The fused stage on exact fc1 inputs: ``(a, sa, w, sw, fc1 fp64, h fp64, golden data, golden scale)``."""
    a, sa, w, sw, fc1, _ = grouped_case(counts, slack, k, 2 * inter)
    h = fc1[:, :inter] * torch.sigmoid(fc1[:, :inter]) * fc1[:, inter:]
    golden = group_op(TorchMXFP4GroupGemm, w, sw, len(counts), swiglu_quant=True)(a, sa, torch.tensor(counts, dtype=torch.int32))
    return a, sa, w, sw, fc1, h, *golden


def check_stage(data, scale, want_data, want_scale, h, what):
    """At most 2e-3 of the data bytes differ; a differing nibble is a neighbouring code of the same sign; scale bytes differ by at
    most 1, and only in blocks whose largest magnitude is within 2^-20 (relative) of a power of two (their nibbles follow the scale)."""
    assert data.dtype == scale.dtype == torch.uint8 and data.shape == want_data.shape and scale.shape == want_scale.shape, what
    moved = scale != want_scale
    amax = h.abs().reshape(h.shape[0], -1, 32).amax(-1)
    to_power = (amax / torch.exp2(torch.round(torch.log2(amax.clamp_min(1e-300)))) - 1).abs()
    assert bool(((scale.int() - want_scale.int()).abs() <= 1).all()) and bool((to_power[moved] <= 2.0 ** -20).all()), what
    share = float((data != want_data).float().mean())
    print(f"{what}: {int((data != want_data).sum())} of {data.numel()} data bytes differ (share {share:.2e}), {int(moved.sum())} scale bytes")
    assert share <= 2e-3, what
    keep = ~moved.repeat_interleave(16, dim=1)
    for shift in (0, 4):
        got, want = (data >> shift) & 0xF, (want_data >> shift) & 0xF
        assert bool((((got.int() - want.int()).abs() <= 1) & ((got ^ want) < 8))[keep].all()), what


def test_goldens_against_the_fp64_model_on_exact_inputs():
    counts, slack, k, inter = (0, 5, 33, 0, 7), 3, 544, 32
    a, sa, w, sw, want, _ = grouped_case(counts, slack, k, 2 * inter)
    group_list = torch.tensor(counts, dtype=torch.int32)
    fc1 = group_op(TorchMXFP4GroupGemm, w, sw, 5, output_dtype=torch.float32)(a, sa, group_list)
    assert fc1.shape == (48, 64) and torch.equal(fc1.double(), want) and not fc1[45:].any() and bool(fc1[:45].any(1).all())
    assert torch.equal(group_op(TorchMXFP4GroupGemm, w, sw, 5)(a, sa, group_list), want.to(torch.bfloat16))
    data, scale = group_op(TorchMXFP4GroupGemm, w, sw, 5, swiglu_quant=True)(a, sa, group_list)
    alone = TorchMXFP4SwiGLUQuant()(fc1)
    assert data.shape == (48, 16) and scale.shape == (48, 1) and torch.equal(data, alone[0]) and torch.equal(scale, alone[1])
    assert not data[45:].any() and not scale[45:].any()


@pytest.mark.parametrize("name", ["sets", "constructors", "plugin", "activation", "I % 32", "N % 16", "group_list dtype",
                                  "group_list length", "CPU tensors", "[G, K, N] weights", "odd halves", "CPU stage", "CPU experts"])
def test_wiring_and_refusals_before_any_device_work(name):
    """CPU tensors throughout: a refusal that came behind the first device step would be the loader's `MojoHipError` instead."""
    names = ("MojoMXFP4GroupGemm", "MojoMXFP4SwiGLUQuant", "MojoMXFP4Experts")
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8)                                   # noqa: E731
    if name == "sets":
        assert mo.MXFP4_MOE_OPS == mo.core.MXFP4_MOE_OPS == mo.core.operators.MXFP4_MOE_OPS == names
        assert not set(names) & (set(mo.__all__) | set(mo.BEYOND_SURVEY_OPS) | set(mo.MXFP4_OPS))
        assert all(getattr(mo, n) is getattr(mo.core, n) for n in names)
    elif name == "constructors":
        op = TorchMXFP4GroupGemm(3, 64, 128, swiglu_quant=True)
        assert op.weight.shape == (3, 128, 32) and op.weight_scale.shape == (3, 128, 2) and op.output_dtype == torch.bfloat16
        assert op.weight.dtype == op.weight_scale.dtype == torch.uint8 and "swiglu_quant=True" in repr(op)
        ex = TorchMXFP4Experts(4, HIDDEN, INTER)
        assert ex.up_proj_weight.shape == (4, 192, 80) and ex.up_proj_weight_scale.shape == (4, 192, 5)
        assert ex.down_proj_weight.shape == (4, 160, 48) and ex.down_proj_weight_scale.shape == (4, 160, 3)
    elif name == "plugin":
        from mojo_opset_amd import plugin

        ref = types.ModuleType("stand_in_mxfp4_moe_reference")
        cores = {n: type(n, (mo.core.MojoOperator,), {"forward": lambda self, *a, **k: None}) for n in names}
        vars(ref).update(cores)
        sys.modules[ref.__name__] = ref
        try:
            made = plugin.rebase_hip_backend(ref, platforms=["rocm", "cpu"])
        finally:
            del sys.modules[ref.__name__]
        for n, hip in zip(names, (HIPMXFP4GroupGemm, HIPMXFP4SwiGLUQuant, HIPMXFP4Experts)):
            assert issubclass(made[n], cores[n]) and made[n].forward is hip.forward
    else:
        error = ValueError if name in ("I % 32", "group_list length", "odd halves") else NotImplementedError
        with pytest.raises(error):
            if name == "activation":
                HIPMXFP4Experts(4, HIDDEN, INTER, activation="gelu")
            elif name == "I % 32":
                HIPMXFP4GroupGemm(2, 64, 96, swiglu_quant=True)
            elif name in ("odd halves", "CPU stage"):
                HIPMXFP4SwiGLUQuant()(torch.zeros(2, 96 if name == "odd halves" else 64))
            elif name == "CPU experts":
                HIPMXFP4Experts(4, HIDDEN, INTER)(torch.zeros(3, HIDDEN, dtype=torch.bfloat16), torch.zeros(4, dtype=torch.int32))
            else:
                op = HIPMXFP4GroupGemm(2, 64, 24 if name == "N % 16" else 32)
                if name == "[G, K, N] weights":
                    op.weight, op.weight_scale = u8(2, 64, 16), u8(2, 2, 32)
                op(u8(4, 32), u8(4, 2), torch.zeros(3 if name == "group_list length" else 2,
                                                    dtype=torch.int64 if name == "group_list dtype" else torch.int32))


@pytest.mark.parametrize("case", COUNTS)
@pytest.mark.parametrize("inter", [32, 96, 160])
def test_the_stage_inputs_do_not_sit_on_thresholds_for_the_reference_itself(case, inter):
    """The golden (fp32 ``silu``) against the same rule with an fp64 ``silu``, inside the criterion of the GPU test below."""
    for k in (160, 1024):
        _, _, _, _, _, h, data, scale = stage_case(*COUNTS[case], k, inter)
        check_stage(data, scale, *quant_model64(h), h, f"golden fp32 against fp64 silu, {case} I {inter} K {k}")


@gpu
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", COUNTS)
def test_hip_grouped_product_is_exact_on_exact_inputs(case, out_dtype):
    counts, slack = COUNTS[case]
    group_list = torch.tensor(counts, dtype=torch.int32, device="cuda")
    for k in (32, 160, 544, 1024):
        for n in (16, 48, 272):
            a, sa, w, sw, want, _ = grouped_case(counts, slack, k, n)
            got = group_op(HIPMXFP4GroupGemm, w, sw, len(counts), "cuda", output_dtype=out_dtype)(a.cuda(), sa.cuda(), group_list)
            assert L.last_launch() == f"mxfp4_group_gemm:plain:splitk{2 if k > 512 else 1}", L.last_launch()
            assert got.dtype == out_dtype and torch.equal(got.cpu(), want.to(out_dtype)), (k, n)


@gpu
@pytest.mark.parametrize("case", COUNTS)
@pytest.mark.parametrize("inter", [32, 96, 160])
def test_hip_fused_stage_and_stand_alone_stage_against_the_golden(case, inter):
    counts, slack = COUNTS[case]
    group_list = torch.tensor(counts, dtype=torch.int32, device="cuda")
    for k in (160, 1024):
        a, sa, w, sw, fc1, h, want_data, want_scale = stage_case(counts, slack, k, inter)
        data, scale = group_op(HIPMXFP4GroupGemm, w, sw, len(counts), "cuda", swiglu_quant=True)(a.cuda(), sa.cuda(), group_list)
        assert L.last_launch() == f"mxfp4_group_gemm:swiglu:splitk{2 if k > 512 else 1}", L.last_launch()
        check_stage(data.cpu(), scale.cpu(), want_data, want_scale, h, f"fused {case} I {inter} K {k}")
        alone = HIPMXFP4SwiGLUQuant()(fc1.float().cuda())                          # one epilogue: the same bits
        assert L.last_launch() == "mxfp4_swiglu_quant" and torch.equal(alone[0], data) and torch.equal(alone[1], scale)
        for dtype in (torch.bfloat16, torch.float16):                              # 16-bit x, rows by a stride
            x = torch.zeros(fc1.shape[0], 2 * inter + 8, dtype=dtype, device="cuda")
            x[:, :2 * inter] = fc1.clamp(-6e4, 6e4).to(dtype).cuda()
            got, want = HIPMXFP4SwiGLUQuant()(x[:, :2 * inter]), TorchMXFP4SwiGLUQuant()(x[:, :2 * inter].cpu())
            h16 = torch.nn.functional.silu(x[:, :inter].cpu().double()) * x[:, inter:2 * inter].cpu().double()
            check_stage(got[0].cpu(), got[1].cpu(), *want, h16, f"stand-alone {dtype} {case} I {inter} K {k}")


@gpu
def test_hip_grouped_product_with_wide_scales_is_within_the_derived_bound():
    counts, slack, k, n = (8, 0, 192, 40, 0), 2, 2880, 320
    a, sa, w, sw, want, magnitude = grouped_case(counts, slack, k, n, 107, 147)
    got = group_op(HIPMXFP4GroupGemm, w, sw, len(counts), "cuda", output_dtype=torch.float32)(
        a.cuda(), sa.cuda(), torch.tensor(counts, dtype=torch.int32, device="cuda")).cpu().double()
    splits = int(L.last_launch().rsplit("splitk", 1)[1])
    rows = sum(counts)
    ratio = float(((got[:rows] - want[:rows]).abs() / ((k // 32 + splits + 2) * 2.0 ** -23 * magnitude[:rows])).max())
    print(f"{L.last_launch()}: max |err| / bound = {ratio:.4f}")
    assert ratio <= 1.0 and not got[rows:].any()


@functools.lru_cache(maxsize=None)
def experts_case():
    """``(x, buffers, golden, distance)``: the core golden and its own largest distance to an fp64 model of the chain."""
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(sum(EXPERT_COUNTS) + 2, HIDDEN, generator=gen).to(torch.bfloat16)
    up, down = torch.randn(4 * 2 * INTER, HIDDEN, generator=gen) * 0.1, torch.randn(4 * HIDDEN, INTER, generator=gen) * 0.1
    (uw, us), (dw, ds) = mxfp4_quantize(up), mxfp4_quantize(down)
    buffers = {"up_proj_weight": uw.reshape(4, 2 * INTER, -1), "up_proj_weight_scale": us.reshape(4, 2 * INTER, -1),
               "down_proj_weight": dw.reshape(4, HIDDEN, -1), "down_proj_weight_scale": ds.reshape(4, HIDDEN, -1)}
    golden = experts_op(TorchMXFP4Experts, buffers)(x, torch.tensor(EXPERT_COUNTS, dtype=torch.int32))
    model, begin = torch.zeros(x.shape[0], HIDDEN, dtype=torch.float64), 0
    a, sa = quant_model64(x)
    for e, count in enumerate(EXPERT_COUNTS):
        rows = slice(begin, begin + count)
        if not count:
            continue
        fc1 =gemm_model64(a[rows], sa[rows], buffers["up_proj_weight"][e], buffers["up_proj_weight_scale"][e])[0]
        y, sy = quant_model64(fc1[:, :INTER] * torch.sigmoid(fc1[:, :INTER]) * fc1[:, INTER:])
        model[rows] = gemm_model64(y, sy, buffers["down_proj_weight"][e], buffers["down_proj_weight_scale"][e])[0]
        begin += count
    return x, buffers, golden, float((golden.double() - model).abs().max())


def experts_op(cls, buffers, device="cpu"):
    op = cls(4, HIDDEN, INTER)
    for name, value in buffers.items():
        setattr(op, name, value.to(device))
    return op


@gpu
def test_hip_experts_end_to_end_repeatable_and_capturable():
    """Tolerance: twice the golden's own distance to the fp64 model of the chain (both sides sit one quantisation away from it)."""
    x, buffers, golden, distance = experts_case()
    op, xd = experts_op(HIPMXFP4Experts, buffers, "cuda"), x.cuda()
    counts = torch.tensor(EXPERT_COUNTS, dtype=torch.int32, device="cuda")
    got = op(xd, counts)
    error = float((got.cpu().double() - golden.double()).abs().max())
    print(f"experts: max |hip - golden| = {error:.3e}, golden's distance to the fp64 model = {distance:.3e}")
    assert got.dtype == torch.bfloat16 and error <= 2 * distance and not got[sum(EXPERT_COUNTS):].any()
    assert torch.equal(op(xd, counts), got)
    graph, static = torch.cuda.CUDAGraph(), None
    with torch.cuda.graph(graph):
        static = op(xd, counts)
    for _ in range(3):
        static.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static, got)
