"""The dense W8A8 quantiser ops (`QUANT_DENSE_OPS`) without a GPU: the goldens against the recorded reference outputs,
registration, the op set, the plugin, constructor and call-contract errors (the checks of `HIP<Op>.forward` that run before any
device work among them), and the room the GPU tests' inputs leave for their bound.

The recorded outputs (tests/make_quant_dense_golden.py) are one file under the 1 MiB bound of a committed file."""
import os
import sys
import types

import pytest
import torch

import mojo_opset_amd as mo
import quant_dense_golden as G
import quant_dense_utils as U
from conftest import GOLDEN, bit_equal, build_op, clone_tree, load_golden
from mojo_opset_amd.core import MojoOperator
from mojo_opset_amd.core.platform import get_platform

NAMES = ("MojoRMSNormQuant", "MojoLayerNormQuant", "MojoResidualAddLayerNormQuant", "MojoStaticQuant", "MojoDequant",
         "MojoDequantSwiGLUQuant")
CASES = load_golden("quant_dense")
IDS = [pytest.param(c, id=f"{c['op']}-{i}") for i, c in enumerate(CASES)]
I8, F8, BF16, F16, F32 = torch.int8, torch.float8_e4m3fn, torch.bfloat16, torch.float16, torch.float32


@pytest.mark.parametrize("case", IDS)
def test_golden_reproduces_the_reference_bit_for_bit(case):
    op = build_op(U.golden_cls(case["op"]), case)
    with torch.no_grad():
        out = op.forward(*clone_tree(case["args"]), **clone_tree(case["kwargs"]))
    want = case["out"]
    if not isinstance(want, tuple):
        out, want = (out,), (want,)
    assert len(out) == len(want)
    for got, exp in zip(out, want):
        assert got.dtype == exp.dtype and got.shape == exp.shape
        assert torch.equal(got, exp) if got.dtype != F8 else bit_equal(got, exp)


def test_fixture_is_small_and_covers_the_envelope():
    assert os.path.getsize(os.path.join(GOLDEN, "quant_dense.pt")) < 1 << 20
    assert {c["op"] for c in CASES} == set(NAMES)
    by = {n: [c for c in CASES if c["op"] == n] for n in NAMES}
    for name in NAMES[:3]:
        kw = [c["ctor"]["kwargs"] for c in by[name]]
        assert {k.get("quant_dtype", I8) for k in kw} == {I8, F8} and any(k.get("symmetric") is False for k in kw)
        assert {c["args"][0].shape[-1] for c in by[name]} == {128, 257, 1000}
        assert {c["args"][0].dtype for c in by[name]} == {BF16, F16, F32} and any(c["args"][0].dim() == 3 for c in by[name])
        assert {c["args"][-1] is None for c in by[name]} == {True, False}                      # smooth scale on and off
    assert any(c["ctor"]["kwargs"].get("elementwise_affine") is False for c in by["MojoLayerNormQuant"])
    assert {c["ctor"]["kwargs"]["norm_pos"] for c in by["MojoResidualAddLayerNormQuant"]} == {"pre", "post"}
    for c in by["MojoResidualAddLayerNormQuant"]:             # both norm_pos return the sum in the input dtype
        assert c["out"][1].dtype == c["args"][0].dtype and torch.equal(c["out"][1], c["args"][0] + c["args"][1])
    grouped = {(tuple(c["args"][0].shape), tuple(c["ctor"]["kwargs"]["input_size"])) for c in by["MojoStaticQuant"]}
    assert {((2, 4, 128), (4, 128)), ((5, 2, 16, 32), (16, 32))} <= grouped
    assert {c["args"][0].dtype for c in by["MojoDequant"]} == {I8, F8}
    assert {c["ctor"]["kwargs"]["output_dtype"] for c in by["MojoDequant"]} == {BF16, F16, F32}
    assert any(c["args"][1].shape == c["args"][0].shape[:-1] + (1,) for c in by["MojoDequant"])
    swiglu = by["MojoDequantSwiGLUQuant"]
    shapes = {(c["args"][0].shape[0], c["args"][0].shape[1] // 2, tuple(c["args"][4].tolist())) for c in swiglu if c["args"][4] is not None}
    assert {(12, 64, (4, 3, 5)), (20, 128, (6, 4, 7, 3)), (24, 256, (5, 8, 4, 7)), (30, 512, (6, 3, 8, 5, 8))} <= shapes
    assert any(c["args"][4] is not None and 0 in c["args"][4].tolist() for c in swiglu)
    assert any(c["ctor"]["kwargs"]["activate_left"] and c["args"][2] is not None and c["args"][1] is None for c in swiglu)
    assert any(c["args"][4] is None for c in swiglu)

    def plain(x):
        if isinstance(x, (list, tuple)):
            return all(plain(v) for v in x)
        if isinstance(x, dict):
            return all(isinstance(k, str) and plain(v) for k, v in x.items())
        return x is None or isinstance(x, (torch.Tensor, torch.dtype, bool, int, float, str))
    assert plain(CASES)


def test_dispatch_registers_torch_and_hip():
    from mojo_opset_amd.backends import hip

    for name in NAMES:
        core = getattr(mo, name)
        assert core.get_backend_impl("torch", strict=True) is U.golden_cls(name)
        hip_cls = getattr(hip, "HIP" + name[4:])
        assert issubclass(hip_cls, core)
        if get_platform() == "rocm":
            assert core.get_backend_impl("hip", strict=True) is hip_cls


def test_quant_dense_ops_is_a_set_of_its_own():
    assert tuple(mo.QUANT_DENSE_OPS) == NAMES and tuple(mo.core.QUANT_DENSE_OPS) == NAMES
    for name in NAMES:
        assert getattr(mo, name).__name__ == name and getattr(mo.core, name) is getattr(mo, name) and name not in mo.__all__
        for other in (mo.EXTENDED_OPS, mo.KV_INT8_OPS, mo.KV_INT8_SWA_OPS, mo.QUANT_MOE_OPS, mo.SAMPLING_OPS, mo.BEYOND_SURVEY_OPS,
                      mo.NSTEP_OPS, mo.NSTEP_KV_INT8_OPS, mo.PACKED_ATTN_OPS):
            assert name not in other
    assert len(mo.BEYOND_SURVEY_OPS) == 16


def test_rebase_registers_the_classes_into_a_stand_in_reference():
    """`plugin.rebase_hip_backend` walks ``QUANT_DENSE_OPS`` too: every class lands on the reference's core class of that name,
    keeps the reference's constructor and takes this repository's forward."""
    from mojo_opset_amd import plugin
    from mojo_opset_amd.backends import hip

    ref = types.ModuleType("stand_in_quant_dense_reference")
    cores = {}
    for name in NAMES:
        mine = getattr(mo, name)
        cores[name] = type(name, (MojoOperator,), {"__init__": mine.__init__, "forward": lambda self, *a, **k: None,
                                                   "extra_repr": mine.extra_repr, "__module__": ref.__name__})
        setattr(ref, name, cores[name])
    sys.modules[ref.__name__] = ref
    try:
        made = plugin.rebase_hip_backend(ref, platforms=["rocm", "cpu"])
    finally:
        del sys.modules[ref.__name__]
    for name in NAMES:
        cls = made[name]
        assert cls.__name__ == "HIP" + name[4:] and issubclass(cls, cores[name])
        assert cls.forward is getattr(hip, "HIP" + name[4:]).forward
        assert "__init__" not in vars(cls) and "extra_repr" not in vars(cls)
        if get_platform() == "rocm":
            assert cores[name].get_backend_impl("hip", strict=True) is cls


def test_constructors_state_and_repr_follow_the_reference():
    op = G.TorchRMSNormQuant(norm_size=16, eps=1e-6, symmetric=False)
    assert (op.q_max, op.q_min, op.variance_epsilon) == (127, 0, 1e-6) and list(op.state_dict()) == ["weight"]
    assert op.extra_repr() == "norm_size=16, variance_epsilon=1e-06, quant_dtype=torch.int8, symmetric=False"
    op = G.TorchLayerNormQuant(norm_size=16, quant_dtype=F8)
    assert (op.q_max, op.q_min) == (448.0, -448.0) and list(op.state_dict()) == ["weight", "bias"]
    assert op.extra_repr() == ("norm_size=16, variance_epsilon=1e-05, elementwise_affine=True, quant_dtype=torch.float8_e4m3fn, "
                               "symmetric=True")
    op = G.TorchResidualAddLayerNormQuant(norm_size=16, elementwise_affine=False, norm_pos="post")
    assert op.weight is None and op.bias is None and list(op.state_dict()) == []
    assert op.extra_repr() == ("norm_size=16, variance_epsilon=1e-05, elementwise_affine=False, norm_pos='post', "
                               "quant_dtype=torch.int8, symmetric=True")
    op = G.TorchStaticQuant(input_size=8)
    assert op.input_size == (8,) and tuple(op.scale.shape) == (8,)
    op = G.TorchStaticQuant(input_size=[4, 8], quant_dtype=F8)
    assert op.input_size == (4, 8) and tuple(op.scale.shape) == (4, 8) and list(op.state_dict()) == ["scale"]
    assert op.extra_repr() == "input_size=(4, 8), quant_dtype=torch.float8_e4m3fn, q_max=448.0, q_min=-448.0"
    assert G.TorchDequant().output_dtype == BF16 and list(G.TorchDequant().state_dict()) == []
    assert G.TorchDequant(output_dtype=F16).extra_repr() == "output_dtype=torch.float16"      # (the reference's raises)
    op = G.TorchDequantSwiGLUQuant(expert_num=3, hidden_size=8, activate_left=True, dtype=BF16)
    assert {k: (tuple(v.shape), v.dtype) for k, v in op.state_dict().items()} == \
        {"weight_scale": ((3, 16), BF16), "quant_scale": ((3, 8), BF16)}
    assert op.extra_repr() == "expert_num=3, hidden_size=8, quant_dtype=torch.int8, activate_left=True, quant_mode=1"

    for cls in (G.TorchRMSNormQuant, G.TorchLayerNormQuant, G.TorchResidualAddLayerNormQuant):
        with pytest.raises(NotImplementedError, match="Unsupported quant_dtype"):
            cls(norm_size=8, quant_dtype=torch.int16)
    with pytest.raises(ValueError, match="norm_pos"):
        G.TorchResidualAddLayerNormQuant(norm_size=8, norm_pos="mid")
    with pytest.raises(NotImplementedError, match="Unsupported quant_dtype"):
        G.TorchStaticQuant(input_size=8, quant_dtype=torch.int16)
    with pytest.raises(NotImplementedError, match="Unsupported output_dtype"):
        G.TorchDequant(output_dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="Unsupported quant_dtype"):
        G.TorchDequantSwiGLUQuant(expert_num=1, hidden_size=8, quant_dtype=F8)
    with pytest.raises(NotImplementedError, match="quant_mode"):
        G.TorchDequantSwiGLUQuant(expert_num=1, hidden_size=8, quant_mode=0)


def test_call_contract_errors_need_no_gpu():
    """The refusals of golden and hip backend alike; `HIP<Op>.forward` raises them before it touches a device."""
    from mojo_opset_amd.backends import hip
    from mojo_opset_amd.backends.hip.lib import MojoHipError

    for cls in (G.TorchStaticQuant, hip.HIPStaticQuant):
        op = cls(input_size=(4, 8))
        with pytest.raises(ValueError, match="at least 2 dims"):
            op.forward(torch.zeros(8))
        with pytest.raises(ValueError, match="trailing dims"):
            op.forward(torch.zeros(3, 8, 4))
    for cls in (G.TorchDequantSwiGLUQuant, hip.HIPDequantSwiGLUQuant):
        op = cls(expert_num=2, hidden_size=4)
        with pytest.raises(ValueError, match="must be 2D"):
            op.forward(torch.zeros(2, 3, 8))
        with pytest.raises(ValueError, match="must be even"):
            cls(expert_num=1, hidden_size=4).forward(torch.zeros(3, 7))
        with pytest.raises(NotImplementedError, match="quant_offset"):
            op.forward(torch.zeros(3, 8), None, None, torch.zeros(4), torch.tensor([1, 2]))
        with pytest.raises(ValueError, match="token_count is required"):
            op.forward(torch.zeros(3, 8))
    op = hip.HIPDequantSwiGLUQuant(expert_num=2, hidden_size=4)
    with pytest.raises(TypeError, match="int32 or int64"):
        op.forward(torch.zeros(3, 8), token_count=torch.tensor([1.0, 2.0]))
    with pytest.raises(ValueError, match="token_count must be 1D"):
        op.forward(torch.zeros(3, 8), token_count=torch.tensor([1, 1, 1]))
    with pytest.raises(ValueError, match="bias must have shape"):
        op.forward(torch.zeros(3, 8), bias=torch.zeros(4), token_count=torch.tensor([1, 2]))
    with pytest.raises(ValueError, match="one value per token"):
        op.forward(torch.zeros(3, 8), activation_scale=torch.zeros(2), token_count=torch.tensor([1, 2]))
    with pytest.raises(NotImplementedError, match="x dtype"):
        op.forward(torch.zeros(3, 8, dtype=torch.int64), token_count=torch.tensor([1, 2]))
    with pytest.raises(ValueError, match="does not match"):
        op.forward(torch.zeros(3, 10), token_count=torch.tensor([1, 2]))
    with pytest.raises(NotImplementedError, match=r"\(3, 1, 8\).*\(3, 4, 8\)"):
        hip.HIPDequant().forward(torch.zeros(3, 4, 8, dtype=I8), torch.ones(3, 1, 8))
    with pytest.raises(NotImplementedError, match="input dtype"):
        hip.HIPDequant().forward(torch.zeros(3, 8), torch.ones(8))
    with pytest.raises(NotImplementedError, match="share shape and dtype"):
        hip.HIPResidualAddLayerNormQuant(norm_size=8).forward(torch.zeros(2, 8), torch.zeros(2, 8, dtype=F16))
    # past the checks: no CPU path
    with pytest.raises(MojoHipError, match="CPU tensor"):
        hip.HIPStaticQuant(input_size=8).forward(torch.zeros(2, 8))
    with pytest.raises(MojoHipError, match="CPU tensor"):
        hip.HIPDequant().forward(torch.zeros(2, 8, dtype=I8), torch.ones(2, 1))
    with pytest.raises(MojoHipError, match="CPU tensor"):
        hip.HIPRMSNormQuant(norm_size=8).forward(torch.zeros(2, 8))
    with pytest.raises(MojoHipError, match="CPU tensor"):
        hip.HIPDequantSwiGLUQuant(expert_num=1, hidden_size=4).forward(torch.zeros(3, 8))


def test_dequant_scale_forms():
    from mojo_opset_amd.backends.hip.operators.quantize import dequant_scale_form as form

    assert form((2, 4, 128), (4, 128)) == ("trailing", 512) and form((5, 2, 16, 32), (16, 32)) == ("trailing", 512)
    assert form((7, 257), (257,)) == ("trailing", 257) and form((7, 257), (1, 257)) == ("trailing", 257)
    assert form((7, 257), (7, 1)) == ("token", 257) and form((3, 2, 128), (3, 2, 1)) == ("token", 128)
    assert form((7, 257), (1,)) == ("trailing", 1) and form((7, 257), ()) == ("trailing", 1)
    assert form((1, 128), (1, 1)) == ("token", 128) and form((8,), (1,)) == ("token", 8)
    for bad in [(7,), (2, 1, 128), (4, 1)]:
        with pytest.raises(NotImplementedError):
            form((2, 4, 128), bad)


def test_golden_defines_short_counts_and_negative_counts():
    """Beyond the reference (which raises): rows at or past sum(token_count) are int8 zeros with scale 1; negative counts read as
    zero."""
    acc, act, ws, qs, bias, _ = U.swiglu_inputs(12, 64, (4, 3, 5))
    op = U.make_op(G.TorchDequantSwiGLUQuant, {"weight_scale": ws, "quant_scale": qs}, expert_num=3, hidden_size=64)
    full_q, full_scale = op.forward(acc, act, bias, None, torch.tensor([4, 3, 5]))
    q, scale = op.forward(acc, act, bias, None, torch.tensor([4, -2, 5], dtype=torch.int32))
    assert torch.equal(q[:4], full_q[:4]) and not bool(q[9:].any()) and scale[9:].flatten().tolist() == [1.0, 1.0, 1.0]
    assert not torch.equal(q[4:9], full_q[4:9])               # rows 4..8 now belong to the third expert
    assert torch.equal(scale[:4], full_scale[:4])


@pytest.mark.parametrize("quant_dtype,symmetric", [(I8, True), (I8, False), (F8, True)], ids=str)
@pytest.mark.parametrize("name", NAMES[:3])
def test_norm_tie_case_puts_the_golden_on_the_analytic_ties(name, quant_dtype, symmetric):
    """The precondition of the GPU rounding-boundary test: on `norm_tie_case` the golden's statistics are exact, its scale is
    2^-4 and its q is round-half-even of the k + 0.5 the case constructs."""
    for dtype in (BF16, F32):
        state, kw, args, expected = U.norm_tie_case(name, quant_dtype, symmetric, dtype)
        op = U.make_op(U.golden_cls(name), state, norm_size=args[0].shape[-1], **kw)
        with torch.no_grad():
            out = op.forward(*args)
        assert bool((out[-1] == 2.0 ** -4).all())
        assert bit_equal(out[0], expected)
        assert int((expected.float() % 2 == 0).sum()) > expected.numel() // 3          # halves went to the even neighbour


# ---- the room the GPU tests' inputs leave for their bound ------------------------------------------------------------------
ROOM_SHARE, ROOM_SCALE = 2e-4, 1e-6


@pytest.mark.parametrize("dtype", U.NORM_DTYPES, ids=str)
@pytest.mark.parametrize("shape", U.SWEEP_SHAPES, ids=str)
def test_norm_inputs_leave_room_for_the_gpu_bound(shape, dtype):
    """fp32 golden against the float64 restatement (statistics in float64, rounded to fp32) on the inputs of the GPU sweep: q
    within one step on at most 2e-4 of the elements, a tenth of the GPU cap; scales within 1e-6 relative."""
    x, r, w, b, smooth = U.norm_inputs(shape, dtype)
    dim = shape[-1]
    with torch.no_grad():
        for sm in (None, smooth):
            ln = U.make_op(G.TorchLayerNormQuant, {"weight": w, "bias": b}, norm_size=dim)
            rms = U.make_op(G.TorchRMSNormQuant, {"weight": w}, norm_size=dim)
            pairs = [(ln.forward(x, sm), U.layernorm_quant_f64(x, w, b, sm, 1e-5, -128, 127, I8)),
                     (ln.forward(x + r, sm), U.layernorm_quant_f64(x + r, w, b, sm, 1e-5, -128, 127, I8)),
                     (rms.forward(x, sm), U.rmsnorm_quant_f64(x, w, sm, 1e-5, -128, 127, I8))]
            for (q, scale), (q64, scale64) in pairs:
                worst, share = U.q_difference(q, q64)
                rel = U.scale_rel_error(scale, scale64)
                print(f"{shape} {dtype} smooth {sm is not None}: max step {worst}, share {share:.2e}, scale rel {rel:.2e}")
                assert worst <= 1 and share <= ROOM_SHARE and rel <= ROOM_SCALE


@pytest.mark.parametrize("case", U.SWIGLU_SWEEP, ids=str)
def test_swiglu_inputs_leave_room_for_the_gpu_bound(case):
    tokens, hidden, counts = case
    acc, act, ws, qs, bias, token_count = U.swiglu_inputs(tokens, hidden, None if counts is None else tuple(counts))
    experts = ws.shape[0]
    with torch.no_grad():
        for left in (False, True):
            op = U.make_op(G.TorchDequantSwiGLUQuant, {"weight_scale": ws, "quant_scale": qs}, expert_num=experts, hidden_size=hidden,
                           activate_left=left)
            for b in (None, bias):
                q, scale = op.forward(acc, act, b, None, token_count)
                q64, scale64 = U.swiglu_quant_f64(acc, act, ws, qs, b, token_count, left)
                worst, share = U.q_difference(q, q64)
                rel = U.scale_rel_error(scale, scale64)
                print(f"{case} left {left} bias {b is not None}: max step {worst}, share {share:.2e}, scale rel {rel:.2e}")
                assert worst <= 1 and share <= ROOM_SHARE and rel <= ROOM_SCALE
