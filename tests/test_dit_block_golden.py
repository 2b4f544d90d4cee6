"""The DiT block ops (`DIT_BLOCK_OPS`: LayerNorm, residual-add LayerNorm, GELU, SiLU, grid RoPE) without a GPU: the goldens
against the recorded reference outputs, the set and its wiring, dispatch and the plugin, constructors and `extra_repr`, every
refusal of the `HIP<Op>.forward`s (reached before any device call) and the C header.

The recorded outputs (tests/make_dit_block_golden.py) are one small file, well under tests/golden/sdpa.pt."""
import os
import re
import sys
import types

import pytest
import torch

import dit_block_golden as G
import mojo_opset_amd as mo
from conftest import GOLDEN, ROOT, bit_equal, build_op, clone_tree, load_golden
from mojo_opset_amd.core import MojoOperator
from mojo_opset_amd.core.platform import get_platform

NAMES = ("MojoLayerNorm", "MojoResidualAddLayerNorm", "MojoGelu", "MojoSilu", "MojoGridRoPE")
CASES = load_golden("dit_block")
IDS = [pytest.param(c, id=f"{i}-{c['op']}-{str(c['args'][0].dtype)[6:]}") for i, c in enumerate(CASES)]


@pytest.mark.parametrize("case", IDS)
def test_golden_reproduces_the_reference_bit_for_bit(case):
    op = build_op(G.GOLDENS[case["op"]], case)
    out = op.forward(*clone_tree(case["args"]), **clone_tree(case["kwargs"]))
    assert bit_equal(out, case["out"])


@pytest.mark.parametrize("case", IDS)
def test_constructor_state_and_repr_follow_the_recording(case):
    op = build_op(G.GOLDENS[case["op"]], case)
    assert op.extra_repr() == case["repr"]
    assert sorted(n for n, _ in op.named_parameters()) == sorted(case["state"])
    for name, value in case["state"].items():
        assert getattr(op, name).dtype == value.dtype and getattr(op, name).shape == value.shape
    # the backend class shares the constructor: same attributes, same repr
    from mojo_opset_amd.backends import hip

    hip_op = build_op(getattr(hip, "HIP" + case["op"][4:]), case)
    assert hip_op.extra_repr() == case["repr"]


def test_constructor_defaults_and_checks():
    ln = G.TorchLayerNorm(16)
    assert (ln.norm_size, ln.variance_epsilon, ln.elementwise_affine) == (16, 1e-5, True)
    assert ln.weight.shape == ln.bias.shape == (16,) and ln.weight.dtype == torch.float32
    assert ln.extra_repr() == "norm_size=16, variance_epsilon=1e-05, elementwise_affine=True"
    bare = G.TorchLayerNorm(16, 1e-6, False, dtype=torch.bfloat16)
    assert bare.weight is None and bare.bias is None and list(bare.parameters()) == []
    ra = G.TorchResidualAddLayerNorm(8, dtype=torch.float16)
    assert (ra.norm_size, ra.variance_epsilon, ra.norm_pos, ra.affine) == (8, 1e-5, "pre", True)
    assert ra.weight.dtype == ra.bias.dtype == torch.float16
    assert ra.extra_repr() == "norm_size=8, variance_epsilon=1e-05, norm_pos='pre', affine=True"
    assert isinstance(G.TorchResidualAddLayerNorm(8, eps=1).variance_epsilon, float)
    with pytest.raises(ValueError, match="norm_pos"):
        G.TorchResidualAddLayerNorm(8, norm_pos="mid")
    assert G.TorchGelu().extra_repr() == "" and G.TorchSilu().extra_repr() == "" and G.TorchGridRoPE().extra_repr() == ""
    assert list(G.TorchGridRoPE().parameters()) == []


def test_fixture_is_small_and_covers_the_ops():
    assert os.path.getsize(os.path.join(GOLDEN, "dit_block.pt")) < os.path.getsize(os.path.join(GOLDEN, "sdpa.pt")) // 3
    assert {c["op"] for c in CASES} == set(NAMES)
    for name in NAMES:
        assert {c["args"][0].dtype for c in CASES if c["op"] == name} == {torch.bfloat16, torch.float16, torch.float32}
    ln = [c for c in CASES if c["op"] == "MojoLayerNorm"]
    assert {c["ctor"]["kwargs"]["elementwise_affine"] for c in ln} == {True, False}
    assert {c["args"][0].shape[-1] for c in ln} >= {1, 2, 7, 40, 1000}
    assert {c["ctor"]["kwargs"]["norm_pos"] for c in CASES if c["op"] == "MojoResidualAddLayerNorm"} == {"pre", "post"}
    for c in CASES:
        if c["op"] == "MojoResidualAddLayerNorm":
            normed, second = c["out"]
            assert bit_equal(second, normed if c["ctor"]["kwargs"]["norm_pos"] == "post" else c["args"][0] + c["args"][1])
        if c["op"] in ("MojoGelu", "MojoSilu") and c["args"][0].dtype != torch.float32:
            x = c["args"][0].float()
            assert x.numel() == 4096 and bool(torch.isnan(x).any()) and bool(torch.isinf(x).any()) and bool((x == 0).any())
    rope = [c for c in CASES if c["op"] == "MojoGridRoPE"]
    assert {c["shared"] for c in rope} == {True, False} and 2 in {c["args"][0].shape[-1] for c in rope}
    for c in rope:
        x, grid, freqs = c["args"]
        assert all(f.dtype == torch.complex64 for f in freqs)
        assert (len({id(f) for f in freqs}) == 1) == (c["shared"] or len(freqs) == 1)
        for i, (f, h, w) in enumerate(grid.tolist()):                       # the padding tokens are the input's
            assert torch.equal(c["out"][i, f * h * w:], x[i, f * h * w:])
    assert any(len({tuple(g) for g in c["args"][1].tolist()}) > 1 for c in rope)                     # per-sample grids
    assert any(any(f * h * w == c["args"][0].shape[1] for f, h, w in c["args"][1].tolist()) for c in rope)   # no padding
    assert any(any(f * h * w == 1 for f, h, w in c["args"][1].tolist()) for c in rope)


@pytest.mark.parametrize("case", [c for c in IDS if c.values[0]["op"] in ("MojoLayerNorm", "MojoResidualAddLayerNorm")])
def test_layernorm_golden_is_the_fp64_formula_within_the_reference_tolerance(case):
    c = case
    out = c["out"][0] if isinstance(c["out"], tuple) else c["out"]
    x = c["args"][0] if len(c["args"]) == 1 else c["args"][0] + c["args"][1]
    want = G.layernorm_fp64(x, c["state"].get("weight"), c["state"].get("bias"), c["ctor"]["kwargs"]["eps"])
    sixteen = out.dtype != torch.float32
    torch.testing.assert_close(out.double(), want, atol=5e-2 if sixteen else 1e-4, rtol=1e-2 if sixteen else 1e-5)


@pytest.mark.parametrize("case", [c for c in IDS if c.values[0]["op"] in ("MojoGelu", "MojoSilu")])
def test_activation_golden_is_the_fp64_formula_where_fp32_does_not_cancel(case):
    """On [-2, inf) the golden is the fp64 value to two storage ulps (torch rounds an fp32 evaluation); further down the
    erf form's `1 + erf` cancels in fp32, which is why the kernel and the fp64 yardstick take erfc.  Inputs below 1e-30 in
    magnitude are left out as well: torch's CPU kernels flush the subnormal ones to zero; and so are those above 1e30: torch's
    GELU doubles before it halves and overflows from 1.7e38 on."""
    c = case
    x = c["args"][0]
    want = (G.gelu_fp64 if c["op"] == "MojoGelu" else G.silu_fp64)(x)
    keep = torch.isfinite(x.float()) & (x.float() >= -2) & ((x.float().abs() >= 1e-30) | (x.float() == 0)) & (x.float().abs() <= 1e30)
    if x.dtype == torch.float32:
        torch.testing.assert_close(c["out"][keep].double(), want[keep], atol=1e-6, rtol=1e-5)
    else:
        assert int(G.ulp_distance(c["out"][keep], want[keep]).max()) <= 2


def test_ulp_distance_counts_storage_steps():
    one = torch.tensor([1.0, -1.0, 0.0, 6e-8], dtype=torch.float16)
    assert G.ulp_distance(one, one.double()).tolist() == [0, 0, 0, 0]
    assert G.ulp_distance(one, torch.tensor([1.0 + 2 ** -10, -1.0 + 2 ** -11, -0.0, 0.0], dtype=torch.float64)).tolist() == [1, 1, 0, 1]
    assert G.ulp_distance(torch.tensor([1.0], dtype=torch.bfloat16), torch.tensor([1.0 + 2 ** -6], dtype=torch.float64)).tolist() == [2]


def test_dit_block_ops_is_a_set_of_its_own():
    assert tuple(mo.DIT_BLOCK_OPS) == NAMES and tuple(mo.core.DIT_BLOCK_OPS) == NAMES and tuple(mo.core.operators.DIT_BLOCK_OPS) == NAMES
    others = (mo.EXTENDED_OPS, mo.KV_INT8_OPS, mo.KV_INT8_SWA_OPS, mo.QUANT_MOE_OPS, mo.SAMPLING_OPS, mo.BEYOND_SURVEY_OPS,
              mo.NSTEP_OPS, mo.NSTEP_KV_INT8_OPS, mo.PACKED_ATTN_OPS, mo.FULL_ATTN_OPS, mo.QUANT_DENSE_OPS)
    for name in NAMES:
        assert getattr(mo, name).__name__ == name and getattr(mo.core, name) is getattr(mo, name)
        assert name not in mo.__all__ and name not in mo.core.__all__ and name not in mo.core.operators.__all__
        assert all(name not in other for other in others)
        assert MojoOperator in getattr(mo, name).__bases__


def test_dispatch_registers_torch_and_hip():
    from mojo_opset_amd.backends import hip

    for name in NAMES:
        core = getattr(mo, name)
        assert core.get_backend_impl("torch", strict=True) is G.GOLDENS[name]
        hip_cls = getattr(hip, "HIP" + name[4:])
        assert issubclass(hip_cls, core) and hip_cls.supported_platforms_list == ["rocm"]
        assert hip_cls.__module__.endswith("operators.streaming")
        if get_platform() == "rocm":
            assert core.get_backend_impl("hip", strict=True) is hip_cls


def test_rebase_registers_the_classes_into_a_stand_in_reference():
    """`plugin.rebase_hip_backend` walks ``DIT_BLOCK_OPS`` too: four classes are in the reference's core package, `MojoGridRoPE`
    in its ``experimental`` package."""
    from mojo_opset_amd import plugin
    from mojo_opset_amd.backends import hip

    ref = types.ModuleType("stand_in_dit_reference")
    exp = types.ModuleType("stand_in_dit_reference.experimental")

    def make(name, where):
        core = type(name, (MojoOperator,), {"__init__": lambda self, *a, **k: MojoOperator.__init__(self),
                                            "forward": lambda self, *a, **k: None, "__module__": where.__name__})
        setattr(where, name, core)
        return core

    cores = {name: make(name, exp if name == "MojoGridRoPE" else ref) for name in NAMES}
    sys.modules[ref.__name__], sys.modules[exp.__name__] = ref, exp
    try:
        made = plugin.rebase_hip_backend(ref, platforms=["rocm", "cpu"])
    finally:
        del sys.modules[ref.__name__], sys.modules[exp.__name__]
    for name in NAMES:
        cls, mine = made[name], getattr(hip, "HIP" + name[4:])
        assert cls.__name__ == mine.__name__ and issubclass(cls, cores[name])
        assert cls.forward is mine.forward and "__init__" not in vars(cls)
        if get_platform() == "rocm":
            assert cores[name].get_backend_impl("hip", strict=True) is cls


def _ln(dim=8, dtype=torch.bfloat16, affine=True, **kw):
    w = torch.ones(dim, dtype=dtype) if affine else None
    return types.SimpleNamespace(**{**dict(weight=w, bias=None if w is None else torch.zeros(dim, dtype=dtype), variance_epsilon=1e-5,
                                           norm_pos="pre"), **kw})


def test_host_refusals_need_no_gpu():
    from mojo_opset_amd.backends.hip import HIPGelu, HIPGridRoPE, HIPLayerNorm, HIPResidualAddLayerNorm, HIPSilu
    from mojo_opset_amd.backends.hip.lib import MojoHipError

    x = torch.zeros(3, 8, dtype=torch.bfloat16)
    # ---- the norms
    for fwd, extra in ((HIPLayerNorm.forward, ()), (HIPResidualAddLayerNorm.forward, (x,))):
        with pytest.raises(NotImplementedError, match="integer input"):
            fwd(_ln(), x.to(torch.int32), *[e.to(torch.int32) for e in extra])
        with pytest.raises(NotImplementedError, match="float64 is not supported"):
            fwd(_ln(dtype=torch.float64), x.double(), *[e.double() for e in extra])
        with pytest.raises(ValueError, match="weight length"):
            fwd(_ln(dim=7), x, *extra)
        with pytest.raises(ValueError, match="weight length"):
            fwd(_ln(bias=torch.zeros(9, dtype=torch.bfloat16)), x, *extra)
        with pytest.raises(NotImplementedError, match="activation dtype"):
            fwd(_ln(dtype=torch.float32), x, *extra)
        with pytest.raises(NotImplementedError, match="together"):
            fwd(_ln(bias=None), x, *extra)
        with pytest.raises(MojoHipError, match="CPU tensor"):                 # inside the envelope: the device check is next
            fwd(_ln(), x, *extra)
    with pytest.raises(MojoHipError, match="CPU tensor"):
        HIPLayerNorm.forward(_ln(affine=False), x.float())
    with pytest.raises(NotImplementedError, match="one shape and dtype"):
        HIPResidualAddLayerNorm.forward(_ln(), x, x.half())
    with pytest.raises(NotImplementedError, match="one shape and dtype"):
        HIPResidualAddLayerNorm.forward(_ln(), x, x[:2])
    # ---- the activations
    for fwd in (HIPGelu.forward, HIPSilu.forward):
        with pytest.raises(NotImplementedError, match="integer input"):
            fwd(None, torch.zeros(4, dtype=torch.int64))
        with pytest.raises(NotImplementedError, match="integer input"):
            fwd(None, torch.zeros(4, dtype=torch.bool))
        with pytest.raises(NotImplementedError, match="float64 is not supported"):
            fwd(None, torch.zeros(4, dtype=torch.float64))
        with pytest.raises(MojoHipError, match="CPU tensor"):
            fwd(None, torch.zeros(4, dtype=torch.float16))
    # ---- grid RoPE
    me = types.SimpleNamespace(check_shape_contract=HIPGridRoPE.check_shape_contract)
    fwd = HIPGridRoPE.forward
    xr = torch.zeros(2, 9, 2, 8, dtype=torch.bfloat16)
    grid = torch.tensor([[1, 2, 4], [1, 2, 4]])
    freqs = [torch.ones(8, 1, 4, dtype=torch.complex64)] * 2
    with pytest.raises(AssertionError, match="even"):
        fwd(me, xr[..., :7], grid, freqs)
    with pytest.raises(AssertionError, match=r"\[B, 3\]"):
        fwd(me, xr, grid[:, :2], freqs)
    with pytest.raises(AssertionError, match=r"\[B, 3\]"):
        fwd(me, xr, grid[0], freqs)
    with pytest.raises(AssertionError, match="4D"):
        fwd(me, xr[0], grid, freqs)
    with pytest.raises(AssertionError, match="per sample"):
        fwd(me, xr, grid, freqs[:1])
    with pytest.raises(NotImplementedError, match="integer input"):
        fwd(me, xr.to(torch.int16), grid, freqs)
    with pytest.raises(NotImplementedError, match="float64 is not supported"):
        fwd(me, xr.double(), grid, freqs)
    with pytest.raises(NotImplementedError, match="integer tensor"):
        fwd(me, xr, grid.float(), freqs)
    with pytest.raises(NotImplementedError, match="complex64"):
        fwd(me, xr, grid, [f.to(torch.complex128) for f in freqs])
    with pytest.raises(NotImplementedError, match="complex64"):
        fwd(me, xr, grid, [f.real for f in freqs])
    with pytest.raises(ValueError, match="is not"):
        fwd(me, xr, grid, [torch.ones(8, 1, 3, dtype=torch.complex64)] * 2)
    with pytest.raises(ValueError, match="10 cells"):                        # more cells than tokens
        fwd(me, xr, torch.tensor([[1, 2, 4], [1, 2, 5]]), [torch.ones(10, 1, 4, dtype=torch.complex64)] * 2)
    with pytest.raises(ValueError, match="9 cells"):                         # more cells than the entry has rows
        fwd(me, xr, torch.tensor([[1, 2, 4], [1, 3, 3]]), freqs)
    with pytest.raises(MojoHipError, match="CPU tensor"):
        fwd(me, xr, grid, freqs)


def test_header_declares_the_entry_points_and_the_cache_table_answers_without_a_gpu():
    from mojo_opset_amd.backends.hip import lib as L

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mojo_hip.h")).read(), flags=re.S)
    for name in ("mojo_hip_layernorm", "mojo_hip_activation", "mojo_hip_grid_rope", "mojo_hip_layernorm_cache_vectors"):
        assert re.search(r"\b" + name + r"\s*\(", header) and name in L.SIGNATURES
    assert L.load().mojo_hip_layernorm_cache_vectors() == 4
    # no switch of their own: the new units read the shared streaming switch only
    for unit in ("layernorm.hip", "activation.hip", "grid_rope.hip"):
        text = open(os.path.join(ROOT, "mojo_opset_amd", "csrc", unit)).read()
        assert set(re.findall(r"MOJO_HIP_[A-Z0-9_]+", text)) == set()
