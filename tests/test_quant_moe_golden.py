"""The W8A8 MoE ops without a GPU: the goldens against the recorded reference outputs (both forms of the integer product),
what the fixture must contain, dispatch and registration, `QUANT_MOE_OPS`, the plugin's registration, the constructor
contract, the host-side refusals of the hip classes and the workspace query.

The recorded outputs (oracle/make_quant_moe_golden.py) are one file under the 1 MiB bound of a committed file."""
import os
import sys
import types

import pytest
import torch

import mojo_opset_amd as mo
import oracle.quant_moe as G
from conftest import GOLDEN, bit_equal, build_op, clone_tree, load_golden
from mojo_opset_amd.core import MojoOperator
from mojo_opset_amd.core.platform import get_platform

OPS = ("MojoMoEDynamicQuant", "MojoQuantExperts", "MojoQuantMoE")
CASES = load_golden("quant_moe")
QUANT = [c for c in CASES if c["op"] == "MojoMoEDynamicQuant"]
EXPERTS = [c for c in CASES if c["op"] == "MojoQuantExperts"]
LAYER = [c for c in CASES if c["op"] == "MojoQuantMoE"]
EXPERT_KEYS = {"up_proj_weight", "down_proj_weight", "up_proj_weight_scale", "down_proj_weight_scale",
               "up_proj_quantize.inv_smooth_scale", "down_proj_quantize.inv_smooth_scale"}


def _golden(case, exact_int):
    op = build_op(getattr(G, "Torch" + case["op"][4:]), case)
    if case["op"] == "MojoQuantExperts":
        op.exact_int = exact_int
    elif case["op"] == "MojoQuantMoE":
        op.experts.exact_int = exact_int
    return op


@pytest.mark.parametrize("exact_int", [False, True])
@pytest.mark.parametrize("case", [pytest.param(c, id=f"{c['op'][4:]}-{i}") for i, c in enumerate(CASES)])
def test_golden_reproduces_the_reference_bit_for_bit(case, exact_int):
    with torch.no_grad():
        out = _golden(case, exact_int).forward(*clone_tree(case["args"]), **clone_tree(case["kwargs"]))
    assert bit_equal(out, case["out"])


def test_exact_int_refuses_data_past_its_bound():
    x = torch.full((1, 2048), -128, dtype=torch.int8)
    w = torch.full((2, 2048), 127, dtype=torch.int8)
    assert G.dot_bound(x, w) == 2048 * 128 * 127 >= G.EXACT_BOUND
    with pytest.raises(AssertionError):
        G.int_dot(x, w, True)
    assert torch.equal(G.int_dot(x[:, :512], w[:, :512], True), G.int_dot(x[:, :512], w[:, :512], False))


def test_int4_packing_round_trips():
    w = torch.randint(-8, 8, (3, 10, 6), dtype=torch.int8)
    packed = G.pack_int4(w)
    assert packed.shape == (3, 5, 6) and packed.dtype == torch.int8
    for e in range(3):
        assert torch.equal(G.unpack_int4(packed[e]), w[e])


def test_fixtures_cover_what_they_must():
    assert os.path.getsize(os.path.join(GOLDEN, "quant_moe.pt")) < (1 << 20)
    for c in CASES:                                            # tensors and scalars only
        for v in list(c["state"].values()) + list(c["args"]):
            assert isinstance(v, torch.Tensor)
    acts = {c["args"][0].dtype for c in EXPERTS + LAYER}
    assert acts == {torch.bfloat16, torch.float16}
    assert {c["args"][0].dtype for c in QUANT} == {torch.float32, torch.bfloat16, torch.float16}
    counts = [c["args"][1] for c in QUANT + EXPERTS]
    assert {t.dtype for t in counts} == {torch.int32, torch.int64}
    int8_experts = [c for c in EXPERTS if c["ctor"]["kwargs"].get("up_weight_dtype", torch.int8) == torch.int8]
    assert any(0 in c["args"][1].tolist() and sum(v > 0 for v in c["args"][1].tolist()) > 1 for c in int8_experts)   # an empty expert
    assert any(sum(v > 0 for v in c["args"][1].tolist()) == 1 and c["args"][1].numel() > 1 for c in int8_experts)    # one expert holds all
    # EP-style counts: ids over 2 * E with the upper half dropped, so fewer rows than tokens * top_k (33 * 2) survive
    assert any(0 < int(c["args"][1].sum()) < 66 and all(v > 0 for v in c["args"][1].tolist()) for c in int8_experts)
    grouped = [c["ctor"]["kwargs"] for c in EXPERTS if c["ctor"]["kwargs"].get("up_weight_dtype") == "int4"]
    assert len(grouped) == 1 and grouped[0]["down_weight_dtype"] == "int4"
    assert grouped[0]["up_quant_group_size"] > 0 and grouped[0]["down_quant_group_size"] > 0
    assert {c["ctor"]["kwargs"]["top_k"] for c in LAYER} == {2, 4}
    for c in EXPERTS:
        assert set(c["state"]) == EXPERT_KEYS
    for c in LAYER:
        assert set(c["state"]) == {"experts." + k for k in EXPERT_KEYS} | {"gating.gate_weight"}


@pytest.mark.parametrize("name", OPS)
def test_dispatch_registers_torch_and_hip(name):
    core = getattr(mo, name)
    assert core.get_backend_impl("torch", strict=True).__name__ == "Torch" + name[4:]
    from mojo_opset_amd.backends import hip

    hip_cls = getattr(hip, "HIP" + name[4:])
    assert issubclass(hip_cls, core)
    if get_platform() == "rocm":
        assert core.get_backend_impl("hip", strict=True) is hip_cls


def test_quant_moe_ops_are_attributes_but_in_no_other_set():
    assert tuple(mo.QUANT_MOE_OPS) == OPS
    for name in OPS:
        assert name not in mo.__all__ and name not in mo.EXTENDED_OPS and name not in mo.KV_INT8_OPS
        assert getattr(mo, name).__name__ == name
    assert len(mo.__all__) == len(set(mo.__all__))


def test_rebase_registers_the_three_classes_into_a_stand_in_reference():
    from mojo_opset_amd import plugin
    from mojo_opset_amd.backends import hip

    ref = types.ModuleType("stand_in_reference_quant_moe")
    sys.modules[ref.__name__] = ref
    try:
        def ctor(self, *args, **kwargs):
            MojoOperator.__init__(self)

        for name in OPS:
            setattr(ref, name, type(name, (MojoOperator,), {"__init__": ctor, "forward": lambda self, *a, **k: None,
                                                            "__module__": ref.__name__}))
        made = plugin.rebase_hip_backend(ref, platforms=["rocm", "cpu"])
        for name in OPS:
            cls = made[name]
            assert cls.__name__ == "HIP" + name[4:] and issubclass(cls, getattr(ref, name))
            assert cls.forward is getattr(hip, "HIP" + name[4:]).forward
            assert "__init__" not in vars(cls)
    finally:
        del sys.modules[ref.__name__]


def test_quantiser_constructor_and_contract():
    op = G.TorchMoEDynamicQuant(expert_num=3, input_size=16)
    assert op.inv_smooth_scale.shape == (3, 16) and op.inv_smooth_scale.force_dtype == torch.float32
    assert (op.q_max, op.q_min) == (127, -128) and set(op.state_dict()) == {"inv_smooth_scale"}
    assert op.extra_repr() == "expert_num=3, input_size=16, quant_dtype=torch.int8"
    with pytest.raises(NotImplementedError):
        G.TorchMoEDynamicQuant(3, 16, quant_dtype=torch.float8_e4m3fn)
    with torch.no_grad():
        op.inv_smooth_scale.fill_(1.0)
    x = torch.randn(4, 16)
    with pytest.raises(ValueError):
        op(x[0], torch.tensor([1, 0, 0], dtype=torch.int32))                    # one dimension
    with pytest.raises(ValueError):
        op(x, torch.tensor([[4, 0, 0]], dtype=torch.int32))                     # counts not 1-D
    with pytest.raises(TypeError):
        op(x, torch.tensor([4.0, 0, 0]))
    with pytest.raises(ValueError):
        op(x, torch.tensor([5, -1, 0], dtype=torch.int32))
    with pytest.raises(ValueError):
        op(x, torch.tensor([1, 1, 1], dtype=torch.int64))                       # sum != rows
    q, s = op(torch.zeros(2, 16), torch.tensor([2, 0, 0], dtype=torch.int32))   # amax 0: the scale becomes 1
    assert torch.equal(s, torch.ones(2, 1)) and q.dtype == torch.int8 and not q.any()


def test_experts_constructor_follows_the_reference():
    op = G.TorchQuantExperts(num_experts=3, hidden_size=8, intermediate_size=6)
    assert set(op.state_dict()) == EXPERT_KEYS
    assert op.up_proj_weight.shape == (3, 12, 8) and op.up_proj_weight.dtype == torch.int8
    assert op.down_proj_weight.shape == (3, 8, 6) and op.down_proj_weight.dtype == torch.int8
    assert "up_proj_weight" in dict(op.named_buffers()) and "up_proj_weight_scale" in dict(op.named_parameters())
    assert op.up_proj_weight_scale.shape == (3, 12) and op.up_proj_weight_scale.dtype == torch.bfloat16
    assert op.down_proj_weight_scale.shape == (3, 8) and op.down_proj_weight_scale.dtype == torch.bfloat16
    assert isinstance(op.up_proj_quantize, G.TorchMoEDynamicQuant) and op.up_proj_quantize.inv_smooth_scale.shape == (3, 8)
    assert isinstance(op.down_proj_quantize, G.TorchMoEDynamicQuant) and op.down_proj_quantize.inv_smooth_scale.shape == (3, 6)
    assert (op.qmax, op.qmin) == (127, -128)
    assert op.extra_repr() == ("num_experts=3, intermediate_size=6, hidden_size=8, quant_dtype=torch.int8, up_quant_group_size=-1, "
                               "up_weight_dtype=torch.int8, down_quant_group_size=-1, down_weight_dtype=torch.int8")
    w4 = G.TorchQuantExperts(3, 8, 6, up_quant_group_size=4, up_weight_dtype="int4", down_quant_group_size=4, down_weight_dtype="int4")
    assert w4.up_proj_weight.shape == (3, 6, 8) and w4.down_proj_weight.shape == (3, 4, 6)
    assert w4.up_proj_weight_scale.shape == (3, 12, 2) and w4.down_proj_weight_scale.shape == (3, 8, 2)
    with pytest.raises(NotImplementedError):
        G.TorchQuantExperts(3, 8, 6, activation="gelu")
    with pytest.raises(ValueError):
        G.TorchQuantExperts(3, 8, 6, quant_dtype=torch.float8_e4m3fn)
    with pytest.raises(NotImplementedError):
        G.TorchQuantExperts(3, 8, 6, up_weight_dtype=torch.int16)
    with pytest.raises(ValueError):
        G.TorchQuantExperts(3, 8, 7, down_weight_dtype="int4")


def test_layer_constructor_follows_the_reference():
    op = G.TorchQuantMoE(num_experts=6, top_k=2, hidden_size=8, intermediate_size=4, ep_size=4, ep_rank=1)
    assert set(op.state_dict()) == {"experts." + k for k in EXPERT_KEYS} | {"gating.gate_weight"}
    assert (op.num_experts_local, op.ep_start, op.ep_end, op.dp_input, op._use_fused_moe) == (2, 2, 4, False, False)
    assert op.experts.up_proj_weight.shape[0] == 2 and op.gating.gate_weight.shape == (8, 6)
    assert isinstance(op.experts, G.TorchQuantExperts) and type(op.gating).__name__ == "TorchMoEGating"
    with pytest.raises(NotImplementedError):
        G.TorchQuantMoE(4, 2, 8, 4, activation="gelu")
    with pytest.raises(NotImplementedError):
        G.TorchQuantMoE(4, 2, 8, 4, quant_dtype=torch.float8_e4m3fn)
    with pytest.raises(ValueError):
        G.TorchQuantMoE(4, 2, 8, 4, up_weight_dtype=torch.int16)
    with pytest.raises(ValueError):
        G.TorchQuantMoE(4, 2, 8)


def test_layer_shares_the_orchestration_of_the_bf16_layer():
    from mojo_opset_amd.backends.hip import HIPQuantMoE

    for cls in (G.TorchQuantMoE, HIPQuantMoE):
        assert "compose_forward" in cls.forward.__code__.co_names
    assert "compose_forward" not in vars(mo.MojoQuantMoE)


def test_hip_classes_refuse_what_is_not_built_on_the_host():
    from mojo_opset_amd.backends.hip import HIPMoEDynamicQuant, HIPQuantExperts
    from mojo_opset_amd.backends.hip import lib as L

    with pytest.raises(NotImplementedError):
        HIPQuantExperts(2, 8, 6, up_weight_dtype="int4")
    with pytest.raises(NotImplementedError):
        HIPQuantExperts(2, 8, 6, down_weight_dtype="int4")
    with pytest.raises(NotImplementedError):
        HIPQuantExperts(2, 8, 6, up_quant_group_size=4)
    with pytest.raises(NotImplementedError):
        HIPQuantExperts(2, 8, 6, down_quant_group_size=2)
    ok = HIPQuantExperts(2, 8, 6)
    me = types.SimpleNamespace(inv_smooth_scale=torch.ones(2, 8))
    x = torch.zeros(3, 8, dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        HIPMoEDynamicQuant.forward(me, x, torch.tensor([3.0, 0.0]))
    with pytest.raises(ValueError):
        HIPMoEDynamicQuant.forward(me, x[0], torch.tensor([1, 0], dtype=torch.int32))
    with pytest.raises(NotImplementedError):
        HIPMoEDynamicQuant.forward(me, x.double(), torch.tensor([3, 0], dtype=torch.int32))
    with pytest.raises(L.MojoHipError):                      # no CPU path: refused before any device work
        ok(x, torch.tensor([3, 0], dtype=torch.int32))
    with pytest.raises(NotImplementedError):
        ok(x.float(), torch.tensor([3, 0], dtype=torch.int32))


def test_workspace_query_answers_without_a_gpu():
    from mojo_opset_amd.backends.hip import lib as L

    lib = L.load()
    prefix = lib.mojo_hip_group_quant_gemm_workspace_bytes(16384, 4096, 28672, 8)        # prefill: no K split, prefix arrays only
    assert 2 * 9 * 4 <= prefix <= 1024 and prefix % 16 == 0
    few = lib.mojo_hip_group_quant_gemm_workspace_bytes(512, 4096, 256, 2)                # few tiles over a long K: int32 slabs
    assert few >= 2 * 512 * 256 * 4
    assert lib.mojo_hip_group_quant_gemm_workspace_bytes(0, 4096, 256, 2) <= 1024
