"""Bidirectional attention with an optional mask (`MojoSdpa`) without a GPU: the golden against the recorded reference outputs,
dispatch and registration, `FULL_ATTN_OPS`, the plugin, constructor and `extra_repr`, every refusal of `HIPSdpa.forward`
(reached before any device call) and the C workspace query.

The recorded outputs (tests/make_sdpa_golden.py) are one file under the 1 MiB bound of a committed file."""
import os
import types

import pytest
import torch

import mojo_opset_amd as mo
import sdpa_golden
from conftest import GOLDEN, build_op, clone_tree, load_golden
from mojo_opset_amd.core import MojoOperator
from mojo_opset_amd.core.platform import get_platform

NAME = "MojoSdpa"
CASES = load_golden("sdpa")
IDS = [pytest.param(c, id=f"{i}-{c['mask_form']}") for i, c in enumerate(CASES)]


@pytest.mark.parametrize("case", IDS)
def test_golden_reproduces_the_reference_bit_for_bit(case):
    op = build_op(sdpa_golden.TorchSdpa, case)
    out = op.forward(*clone_tree(case["args"]), **clone_tree(case["kwargs"]))
    assert torch.equal(out, case["out"])


@pytest.mark.parametrize("case", IDS)
def test_golden_is_the_step_by_step_attention_within_the_bound(case):
    """The fp32 restatement the GPU tests lean on for rows torch leaves undefined agrees with the library call."""
    kw = case["ctor"]["kwargs"]
    ref = sdpa_golden.reference_fp32(*case["args"], scale=kw["scale"], enable_gqa=kw["enable_gqa"])
    torch.testing.assert_close(case["out"].float(), ref, atol=2e-2, rtol=2e-2)


def test_fixture_is_small_and_covers_the_envelope():
    assert os.path.getsize(os.path.join(GOLDEN, "sdpa.pt")) < 1 << 20
    assert 8 <= len(CASES) <= 12
    shapes = [(c["args"][0].shape, c["args"][1].shape) for c in CASES]
    assert {c["args"][0].dtype for c in CASES} == {torch.bfloat16, torch.float16}
    assert {q[3] for q, _ in shapes} == {64, 96, 128}
    assert {q[1] // k[1] for q, k in shapes} == {1, 2, 4, 8}
    assert {q[0] for q, _ in shapes} == {1, 3}
    assert any(q[2] > k[2] for q, k in shapes) and any(q[2] == k[2] for q, k in shapes) and any(q[2] < k[2] for q, k in shapes)
    assert any(k[2] % 64 == 0 for _, k in shapes) and any(k[2] % 64 for _, k in shapes) and any(k[2] % 4 for _, k in shapes)
    assert {c["mask_form"] for c in CASES} == {"none", "bool_2d", "bool_b1", "key_padding", "block", "bias", "bias_fp32", "bias_inf"}
    assert {c["ctor"]["kwargs"]["scale"] for c in CASES} >= {None, 1.0} and {c["ctor"]["kwargs"]["enable_gqa"] for c in CASES} == {True, False}
    assert any(not c["args"][0].is_contiguous() for c in CASES) and any(c["args"][0].is_contiguous() for c in CASES)
    for c in CASES:
        assert bool(torch.isfinite(c["out"].float()).all())
        mask = c["args"][3]
        if mask is not None:                               # every row keeps a visible key
            seen = mask if mask.dtype == torch.bool else ~torch.isneginf(mask)
            assert bool(seen.any(dim=-1).all())
    inf_case = next(c for c in CASES if c["mask_form"] == "bias_inf")
    assert bool(torch.isneginf(inf_case["args"][3]).any())


def test_enable_gqa_groups_heads_as_repeat_interleave():
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(1, h, 7, 64, generator=g) for h in (4, 2, 2))
    grouped = sdpa_golden.TorchSdpa(enable_gqa=True).forward(q, k, v)
    spelled = sdpa_golden.TorchSdpa().forward(q, k.repeat_interleave(2, dim=1), v.repeat_interleave(2, dim=1))
    torch.testing.assert_close(grouped, spelled, atol=1e-6, rtol=1e-6)


def test_dispatch_registers_torch_and_hip():
    core = getattr(mo, NAME)
    assert core.get_backend_impl("torch", strict=True) is sdpa_golden.TorchSdpa
    from mojo_opset_amd.backends import hip

    assert issubclass(hip.HIPSdpa, core)
    if get_platform() == "rocm":
        assert core.get_backend_impl("hip", strict=True) is hip.HIPSdpa


def test_full_attn_ops_is_a_set_of_its_own():
    assert tuple(mo.FULL_ATTN_OPS) == (NAME,) and tuple(mo.core.FULL_ATTN_OPS) == (NAME,)
    assert getattr(mo, NAME).__name__ == NAME and getattr(mo.core, NAME) is getattr(mo, NAME) and NAME not in mo.__all__
    for other in (mo.EXTENDED_OPS, mo.KV_INT8_OPS, mo.KV_INT8_SWA_OPS, mo.QUANT_MOE_OPS, mo.SAMPLING_OPS,
                  mo.BEYOND_SURVEY_OPS, mo.NSTEP_OPS, mo.NSTEP_KV_INT8_OPS, mo.PACKED_ATTN_OPS, mo.QUANT_DENSE_OPS):
        assert NAME not in other


def test_constructor_and_repr_follow_the_reference():
    cls = sdpa_golden.TorchSdpa
    op = cls()
    assert (op.scale, op.enable_gqa) == (None, False)
    assert op.extra_repr() == "scale=None, enable_gqa=False"
    op = cls(scale=0.125, enable_gqa=True)
    assert (op.scale, op.enable_gqa) == (0.125, True)
    assert op.extra_repr() == "scale=0.125, enable_gqa=True"
    assert cls(1.0, True).extra_repr() == "scale=1.0, enable_gqa=True"


def _me(**kw):
    return types.SimpleNamespace(**{**dict(scale=None, enable_gqa=False), **kw})


def _qkv(b=1, hq=2, hkv=2, sq=5, sk=7, d=64, dtype=torch.bfloat16):
    return (torch.zeros(b, hq, sq, d, dtype=dtype), torch.zeros(b, hkv, sk, d, dtype=dtype), torch.zeros(b, hkv, sk, d, dtype=dtype))


def test_host_refusals_need_no_gpu():
    from mojo_opset_amd.backends.hip import HIPSdpa
    from mojo_opset_amd.backends.hip.lib import MojoHipError

    fwd = HIPSdpa.forward
    q, k, v = _qkv()
    # outside the envelope
    with pytest.raises(NotImplementedError, match="dtype"):
        fwd(_me(), *_qkv(dtype=torch.float32))
    with pytest.raises(NotImplementedError, match="head_dim"):
        fwd(_me(), *_qkv(d=32))
    with pytest.raises(NotImplementedError, match="per kv head"):
        fwd(_me(enable_gqa=True), *_qkv(hq=6, hkv=2))
    with pytest.raises(NotImplementedError, match="per kv head"):
        fwd(_me(enable_gqa=True), *_qkv(hq=16, hkv=1))
    with pytest.raises(NotImplementedError, match="four dimensions"):
        fwd(_me(), q[None], k[None], v[None])
    with pytest.raises(NotImplementedError, match="mask dtype"):
        fwd(_me(), q, k, v, torch.zeros(5, 7, dtype=torch.float16))      # neither bool, the query's dtype nor fp32
    with pytest.raises(NotImplementedError, match="mask dtype"):
        fwd(_me(), q, k, v, torch.zeros(5, 7, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="mask of 5"):
        fwd(_me(), q, k, v, torch.ones(1, 1, 1, 5, 7, dtype=torch.bool))
    # shape errors: RuntimeError, the type torch's own shape checks raise
    with pytest.raises(RuntimeError, match="query heads"):
        fwd(_me(), *_qkv(hq=4, hkv=2))                                    # unequal head counts without enable_gqa
    with pytest.raises(RuntimeError, match="query heads"):
        fwd(_me(enable_gqa=True), *_qkv(hq=3, hkv=2))
    with pytest.raises(RuntimeError, match="do not match"):
        fwd(_me(), q, k, v[:, :, :6])
    with pytest.raises(RuntimeError, match="do not match"):
        fwd(_me(), q, k[..., :32], v[..., :32])
    with pytest.raises(RuntimeError, match="do not match"):
        fwd(_me(), q, torch.cat([k, k]), torch.cat([v, v]))
    with pytest.raises(RuntimeError, match="share a dtype"):
        fwd(_me(), q, k.half(), v.half())
    with pytest.raises(RuntimeError, match="all"):
        fwd(_me(), q, k[0], v[0])
    with pytest.raises(RuntimeError, match="broadcastable"):
        fwd(_me(), q, k, v, torch.ones(5, 6, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="broadcastable"):
        fwd(_me(), q, k, v, torch.ones(3, 1, 5, 7, dtype=torch.bool))
    # inside the envelope: the call reaches the device check, and nothing before it touched a device
    for mask in (None, torch.ones(5, 7, dtype=torch.bool), torch.zeros(1, 2, 5, 7), torch.zeros(1, 1, 1, 7, dtype=torch.bfloat16)):
        with pytest.raises(MojoHipError, match="CPU tensor"):
            fwd(_me(), q, k, v, mask)
    with pytest.raises(MojoHipError, match="CPU tensor"):
        fwd(_me(enable_gqa=True), q[0], k[0, :1], v[0, :1])               # 3-D: one batch entry


def test_rebase_registers_the_class_into_a_stand_in_reference():
    """`plugin.rebase_hip_backend` walks ``FULL_ATTN_OPS`` too; the class is in the reference's core package."""
    import sys

    from mojo_opset_amd import plugin
    from mojo_opset_amd.backends import hip

    ref = types.ModuleType("stand_in_sdpa_reference")

    def ctor(self, scale=None, enable_gqa=False):
        MojoOperator.__init__(self)
        self.scale, self.enable_gqa = scale, enable_gqa

    core = type(NAME, (MojoOperator,), {"__init__": ctor, "forward": lambda self, *a, **k: None, "__module__": ref.__name__})
    setattr(ref, NAME, core)
    sys.modules[ref.__name__] = ref
    try:
        made = plugin.rebase_hip_backend(ref, platforms=["rocm", "cpu"])
    finally:
        del sys.modules[ref.__name__]
    cls = made[NAME]
    assert cls.__name__ == "HIPSdpa" and issubclass(cls, core)
    assert cls.forward is hip.HIPSdpa.forward
    assert "__init__" not in vars(cls)
    if get_platform() == "rocm":
        assert core.get_backend_impl("hip", strict=True) is cls


def test_workspace_query_answers_without_a_gpu():
    from mojo_opset_amd.backends.hip import lib as L

    query = L.load().mojo_hip_sdpa_workspace_bytes
    # (batch, Hq, Hkv, Sq, Sk, D)
    assert query(1, 40, 40, 8192, 8192, 128) == 0                          # 2560 blocks: the chip is full
    assert query(1, 40, 40, 32760, 512, 128) == 0
    chunk = query(1, 8, 2, 128, 6000, 128)                                 # 8 blocks of 94 key tiles: key split
    # 11 slices (6000 / 512 keys) of 8 blocks x 128 rows x (128 + 2) floats, plus the alignment slack: the prefill's plan
    assert chunk == 8 * 11 * 128 * 130 * 4 + 64
    assert chunk == L.load().mojo_hip_swa_packed_workspace_bytes(128, 6000, 1, 8, 2, 128, 0, 0, -1, 0)
    assert query(1, 8, 2, 128, 600, 128) == 0                              # too few keys to cut
    assert query(0, 8, 2, 128, 6000, 128) == 0 and query(1, 8, 2, 0, 6000, 128) == 0 and query(1, 8, 2, 128, 0, 128) == 0

