"""The sliding-window pair without a GPU: the golden against the recorded reference outputs, dispatch, constructor and
forward errors, `EXTENDED_OPS`, and the plugin's registration of both classes.

The recorded outputs (oracle/make_swa_golden.py) are two files, decode and prefill, each under the 1 MiB bound of a
committed file.  They hold no pages of 1024 tokens (one such page of K/V is 256 KiB at the smallest head) and no prefill
at (4, 1023); tests/test_hip_swa.py runs both against oracle/swa.py instead."""
import types

import pytest
import torch

import mojo_opset_amd as mo
import oracle.swa
from conftest import build_op, clone_tree, load_golden
from mojo_opset_amd.core import MojoOperator
from mojo_opset_amd.core.platform import get_platform

SWA_OPS = ("MojoPagedDecodeSWA", "MojoPagedPrefillSWA")
CASES = load_golden("paged_swa") + load_golden("paged_swa_prefill")


@pytest.mark.parametrize("case", [pytest.param(c, id=f"{c['op'][4:]}-{i}") for i, c in enumerate(CASES)])
def test_golden_reproduces_the_reference_bit_for_bit(case):
    op = build_op(getattr(oracle.swa, "Torch" + case["op"][4:]), case)
    out = op.forward(*clone_tree(case["args"]), **clone_tree(case["kwargs"]))
    assert torch.equal(out, case["out"])


def test_fixtures_cover_the_layouts_and_windows():
    seen = {(c["ctor"]["kwargs"]["gqa_layout"], c["ctor"]["kwargs"]["global_window_size"],
             c["ctor"]["kwargs"]["local_window_size"]) for c in CASES}
    assert {("AABB", 4, 1023), ("ABAB", 4, 255), ("AABB", None, 0), ("ABAB", None, 17), ("AABB", 8, None)} <= seen


@pytest.mark.parametrize("name", SWA_OPS)
def test_dispatch_registers_torch_and_hip(name):
    core = getattr(mo, name)
    assert core.get_backend_impl("torch", strict=True).__name__ == "Torch" + name[4:]
    from mojo_opset_amd.backends import hip

    hip_cls = getattr(hip, "HIP" + name[4:])
    assert issubclass(hip_cls, core)
    if get_platform() == "rocm":
        assert core.get_backend_impl("hip", strict=True) is hip_cls


def test_extended_ops_are_attributes_but_not_in_all():
    assert tuple(mo.EXTENDED_OPS) == SWA_OPS
    for name in SWA_OPS:
        assert name not in mo.__all__ and getattr(mo, name).__name__ == name


@pytest.mark.parametrize("name", SWA_OPS)
def test_constructor_and_repr_follow_the_reference(name):
    cls = getattr(oracle.swa, "Torch" + name[4:])
    op = cls(gqa_layout="ABAB", global_window_size=4, local_window_size=255)
    assert (op.is_causal, op.gqa_layout, op.gqa_interleave, op.global_window_size, op.local_window_size) == \
        (True, "ABAB", True, 4, 255)
    assert op.extra_repr() == "is_causal=True, gqa_layout=ABAB, global_window_size=4, local_window_size=255"
    with pytest.raises(ValueError):
        cls(gqa_layout="BBAA")


def _decode_inputs():
    q = torch.zeros(1, 2, 64, dtype=torch.bfloat16)
    k = torch.zeros(2, 1, 16, 64, dtype=torch.bfloat16)
    return q, k, k.clone(), torch.tensor([5], dtype=torch.int32), torch.tensor([[0, -1]], dtype=torch.int32)


@pytest.mark.parametrize("windows", [(0, None), (-1, 4), (None, -3)])
def test_degenerate_windows_raise_before_any_device_work(windows):
    """``global_window_size=0`` alone, or a negative size, leaves rows with no visible key (the golden returns NaN):
    the hip forward raises on the host, from Python ints — it needs neither a GPU nor a sync."""
    from mojo_opset_amd.backends.hip import HIPPagedDecodeSWA, HIPPagedPrefillSWA

    glob, local = windows
    me = types.SimpleNamespace(is_causal=True, gqa_layout="AABB", gqa_interleave=False, global_window_size=glob,
                               local_window_size=local)
    q, k, v, lens, table = _decode_inputs()
    with pytest.raises(ValueError):
        HIPPagedDecodeSWA.forward(me, q, k, v, lens, table)
    cu = torch.tensor([0, 1], dtype=torch.int32)
    with pytest.raises(ValueError):
        HIPPagedPrefillSWA.forward(me, q, k, v, cu, table)


def test_non_causal_prefill_is_not_implemented():
    from mojo_opset_amd.backends.hip import HIPPagedPrefillSWA

    me = types.SimpleNamespace(is_causal=False, gqa_layout="AABB", gqa_interleave=False, global_window_size=None,
                               local_window_size=8)
    q, k, v, _, table = _decode_inputs()
    with pytest.raises(NotImplementedError):
        HIPPagedPrefillSWA.forward(me, q, k, v, torch.tensor([0, 1], dtype=torch.int32), table)


def test_golden_raises_on_a_missing_first_page():
    q, k, v, lens, _ = _decode_inputs()
    op = oracle.swa.TorchPagedDecodeSWA(local_window_size=3)
    with pytest.raises(ValueError):
        op.forward(q, k, v, lens, torch.tensor([[-1, -1]], dtype=torch.int32))


def test_rebase_registers_both_classes_into_a_stand_in_reference():
    """`plugin.rebase_hip_backend` walks ``__all__ + EXTENDED_OPS``: a stand-in reference module whose two classes are
    core ops of a `MojoOperator` gets a ``hip`` backend for each, keeping its own constructor."""
    from mojo_opset_amd import plugin
    from mojo_opset_amd.backends import hip

    ref = types.ModuleType("stand_in_reference")

    def ctor(self, is_causal=True, gqa_layout="AABB", global_window_size=None, local_window_size=None):
        MojoOperator.__init__(self)
        self.is_causal, self.gqa_layout = is_causal, gqa_layout
        self.gqa_interleave = gqa_layout == "ABAB"
        self.global_window_size, self.local_window_size = global_window_size, local_window_size

    for name in SWA_OPS:
        core = type(name, (MojoOperator,), {"__init__": ctor, "forward": lambda self, *a, **k: None,
                                            "__module__": ref.__name__})
        setattr(ref, name, core)
    made = plugin.rebase_hip_backend(ref, platforms=["rocm", "cpu"])
    for name in SWA_OPS:
        cls = made[name]
        assert cls.__name__ == "HIP" + name[4:] and issubclass(cls, getattr(ref, name))
        assert cls.forward is getattr(hip, "HIP" + name[4:]).forward
        assert "__init__" not in vars(cls)
        if get_platform() == "rocm":                       # (elsewhere the registry ignores a "hip" class)
            assert getattr(ref, name).get_backend_impl("hip", strict=True) is cls
