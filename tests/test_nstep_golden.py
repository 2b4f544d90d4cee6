"""The n-step paged decode (`MojoPagedDecodeNstepSWA`) without a GPU: the golden against the recorded reference outputs and
against the single-step SWA golden, dispatch and registration, `NSTEP_OPS`, the plugin, constructor and forward errors, and
the C workspace query.

The recorded outputs (tests/make_nstep_golden.py) are one file under the 1 MiB bound of a committed file."""
import os
import types

import pytest
import torch

import mojo_opset_amd as mo
import nstep_golden
import oracle.swa
from conftest import GOLDEN, build_op, clone_tree, load_golden
from mojo_opset_amd.core import MojoOperator
from mojo_opset_amd.core.platform import get_platform

NAME = "MojoPagedDecodeNstepSWA"
CASES = load_golden("paged_nstep_swa")


@pytest.mark.parametrize("case", [pytest.param(c, id=str(i)) for i, c in enumerate(CASES)])
def test_golden_reproduces_the_reference_bit_for_bit(case):
    op = build_op(nstep_golden.TorchPagedDecodeNstepSWA, case)
    out = op.forward(*clone_tree(case["args"]), **clone_tree(case["kwargs"]))
    assert torch.equal(out, case["out"])


def test_fixture_is_small_and_covers_the_envelope():
    assert os.path.getsize(os.path.join(GOLDEN, "paged_nstep_swa.pt")) < 1 << 20
    kw = [c["ctor"]["kwargs"] for c in CASES]
    assert {k["gqa_layout"] for k in kw} == {"ABAB", "AABB"}
    assert {c["args"][0].dtype for c in CASES} == {torch.bfloat16, torch.float16}
    assert {c["args"][0].shape[1] for c in CASES} >= {1, 2, 3, 4}
    assert any(0 in c["args"][3].tolist() for c in CASES)
    assert any(c["args"][0].shape[1] in c["args"][3].tolist() and c["args"][0].shape[1] > 1 for c in CASES)   # len == S
    windows = {(k["global_window_size"] is not None, k["local_window_size"] is not None) for k in kw}
    assert windows == {(False, False), (True, False), (False, True), (True, True)}

    def plain(x):
        if isinstance(x, (list, tuple)):
            return all(plain(v) for v in x)
        if isinstance(x, dict):
            return all(isinstance(k, str) and plain(v) for k, v in x.items())
        return x is None or isinstance(x, (torch.Tensor, bool, int, float, str))
    assert plain(CASES)


@pytest.mark.parametrize("case", [pytest.param(c, id=str(i)) for i, c in enumerate(CASES)])
def test_step_j_is_the_single_step_golden_on_shortened_lengths(case):
    """Step j of a row of ``len`` keys is the single-step op on ``len - (S - 1 - j)`` keys, bit for bit: what the composed
    route of the hip class relies on."""
    q, k, v, lens, table = case["args"]
    single = oracle.swa.TorchPagedDecodeSWA(**case["ctor"]["kwargs"])
    steps = q.shape[1]
    for j in range(steps):
        lens_j = torch.where(lens > 0, lens - (steps - 1 - j), lens)
        assert torch.equal(single.forward(q[:, j].contiguous(), k, v, lens_j, table), case["out"][:, j])


def test_dispatch_registers_torch_and_hip():
    core = getattr(mo, NAME)
    assert core.get_backend_impl("torch", strict=True) is nstep_golden.TorchPagedDecodeNstepSWA
    from mojo_opset_amd.backends import hip

    assert issubclass(hip.HIPPagedDecodeNstepSWA, core)
    if get_platform() == "rocm":
        assert core.get_backend_impl("hip", strict=True) is hip.HIPPagedDecodeNstepSWA


def test_nstep_ops_is_a_set_of_its_own():
    assert tuple(mo.NSTEP_OPS) == (NAME,)
    assert getattr(mo, NAME).__name__ == NAME and NAME not in mo.__all__
    for other in (mo.EXTENDED_OPS, mo.KV_INT8_OPS, mo.KV_INT8_SWA_OPS, mo.QUANT_MOE_OPS, mo.SAMPLING_OPS,
                  mo.BEYOND_SURVEY_OPS):
        assert NAME not in other
    assert len(mo.BEYOND_SURVEY_OPS) == 16


def test_constructor_and_repr_follow_the_reference():
    cls = nstep_golden.TorchPagedDecodeNstepSWA
    op = cls(gqa_layout="ABAB", global_window_size=4, local_window_size=255)
    assert (op.is_causal, op.gqa_layout, op.gqa_interleave, op.global_window_size, op.local_window_size) == \
        (True, "ABAB", True, 4, 255)
    assert op.extra_repr() == "is_causal=True, gqa_layout=ABAB, global_window_size=4, local_window_size=255"
    op = cls()
    assert (op.is_causal, op.gqa_layout, op.global_window_size, op.local_window_size) == (True, "AABB", None, None)
    with pytest.raises(ValueError):
        cls(gqa_layout="BBAA")


def _inputs(steps=2):
    q = torch.zeros(1, steps, 2, 64, dtype=torch.bfloat16)
    k = torch.zeros(2, 1, 16, 64, dtype=torch.bfloat16)
    return q, k, k.clone(), torch.tensor([5], dtype=torch.int32), torch.tensor([[0, -1]], dtype=torch.int32)


def _me(**kw):
    base = dict(is_causal=True, gqa_layout="AABB", gqa_interleave=False, global_window_size=None, local_window_size=None)
    return types.SimpleNamespace(**{**base, **kw})


def test_host_refusals_need_no_gpu():
    from mojo_opset_amd.backends.hip import HIPPagedDecodeNstepSWA
    from mojo_opset_amd.backends.hip.lib import MojoHipError

    q, k, v, lens, table = _inputs()
    with pytest.raises(AssertionError, match="4D query"):
        HIPPagedDecodeNstepSWA.forward(_me(), q[:, 0], k, v, lens, table)
    with pytest.raises(AssertionError, match="4D query"):
        nstep_golden.TorchPagedDecodeNstepSWA().forward(q[:, 0], k, v, lens, table)
    with pytest.raises(NotImplementedError):
        HIPPagedDecodeNstepSWA.forward(_me(is_causal=False), q, k, v, lens, table)
    for glob, local in [(0, None), (-1, 4), (None, -3)]:
        with pytest.raises(ValueError):
            HIPPagedDecodeNstepSWA.forward(_me(global_window_size=glob, local_window_size=local), q, k, v, lens, table)
    with pytest.raises(MojoHipError, match="CPU tensor"):
        HIPPagedDecodeNstepSWA.forward(_me(), q, k, v, lens, table)


def test_golden_raises_on_a_missing_first_page():
    q, k, v, lens, _ = _inputs()
    with pytest.raises(ValueError):
        nstep_golden.TorchPagedDecodeNstepSWA().forward(q, k, v, lens, torch.tensor([[-1, -1]], dtype=torch.int32))


def test_rebase_registers_the_class_into_a_stand_in_reference():
    """`plugin.rebase_hip_backend` walks ``NSTEP_OPS`` too and looks the class up in ``<reference>.experimental``."""
    import sys

    from mojo_opset_amd import plugin
    from mojo_opset_amd.backends import hip

    ref = types.ModuleType("stand_in_nstep_reference")
    exp = types.ModuleType(ref.__name__ + ".experimental")

    def ctor(self, is_causal=True, gqa_layout="AABB", global_window_size=None, local_window_size=None):
        MojoOperator.__init__(self)
        self.is_causal, self.gqa_layout = is_causal, gqa_layout
        self.gqa_interleave = gqa_layout == "ABAB"
        self.global_window_size, self.local_window_size = global_window_size, local_window_size

    core = type(NAME, (MojoOperator,), {"__init__": ctor, "forward": lambda self, *a, **k: None, "__module__": exp.__name__})
    setattr(exp, NAME, core)
    sys.modules[ref.__name__], sys.modules[exp.__name__] = ref, exp
    try:
        made = plugin.rebase_hip_backend(ref, platforms=["rocm", "cpu"])
    finally:
        del sys.modules[ref.__name__], sys.modules[exp.__name__]
    cls = made[NAME]
    assert cls.__name__ == "HIPPagedDecodeNstepSWA" and issubclass(cls, core)
    assert cls.forward is hip.HIPPagedDecodeNstepSWA.forward
    assert "__init__" not in vars(cls)
    if get_platform() == "rocm":
        assert core.get_backend_impl("hip", strict=True) is cls


def test_workspace_query_answers_without_a_gpu():
    from mojo_opset_amd.backends.hip import lib as L

    lib = L.load()
    geom = (64, 32, 8, 128, 16, 256, 0)
    for windows in [(-1, 0), (4095, 0), (255, 4)]:
        assert lib.mojo_hip_paged_decode_nstep_workspace_bytes(*geom, *windows, 1) == \
            lib.mojo_hip_paged_decode_swa_workspace_bytes(*geom, *windows)
    one = lib.mojo_hip_paged_decode_swa_workspace_bytes(*geom, -1, 0)
    four = lib.mojo_hip_paged_decode_nstep_workspace_bytes(*geom, -1, 0, 4)
    assert four >= one > 0                                   # 16 columns per (sequence, kv head) instead of 4
    # 8 q / 1 kv heads at three steps: two blocks of steps, each with partials of its own
    assert lib.mojo_hip_paged_decode_nstep_workspace_bytes(64, 8, 1, 128, 16, 256, 0, -1, 0, 3) > 0
    # geometries of the composed route: no n-step kernel, the query says so
    assert lib.mojo_hip_paged_decode_nstep_workspace_bytes(64, 32, 8, 96, 16, 256, 0, -1, 0, 4) < 0
    assert lib.mojo_hip_paged_decode_nstep_workspace_bytes(64, 32, 8, 128, 48, 256, 0, -1, 0, 4) < 0
    assert lib.mojo_hip_paged_decode_nstep_workspace_bytes(64, 32, 1, 128, 16, 256, 0, -1, 0, 4) < 0
