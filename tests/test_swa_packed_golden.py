"""Packed var-len attention over contiguous K/V (`MojoSWA`) without a GPU: the golden against the recorded reference outputs
and against the paged prefill golden on the same tokens, dispatch and registration, `PACKED_ATTN_OPS`, the plugin,
constructor and forward errors, and the C workspace query.

The recorded outputs (tests/make_swa_packed_golden.py) are one file under the 1 MiB bound of a committed file."""
import os
import types

import pytest
import torch

import mojo_opset_amd as mo
import oracle.swa
import swa_packed_golden
from conftest import GOLDEN, build_op, clone_tree, load_golden
from mojo_opset_amd.core import MojoOperator
from mojo_opset_amd.core.platform import get_platform
from swa_packed_utils import packed_inputs, scatter_to_pages

NAME = "MojoSWA"
CASES = load_golden("swa_packed")
IDS = [pytest.param(c, id=str(i)) for i, c in enumerate(CASES)]


@pytest.mark.parametrize("case", IDS)
def test_golden_reproduces_the_reference_bit_for_bit(case):
    op = build_op(swa_packed_golden.TorchSWA, case)
    out = op.forward(*clone_tree(case["args"]), **clone_tree(case["kwargs"]))
    assert torch.equal(out, case["out"])


def test_fixture_is_small_and_covers_the_envelope():
    assert os.path.getsize(os.path.join(GOLDEN, "swa_packed.pt")) < 1 << 20
    assert 8 <= len(CASES) <= 12
    kw = [c["ctor"]["kwargs"] for c in CASES]
    assert {k["gqa_layout"] for k in kw} == {"ABAB", "AABB"}
    assert {c["args"][0].dtype for c in CASES} == {torch.bfloat16, torch.float16}
    assert {c["args"][0].shape[2] for c in CASES} == {64, 96, 128}
    assert {c["args"][0].shape[1] // c["args"][1].shape[1] for c in CASES} == {1, 2, 4, 8}
    windows = {(k["global_window_size"] is not None, k["local_window_size"] is not None) for k in kw}
    assert windows == {(False, False), (True, False), (False, True), (True, True)}
    assert any(k["local_window_size"] == 0 for k in kw)
    starts = [s for c in CASES for s in c["args"][4].tolist()[1:-1]]
    assert any(s % 4 for s in starts) and all(any(s % m for s in starts) for m in (16, 64))
    assert any(c["args"][4][0] > 0 for c in CASES) and any(c["args"][4][-1] < c["args"][1].shape[0] for c in CASES)
    for c in CASES:
        q, k, _, cu_q, cu_kv = c["args"]
        q_lens, kv_lens = cu_q[1:] - cu_q[:-1], cu_kv[1:] - cu_kv[:-1]
        assert bool((q_lens >= 1).all()) and bool((kv_lens >= q_lens).all()) and int(cu_q[-1]) == q.shape[0]
    assert any(bool((c["args"][3][1:] - c["args"][3][:-1] == c["args"][4][1:] - c["args"][4][:-1]).any()) and
               bool((c["args"][3][1:] - c["args"][3][:-1] < c["args"][4][1:] - c["args"][4][:-1]).any()) for c in CASES)

    def plain(x):
        if isinstance(x, (list, tuple)):
            return all(plain(v) for v in x)
        if isinstance(x, dict):
            return all(isinstance(k, str) and plain(v) for k, v in x.items())
        return x is None or isinstance(x, (torch.Tensor, bool, int, float, str))
    assert plain(CASES)


@pytest.mark.parametrize("page", [16, 64])
@pytest.mark.parametrize("case", IDS)
def test_golden_is_the_paged_prefill_golden_on_the_same_tokens(case, page):
    """The same tokens scattered into pages, through `oracle.swa.TorchPagedPrefillSWA`: the same bits (what the exact
    linear-against-paged GPU test stands on)."""
    q, k, v, cu_q, cu_kv = case["args"]
    kc, vc, table, cu0 = scatter_to_pages(k, v, cu_kv, page)
    paged = oracle.swa.TorchPagedPrefillSWA(**case["ctor"]["kwargs"])
    packed = build_op(swa_packed_golden.TorchSWA, case)
    assert torch.equal(paged.forward(q, kc, vc, cu_q, table, cu_total_seq_lens=cu0), packed.forward(q, k, v, cu_q, cu_kv))


def test_golden_defines_empty_sequences_and_padding_rows_as_zeros():
    q, k, v, cu_q, cu_kv = packed_inputs([9, 0, 0, 20], [9, 4, 0, 3], hq=2, hkv=1, d=64, q_pad=5, lead=2, tail=2)
    out = swa_packed_golden.TorchSWA(local_window_size=3).forward(q, k, v, cu_q, cu_kv)
    assert not bool(out[9:13].any()) and not bool(out[16:].any())
    assert bool(out[:9].any()) and bool(out[13:16].any())


def test_dispatch_registers_torch_and_hip():
    core = getattr(mo, NAME)
    assert core.get_backend_impl("torch", strict=True) is swa_packed_golden.TorchSWA
    from mojo_opset_amd.backends import hip

    assert issubclass(hip.HIPSWA, core)
    if get_platform() == "rocm":
        assert core.get_backend_impl("hip", strict=True) is hip.HIPSWA


def test_packed_attn_ops_is_a_set_of_its_own():
    assert tuple(mo.PACKED_ATTN_OPS) == (NAME,) and tuple(mo.core.PACKED_ATTN_OPS) == (NAME,)
    assert getattr(mo, NAME).__name__ == NAME and getattr(mo.core, NAME) is getattr(mo, NAME) and NAME not in mo.__all__
    for other in (mo.EXTENDED_OPS, mo.KV_INT8_OPS, mo.KV_INT8_SWA_OPS, mo.QUANT_MOE_OPS, mo.SAMPLING_OPS,
                  mo.BEYOND_SURVEY_OPS, mo.NSTEP_OPS, mo.NSTEP_KV_INT8_OPS):
        assert NAME not in other
    assert len(mo.BEYOND_SURVEY_OPS) == 16


def test_constructor_and_repr_follow_the_reference():
    cls = swa_packed_golden.TorchSWA
    op = cls(gqa_layout="ABAB", global_window_size=4, local_window_size=255)
    assert (op.is_causal, op.gqa_layout, op.gqa_interleave, op.global_window_size, op.local_window_size) == \
        (True, "ABAB", True, 4, 255)
    assert op.extra_repr() == "is_causal=True, gqa_layout=ABAB, global_window_size=4, local_window_size=255"
    op = cls()
    assert (op.is_causal, op.gqa_layout, op.gqa_interleave, op.global_window_size, op.local_window_size) == \
        (True, "AABB", False, None, None)
    with pytest.raises(ValueError, match="gqa_layout"):
        cls(gqa_layout="BBAA")


def _me(**kw):
    base = dict(is_causal=True, gqa_layout="AABB", gqa_interleave=False, global_window_size=None, local_window_size=None)
    return types.SimpleNamespace(**{**base, **kw})


def test_host_refusals_need_no_gpu():
    from mojo_opset_amd.backends.hip import HIPSWA
    from mojo_opset_amd.backends.hip.lib import MojoHipError

    q, k, v, cu_q, cu_kv = packed_inputs([5], [5], hq=2, hkv=1, d=64)
    for cls in (HIPSWA, swa_packed_golden.TorchSWA):
        with pytest.raises(AssertionError):
            cls.forward(_me(), q, k, v, cu_q.long(), cu_kv)
        with pytest.raises(AssertionError):
            cls.forward(_me(), q, k, v, cu_q, cu_kv.long())
        with pytest.raises(AssertionError):
            cls.forward(_me(), q, k, v, cu_q, cu_kv[:-1])
        with pytest.raises(AssertionError):
            cls.forward(_me(), q, k, v[:, :, :32], cu_q, cu_kv)
        with pytest.raises(AssertionError):
            cls.forward(_me(), q, k.float(), v.float(), cu_q, cu_kv)
    with pytest.raises(NotImplementedError, match="causal"):
        HIPSWA.forward(_me(is_causal=False), q, k, v, cu_q, cu_kv)
    for glob, local in [(0, None), (-1, 4), (None, -3)]:
        with pytest.raises(ValueError):
            HIPSWA.forward(_me(global_window_size=glob, local_window_size=local), q, k, v, cu_q, cu_kv)
    with pytest.raises(MojoHipError, match="CPU tensor"):
        HIPSWA.forward(_me(), q, k, v, cu_q, cu_kv)


def test_rebase_registers_the_class_into_a_stand_in_reference():
    """`plugin.rebase_hip_backend` walks ``PACKED_ATTN_OPS`` too; the class is in the reference's core package."""
    import sys

    from mojo_opset_amd import plugin
    from mojo_opset_amd.backends import hip

    ref = types.ModuleType("stand_in_packed_reference")

    def ctor(self, is_causal=True, gqa_layout="AABB", global_window_size=None, local_window_size=None):
        MojoOperator.__init__(self)
        self.is_causal, self.gqa_layout = is_causal, gqa_layout
        self.gqa_interleave = gqa_layout == "ABAB"
        self.global_window_size, self.local_window_size = global_window_size, local_window_size

    core = type(NAME, (MojoOperator,), {"__init__": ctor, "forward": lambda self, *a, **k: None, "__module__": ref.__name__})
    setattr(ref, NAME, core)
    sys.modules[ref.__name__] = ref
    try:
        made = plugin.rebase_hip_backend(ref, platforms=["rocm", "cpu"])
    finally:
        del sys.modules[ref.__name__]
    cls = made[NAME]
    assert cls.__name__ == "HIPSWA" and issubclass(cls, core)
    assert cls.forward is hip.HIPSWA.forward
    assert "__init__" not in vars(cls)
    if get_platform() == "rocm":
        assert core.get_backend_impl("hip", strict=True) is cls


def test_workspace_query_answers_without_a_gpu():
    from mojo_opset_amd.backends.hip import lib as L

    query = L.load().mojo_hip_swa_packed_workspace_bytes
    # (Tq, Tk, batch, Hq, Hkv, D, max_q hint, max_kv hint, local, global)
    assert query(16384, 16384, 1, 32, 8, 128, 0, 0, -1, 0) == 0              # 4096 blocks: the chip is full
    assert query(8192, 8192, 4, 32, 8, 128, 2048, 2048, 4095, 0) == 0
    chunk = query(128, 6000, 1, 8, 2, 128, 0, 0, -1, 0)                      # 8 blocks of up to 94 key tiles: key split
    assert chunk > 0
    # 11 slices (6000 / 512 keys) of 8 blocks x 128 rows x (128 + 2) floats, plus the alignment slack
    assert chunk == 8 * 11 * 128 * 130 * 4 + 64
    assert query(128, 6000, 1, 8, 2, 128, 0, 1024, -1, 0) == 8 * 2 * 128 * 130 * 4 + 64    # the hint caps the capacity
    # a window: sized on the keys a block can see (4 + 1023 + 32 -> 2 slices), whatever the tensor holds
    windowed = query(128, 6000, 1, 8, 2, 128, 0, 0, 1023, 4)
    assert windowed == 8 * 2 * 128 * 130 * 4 + 64
    assert query(128, 60000, 1, 8, 2, 128, 0, 0, 1023, 4) == windowed and query(128, 60000, 1, 8, 2, 128, 0, 0, -1, 0) > chunk
    assert query(0, 0, 0, 8, 2, 128, 0, 0, -1, 0) == 0 and query(128, 0, 1, 8, 2, 128, 0, 0, -1, 0) == 0
