"""The vision-tower ops (`VISION_TOWER_OPS`: packed bidirectional attention, the vision tower's 2-D rotary pair, MRoPE and its
in-place form) without a GPU: the goldens against the recorded reference outputs, the set and its wiring, dispatch and the
plugin, constructors and `extra_repr`, the contract errors of the `HIP<Op>.forward`s (reached before any device call) and the C
header.

The recorded outputs (tests/make_vision_tower_golden.py) are one file under 256 KiB."""
import os
import re
import sys
import types

import pytest
import torch

import mojo_opset_amd as mo
import vision_tower_golden as G
from conftest import GOLDEN, ROOT, bit_equal, build_op, clone_tree, load_golden
from mojo_opset_amd.core import MojoOperator
from mojo_opset_amd.core.platform import get_platform

NAMES = ("MojoPackedSdpa", "MojoVisionRotaryEmbedding2D", "MojoApplyVisionRoPE2D", "MojoMRoPE", "MojoMRoPEInplace")
CASES = load_golden("vision_tower")
IDS = [pytest.param(c, id=f"{i}-{c['op']}") for i, c in enumerate(CASES)]


@pytest.mark.parametrize("case", IDS)
def test_golden_reproduces_the_reference_bit_for_bit(case):
    op = build_op(G.GOLDENS[case["op"]], case)
    args = clone_tree(case["args"])
    out = op.forward(*args, **clone_tree(case["kwargs"]))
    assert bit_equal(out, case["out"])                                       # (dtypes included: bit_equal compares them)
    if case["op"] == "MojoMRoPEInplace" and case["ctor"]["kwargs"]["inplace"]:
        assert out[0] is args[0] and out[1] is args[1]


@pytest.mark.parametrize("case", IDS)
def test_constructor_and_repr_follow_the_recording(case):
    from mojo_opset_amd.backends import hip

    for cls in (G.GOLDENS[case["op"]], getattr(hip, "HIP" + case["op"][4:])):
        op = build_op(cls, case)
        assert list(op.parameters()) == []
        if case["op"] == "MojoPackedSdpa":
            # the reference's class for these semantics is MojoSWA(is_causal=False): its repr names the layout this op keeps
            layout = case["ctor"]["kwargs"]["gqa_layout"]
            assert case["reference_repr"] == f"is_causal=False, gqa_layout={layout}, global_window_size=None, local_window_size=None"
            assert op.extra_repr() == f"gqa_layout={layout}" and op.gqa_interleave == (layout == "ABAB")
        else:
            assert op.extra_repr() == case["repr"]


def test_fixture_is_small_and_covers_the_cases():
    assert os.path.getsize(os.path.join(GOLDEN, "vision_tower.pt")) < 256 * 1024
    assert {c["op"] for c in CASES} == set(NAMES)
    packed = [c for c in CASES if c["op"] == "MojoPackedSdpa"]
    assert {c["ctor"]["kwargs"]["gqa_layout"] for c in packed} == {"AABB", "ABAB"}
    q_lens = [(c["args"][3][1:] - c["args"][3][:-1]).tolist() for c in packed]
    kv_lens = [(c["args"][4][1:] - c["args"][4][:-1]).tolist() for c in packed]
    assert any(0 in ql for ql in q_lens)                                                        # an empty-query sequence
    assert any(a > b for ql, kl in zip(q_lens, kv_lens) for a, b in zip(ql, kl))                # q_len > kv_len
    assert any(a < b for ql, kl in zip(q_lens, kv_lens) for a, b in zip(ql, kl))                # q_len < kv_len
    assert any(len(set(ql)) > 2 for ql in q_lens) and any(int(c["args"][4][0]) > 0 for c in packed)
    grids = [(c["args"][0].tolist(), c["ctor"]["kwargs"]["adapooling_factor"]) for c in CASES if c["op"] == "MojoVisionRotaryEmbedding2D"]
    assert [g for g, f in grids if f == 1] == [[[4, 4]], [[8, 6]], [[8, 8], [4, 6]]] and any(f == 2 for _, f in grids)
    mrope = [c for c in CASES if c["op"] == "MojoMRoPE"]
    assert {c["args"][5] for c in mrope} == {True, False}                                       # interleaved and chunked
    assert any(2 * sum(c["args"][4]) < c["args"][6] for c in mrope)                              # partial rotation
    assert {c["args"][2].dim() for c in mrope} == {2, 3} and {c["args"][2].dtype for c in mrope} == {torch.float32, torch.bfloat16}
    assert {c["ctor"]["kwargs"]["inplace"] for c in CASES if c["op"] == "MojoMRoPEInplace"} == {True, False}
    # the reference's out-of-place MRoPE is fp32 for 16-bit queries with fp32 tables (torch's promotion inside cat), and the
    # in-place form stores that result rounded once
    pairs = [(a, b) for a, b in zip(CASES, CASES[1:]) if a["op"] == "MojoMRoPE" and b["op"] == "MojoMRoPEInplace"]
    assert pairs
    for out_of_place, in_place in pairs:
        if out_of_place["args"][2].dtype == torch.float32:
            assert out_of_place["out"][0].dtype == torch.float32
        assert in_place["out"][0].dtype == in_place["args"][0].dtype


def test_positions_follow_the_definition():
    """(h, w) of token i: window i // f^2 in row-major window order, patch i % f^2 row-major inside it."""
    for (gh, gw), f in (((4, 6), 2), ((8, 2), 2), ((4, 4), 4), ((3, 5), 1)):
        got = G.vision_positions([(gh, gw)], f).tolist()
        want = []
        for i in range(gh * gw):
            win, inside = divmod(i, f * f)
            bh, bw = divmod(win, gw // f)
            ih, iw = divmod(inside, f)
            want.append([bh * f + ih, bw * f + iw])
        assert got == want
        assert sorted(map(tuple, got)) == [(h, w) for h in range(gh) for w in range(gw)]       # a permutation of the grid


def test_mrope_table_choice_is_the_references_slice_assignment():
    for sec in ([24, 20, 20], [16, 24, 24], [2, 1, 3], [1, 1, 2], [8, 12, 12]):
        half = sum(sec)
        marks = torch.stack([torch.full((1, half), float(t)) for t in range(3)])               # table t holds the value t
        for inter in (False, True):
            merged, _ = G.merged_mrope_tables(marks, marks, sec, inter)
            assert merged[0].tolist() == [float(t) for t in G.mrope_table_of(half, sec, inter)]


def test_vision_tower_ops_is_a_set_of_its_own():
    assert tuple(mo.VISION_TOWER_OPS) == NAMES and tuple(mo.core.VISION_TOWER_OPS) == NAMES and tuple(mo.core.operators.VISION_TOWER_OPS) == NAMES
    others = (mo.EXTENDED_OPS, mo.KV_INT8_OPS, mo.KV_INT8_SWA_OPS, mo.QUANT_MOE_OPS, mo.SAMPLING_OPS, mo.BEYOND_SURVEY_OPS,
              mo.NSTEP_OPS, mo.NSTEP_KV_INT8_OPS, mo.PACKED_ATTN_OPS, mo.FULL_ATTN_OPS, mo.QUANT_DENSE_OPS, mo.DIT_BLOCK_OPS)
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
        assert hip_cls.__module__.endswith("operators.attention" if name == "MojoPackedSdpa" else "operators.streaming")
        if get_platform() == "rocm":
            assert core.get_backend_impl("hip", strict=True) is hip_cls


def test_rebase_registers_the_classes_the_reference_has():
    """`plugin.rebase_hip_backend` walks ``VISION_TOWER_OPS`` too: three classes are in the reference's core package,
    `MojoMRoPEInplace` in its ``experimental`` package, and `MojoPackedSdpa` is a name the reference lacks: skipped."""
    from mojo_opset_amd import plugin
    from mojo_opset_amd.backends import hip

    ref = types.ModuleType("stand_in_vision_reference")
    exp = types.ModuleType("stand_in_vision_reference.experimental")

    def make(name, where):
        core = type(name, (MojoOperator,), {"__init__": lambda self, *a, **k: MojoOperator.__init__(self),
                                            "forward": lambda self, *a, **k: None, "__module__": where.__name__})
        setattr(where, name, core)
        return core

    cores = {name: make(name, exp if name == "MojoMRoPEInplace" else ref) for name in NAMES if name != "MojoPackedSdpa"}
    sys.modules[ref.__name__], sys.modules[exp.__name__] = ref, exp
    try:
        made = plugin.rebase_hip_backend(ref, platforms=["rocm", "cpu"])
    finally:
        del sys.modules[ref.__name__], sys.modules[exp.__name__]
    assert "MojoPackedSdpa" not in made
    for name, core in cores.items():
        cls, mine = made[name], getattr(hip, "HIP" + name[4:])
        assert cls.__name__ == mine.__name__ and issubclass(cls, core)
        assert cls.forward is mine.forward and "__init__" not in vars(cls)
    assert made["MojoVisionRotaryEmbedding2D"].check_grid_contract is hip.HIPVisionRotaryEmbedding2D.check_grid_contract


def test_constructor_and_contract_errors_need_no_gpu():
    from mojo_opset_amd.backends import hip
    from mojo_opset_amd.backends.hip.lib import MojoHipError

    # ---- packed attention
    for cls in (mo.MojoPackedSdpa, hip.HIPPackedSdpa, G.TorchPackedSdpa):
        with pytest.raises(ValueError, match="gqa_layout"):
            cls(gqa_layout="BABA")
        assert cls().gqa_layout == "AABB"
    op = hip.HIPPackedSdpa()
    q, kv = torch.zeros(6, 4, 64, dtype=torch.bfloat16), torch.zeros(9, 2, 64, dtype=torch.bfloat16)
    cu_q, cu_kv = torch.tensor([0, 2, 6], dtype=torch.int32), torch.tensor([0, 4, 9], dtype=torch.int32)
    with pytest.raises(AssertionError):
        op.forward(q, kv, kv, cu_q.long(), cu_kv)
    with pytest.raises(AssertionError):
        op.forward(q, kv, kv, cu_q, cu_kv[:2])
    with pytest.raises(AssertionError):
        op.forward(q, kv, kv.half(), cu_q, cu_kv)
    with pytest.raises(NotImplementedError, match="head_dim 80"):
        op.forward(torch.zeros(6, 4, 80, dtype=torch.bfloat16), torch.zeros(9, 2, 80, dtype=torch.bfloat16),
                   torch.zeros(9, 2, 80, dtype=torch.bfloat16), cu_q, cu_kv)
    with pytest.raises(NotImplementedError, match="3 query heads per kv head"):
        op.forward(torch.zeros(6, 6, 64, dtype=torch.bfloat16), kv, kv, cu_q, cu_kv)
    with pytest.raises(NotImplementedError, match="float32"):
        op.forward(q.float(), kv.float(), kv.float(), cu_q, cu_kv)
    with pytest.raises(MojoHipError, match="CPU tensor"):                  # inside the envelope: the device check is next
        op.forward(q, kv, kv, cu_q, cu_kv)
    # ---- the vision rotary embedding
    for cls in (mo.MojoVisionRotaryEmbedding2D, hip.HIPVisionRotaryEmbedding2D):
        with pytest.raises(AssertionError, match="divisible by 4"):
            cls(rope_dim=6)
        with pytest.raises(AssertionError, match=">= 1"):
            cls(adapooling_factor=0)
    emb = hip.HIPVisionRotaryEmbedding2D(rope_theta=10000.0, rope_dim=8, adapooling_factor=2)
    assert emb.inv_freq.dtype == torch.float32 and emb.inv_freq.shape == (2,) and "inv_freq" not in emb.state_dict()
    with pytest.raises(AssertionError, match="integer tensor"):
        emb.forward(torch.tensor([[4.0, 4.0]]))
    with pytest.raises(AssertionError, match=r"\[B, 2\]"):
        emb.forward(torch.tensor([4, 4]))
    with pytest.raises(AssertionError, match=r"\[B, 2\]"):
        emb.forward(torch.tensor([[4, 4, 4]]))
    with pytest.raises(AssertionError, match="positive"):
        emb.forward(torch.tensor([[4, 0]]))
    with pytest.raises(AssertionError, match="divisible by adapooling_factor"):
        emb.forward(torch.tensor([[4, 4], [6, 3]]))
    with pytest.raises(MojoHipError, match="CPU tensor"):                  # (inv_freq lives on the CPU here)
        emb.forward(torch.tensor([[4, 4]]))
    # ---- the vision apply
    ap = hip.HIPApplyVisionRoPE2D()
    x, t = torch.zeros(3, 2, 8, dtype=torch.bfloat16), torch.zeros(3, 8)
    with pytest.raises(AssertionError, match="3D packed"):
        ap.forward(x[None], x[None], t, t)
    with pytest.raises(AssertionError, match="full head_dim"):
        ap.forward(x, x, t[:, :4], t[:, :4])
    with pytest.raises(AssertionError, match="token count"):
        ap.forward(x, x, t[:2], t[:2])
    with pytest.raises(AssertionError, match="same shape"):
        ap.forward(x, x, t, t[:2])
    with pytest.raises(MojoHipError, match="CPU tensor"):
        ap.forward(x, x, t, t)
    # ---- MRoPE: the same ValueErrors from both classes and from the golden
    qm, km = torch.zeros(3, 4 * 16, dtype=torch.bfloat16), torch.zeros(3, 2 * 16, dtype=torch.bfloat16)
    tab = torch.zeros(3, 3, 8)
    for op in (hip.HIPMRoPE(), hip.HIPMRoPEInplace(inplace=True), G.TorchMRoPE()):
        with pytest.raises(ValueError, match="mrope_section"):
            op.forward(qm, km, tab, tab, [4, 4], False, 16)
        with pytest.raises(ValueError, match="mrope_section"):
            op.forward(qm, km, tab, tab, [2, 2, 2, 2], False, 16)
        with pytest.raises(ValueError, match="more than head_dim"):
            op.forward(qm, km, torch.zeros(3, 3, 9), torch.zeros(3, 3, 9), [3, 3, 3], False, 16)
        with pytest.raises(ValueError, match="query row width"):
            op.forward(qm[:, :60], km, tab, tab, [2, 3, 3], False, 16)
        with pytest.raises(ValueError, match="key row width"):
            op.forward(qm, km[:, :30], tab, tab, [2, 3, 3], False, 16)
        with pytest.raises(ValueError, match="token counts"):
            op.forward(qm, km[:2], tab, tab, [2, 3, 3], False, 16)
        with pytest.raises(ValueError, match="cos_table of shape"):
            op.forward(qm, km, tab[:, :2], tab[:, :2], [2, 3, 3], False, 16)
    for op in (hip.HIPMRoPE(), hip.HIPMRoPEInplace(inplace=True)):
        with pytest.raises(MojoHipError, match="CPU tensor"):
            op.forward(qm, km, tab, tab, [2, 3, 3], False, 16)


def test_header_declares_the_entry_points_and_the_plan_answers_without_a_gpu():
    from mojo_opset_amd.backends.hip import lib as L

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mojo_hip.h")).read(), flags=re.S)
    for name in ("mojo_hip_packed_sdpa", "mojo_hip_packed_sdpa_workspace_bytes", "mojo_hip_vision_rotary_2d", "mojo_hip_mrope"):
        assert re.search(r"\b" + name + r"\s*\(", header) and name in L.SIGNATURES
    lib = L.load()
    # the plan is the packed causal op's without windows: the same workspace for the same geometry
    for geom in ((16384, 16384, 16, 20, 20, 64, 0, 0), (512, 16896, 1, 32, 8, 128, 0, 0), (512, 16896, 1, 32, 8, 128, 512, 4096)):
        assert lib.mojo_hip_packed_sdpa_workspace_bytes(*geom) == lib.mojo_hip_swa_packed_workspace_bytes(*geom, -1, 0)
    assert lib.mojo_hip_packed_sdpa_workspace_bytes(512, 16896, 1, 32, 8, 128, 0, 0) > 0
    # no switch of their own
    for unit in ("packed_sdpa.hip", "vision_rope.hip", "mrope.hip"):
        text = open(os.path.join(ROOT, "mojo_opset_amd", "csrc", unit)).read()
        assert set(re.findall(r"MOJO_HIP_[A-Z0-9_]+", text)) == set()
